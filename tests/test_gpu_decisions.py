"""GPU: association with any set of decisions (include/pcr.h section A3, "Any set of decisions"; pcr_amd/associate.py
association_cost_multi / decode_assignment; ReIDNet.associate / track_step with decisions=) against the numpy restatement
of tests/decisions_ref.py.  The margin and reduce matrices, the chosen decisions and everything the decode returns are
compared exactly; only the softmax matrix has a tolerance."""
import numpy as np
import pytest
import torch

import assoc_ref as AR
import decisions_ref as R

gpu = pytest.mark.gpu

SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), (130, 70)]
DECISIONS = [(0, 0), (2, 0), (0, 2), (2, 1), (4, 4)]
FILL = 10000.0

# The softmax matrix is compared with the float64 restatement.  The yardstick is what float32 itself costs on THESE
# inputs: the largest deviation of torch's float32 softmax (CPU) from the float64 one over every row and column set of
# every (shape, decisions) case below, measured by f32_softmax_deviation() (test_the_softmax_bound_is_the_measured_one
# repeats the measurement).  The device's exp and its order of summation each differ from torch's by a few ulp: 4x.
SOFTMAX_F32_DEVIATION = 4.07e-7          # measured: 4.06924128e-07
SOFTMAX_TOL = 4 * SOFTMAX_F32_DEVIATION  # 1.628e-6


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def case(T, D, dd, td):
    """the inputs of one (shape, decisions) case: class-gated pairs (3 classes), logits ~ N(0, 4^2), N(0, 1) decisions"""
    return R.random_case(T, D, dd, td, seed=[T, D, dd, td])


def sets_of(logits, pairs, count, T, D, det, trk):
    """the softmax's sets as two padded matrices: rows (T, D + td), columns (T + dd, D); -inf = not in the set"""
    score = np.full((T, D), -np.inf, np.float32)
    score[pairs[:count, 0], pairs[:count, 1]] = logits[:count]
    return np.concatenate([score, trk.T], axis=1), np.concatenate([score, det], axis=0)


def f32_softmax_deviation():
    worst = 0.0
    for T, D in SHAPES:
        for dd, td in DECISIONS:
            logits, pairs, count, det, trk = case(T, D, dd, td)
            rows, cols = sets_of(logits, pairs, count, T, D, det, trk)
            for m, dim in ((rows, 1), (cols, 0)):
                m = m[np.isfinite(m).any(axis=dim)] if dim == 1 else m[:, np.isfinite(m).any(axis=dim)]
                if m.size == 0:
                    continue
                a = torch.softmax(torch.from_numpy(m), dim=dim).double()
                b = torch.softmax(torch.from_numpy(m).double(), dim=dim)
                worst = max(worst, float((a - b).abs().max()))
    return worst


def test_the_softmax_bound_is_the_measured_one():
    measured = f32_softmax_deviation()
    print("float32 softmax deviates from float64 by %.4g on the test inputs; constant %.4g, bound %.4g"
          % (measured, SOFTMAX_F32_DEVIATION, SOFTMAX_TOL))
    assert measured > 0 and 0.5 * measured <= SOFTMAX_F32_DEVIATION <= 2 * measured      # (another CPU's exp may differ a little)


def multi(logits, pairs, count, T, D, det, trk, **args):
    from pcr_amd import associate as A
    return A.association_cost_multi(dev(logits), dev(pairs), dev(np.array([count], np.int32)), T, D,
                                    dev(det) if len(det) else None, dev(trk) if len(trk) else None, **args)


def solve_and_decode(cost, T, D, dd, td, choices=None, born=-1, kill=-1):
    """the device's assignment and decode over the device's cost, and the restatement's decode of the same matrix and
    assignment copied to the host -> (got, want) dicts of numpy arrays"""
    from pcr_amd import associate as A
    assignment = A.linear_assignment(cost)
    got = A.decode_assignment(cost, assignment, T, D, dd, td, fill=FILL, choices=choices, born_decision=born,
                              kill_decision=kill)
    h = None if choices is None else (host(choices[0]), host(choices[1]))
    want = R.decode(host(cost), host(assignment[0]), host(assignment[1]), T, D, dd, td, fill=FILL, choices=h, born_dec=born,
                    kill_dec=kill, solver_info=int(assignment[2][0]))
    return {k: host(v) for k, v in got.items()}, want


def assert_decoded(got, want, what=""):
    assert sorted(got) == sorted(want)
    for k in want:
        assert same_bits(got[k], want[k]), "%s: %s differs: %s != %s" % (what, k, got[k], want[k])


# ---- 1. the matrices and the decode over every shape ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dd,td", DECISIONS)
@pytest.mark.parametrize("T,D", SHAPES)
def test_cost_and_decode_equal_the_restatement(T, D, dd, td):
    from pcr_amd import _lib, associate as A
    assert _lib.load().pcr_assoc_multi_ok(T, D, dd, td, T * D) == 1
    logits, pairs, count, det, trk = case(T, D, dd, td)
    dist = (np.random.default_rng([T, D]).random((T, D)) * 40).astype(np.float32)
    born, kill = (1 if dd > 1 else dd - 1), td - 1
    # margin, with and without the distance prior
    for dist_ in (None, dist):
        cost = multi(logits, pairs, count, T, D, det, trk, dist=dev(dist_))
        want = R.cost_multi(logits, pairs, count, T, D, det, trk, dist=dist_)
        assert tuple(cost.shape) == A.multi_shape(T, D, dd, td) and same_bits(host(cost), want)
    got, ref = solve_and_decode(cost, T, D, dd, td, born=born, kill=kill)
    assert_decoded(got, ref, "margin")
    assert ref["info"][0] == 0
    if min(T, D) >= 63:
        assert (ref["det_decision"] == 0).any() and (ref["track_decision"] == 0).any()
    # reduce: one block per side, the cheapest decision and its index
    cost, det_choice, trk_choice = multi(logits, pairs, count, T, D, det, trk, reduce=True, dist=dev(dist))
    want, w_det, w_trk = R.cost_multi(logits, pairs, count, T, D, det, trk, reduce=True, dist=dist)
    assert tuple(cost.shape) == A.multi_shape(T, D, dd, td, reduce=True) and same_bits(host(cost), want)
    assert same_bits(host(det_choice), w_det) and same_bits(host(trk_choice), w_trk)
    got, ref = solve_and_decode(cost, T, D, dd, td, choices=(det_choice, trk_choice), born=born, kill=kill)
    assert_decoded(got, ref, "reduce")
    # softmax: a tolerance on the matrix, none on the bits of two runs, none on the decisions
    cost = multi(logits, pairs, count, T, D, det, trk, kind="softmax")
    again = multi(logits, pairs, count, T, D, det, trk, kind="softmax")
    want = R.cost_multi(logits, pairs, count, T, D, det, trk, kind="softmax")
    assert same_bits(host(cost), host(again))
    assert np.array_equal(host(cost) == np.float32(FILL), want == np.float32(FILL))
    if cost.numel():
        worst = float(np.abs(host(cost).astype(np.float64) - want.astype(np.float64)).max())
        print("softmax (%d, %d) x (%d, %d): largest deviation %.3g, bound %.3g" % (T, D, dd, td, worst, SOFTMAX_TOL))
        assert worst <= SOFTMAX_TOL
    got, ref = solve_and_decode(cost, T, D, dd, td, born=born, kill=kill)
    assert_decoded(got, ref, "softmax")


@gpu
def test_one_decision_per_side_is_association_cost_bit_for_bit():
    from pcr_amd import associate as A
    for T, D in ((1, 1), (63, 65), (130, 70)):
        logits, pairs, count, det, trk = case(T, D, 1, 1)
        dist = (np.random.default_rng([D, T]).random((T, D)) * 40).astype(np.float32)
        a = A.association_cost(dev(logits), dev(pairs), dev(np.array([count], np.int32)), T, D, track_miss=dev(trk[0]),
                               det_new=dev(det[0]), dist=dev(dist))
        b = multi(logits, pairs, count, T, D, det, trk, dist=dev(dist))
        assert same_bits(host(a), host(b)) and same_bits(host(b), R.cost_multi(logits, pairs, count, T, D, det, trk, dist=dist))


@gpu
def test_counts_below_at_and_above_cap_and_an_empty_list():
    T, D, dd, td = 9, 7, 2, 1
    logits, pairs, count, det, trk = case(T, D, dd, td)
    assert 8 < count < T * D
    for cap, cnt in ((count, count - 3), (count, count), (count - 4, count), (count, 0), (0, 0)):
        lg, pr = logits[:cap].copy(), pairs[:cap].copy()
        for kind in ("margin", "softmax"):
            cost = multi(lg, pr, cnt, T, D, det, trk, kind=kind)
            want = R.cost_multi(lg, pr, cnt, T, D, det, trk, kind=kind)
            if kind == "margin":
                assert same_bits(host(cost), want), (cap, cnt)
            else:
                assert np.array_equal(host(cost) == np.float32(FILL), want == np.float32(FILL))
                assert np.abs(host(cost).astype(np.float64) - want).max() <= SOFTMAX_TOL, (cap, cnt)
            assert (host(cost)[:T, :D] != np.float32(FILL)).sum() == min(cap, cnt)
            assert_decoded(*solve_and_decode(cost, T, D, dd, td, born=1, kill=0), what=kind)


# ---- 2. the decode's paths ----------------------------------------------------------------------------------------------
def decode_given(cost, col4row, row4col, T, D, dd, td, solver_info=0):
    from pcr_amd import associate as A
    got = A.decode_assignment(dev(cost), (dev(np.asarray(col4row, np.int32)[None]), dev(np.asarray(row4col, np.int32)[None]),
                                          dev(np.array([solver_info], np.int32))), T, D, dd, td, fill=FILL, born_decision=dd - 1,
                              kill_decision=td - 1)
    want = R.decode(cost, col4row, row4col, T, D, dd, td, fill=FILL, born_dec=dd - 1, kill_dec=td - 1, solver_info=solver_info)
    got = {k: host(v) for k, v in got.items()}
    assert_decoded(got, want)
    return got


@gpu
def test_decode_void_collision_and_a_refused_problem():
    f = np.float32(FILL)
    # void: track 1 has nothing but fill; the solver must give it a fill entry
    cost = np.array([[-3.0, f, 0.25, f], [f, f, f, f]], np.float32)
    got, want = solve_and_decode(dev(cost), 2, 2, 0, 1, kill=0)
    assert_decoded(got, want)
    assert got["info"].tolist() == [0, 1, 0, 0] and got["track_decision"].tolist() == [0, 2] and got["kill"].tolist() == [0, 0]
    # collision: both forgotten tracks like detection 0 best; the sequential rule gives it to track 0
    T, D, dd, td = 2, 1, 2, 1
    cost = np.full((T + dd * D, D + td * T), f, np.float32)
    cost[0, 0], cost[1, 0], cost[0, 1], cost[1, 2], cost[2, 0], cost[3, 0] = -5.0, -4.0, 1.0, 2.0, 0.5, 0.7
    cost[2, 1], cost[2, 2], cost[3, 1], cost[3, 2] = -5.0, -4.0, -5.0, -4.0
    got = decode_given(cost, [-1, -1, 1, 2], [-1, 2, 3], T, D, dd, td)
    assert got["track_to_det"].tolist() == [0, -1] and got["track_decision"].tolist() == [0, 1]
    assert got["info"].tolist() == [0, 0, 2, 0] and got["kill"].tolist() == [0, 1]
    # a detection without a row of its own (dd = 0, D > T) stays unmatched
    got = decode_given(np.array([[-1.0, -2.0, 0.5]], np.float32), [1], [-1, 0, -1], 1, 2, 0, 1)
    assert got["det_decision"].tolist() == [1, 0] and got["info"].tolist() == [0, 0, 0, 0]
    # the solver refuses a problem that holds a NaN (info 1): nothing is assigned, nothing is born or killed
    T, D, dd, td = 6, 5, 2, 1
    logits, pairs, count, det, trk = case(T, D, dd, td)
    logits[1] = np.nan
    cost = multi(logits, pairs, count, T, D, det, trk)
    got, want = solve_and_decode(cost, T, D, dd, td, born=1, kill=0)
    assert_decoded(got, want)
    assert got["info"].tolist() == [1, 0, 0, 0] and (got["track_to_det"] == -1).all() and (got["det_decision"] == 1 + dd).all()
    assert not got["born"].any() and not got["kill"].any()


@gpu
def test_decode_repairs_on_each_side():
    """(2, 1) leaves rows unassigned (tracks can be forgotten), (1, 2) columns (detections can be): over these seeds both
    repairs run, and the device's decode equals the restatement's on each"""
    tracks = dets = 0
    for dd, td in ((2, 1), (1, 2), (3, 1), (2, 2)):
        for seed in range(8):
            T, D = 5 + seed % 4, 4 + (seed * 3) % 5
            logits, pairs, count, det, trk = R.random_case(T, D, dd, td, seed=[seed, dd, td], classes=2)
            cost = multi(logits, pairs, count, T, D, det, trk)
            got, want = solve_and_decode(cost, T, D, dd, td, born=0, kill=0)
            assert_decoded(got, want, (dd, td, seed))
            tracks, dets = tracks + int(got["info"][2]), dets + int(got["info"][3])
    assert tracks > 0 and dets > 0, (tracks, dets)


@gpu
def test_argument_errors_raise_before_any_launch():
    from pcr_amd import associate as A
    from pcr_amd._lib import PcrError
    T, D = 6, 5
    logits, pairs, count, det, trk = case(T, D, 2, 1)
    with pytest.raises(PcrError, match="distance prior"):
        multi(logits, pairs, count, T, D, det, trk, kind="softmax", dist=dev(np.zeros((T, D), np.float32)))
    with pytest.raises(PcrError, match="margin kind only"):
        multi(logits, pairs, count, T, D, det, trk, kind="softmax", reduce=True)
    with pytest.raises(PcrError, match="pcr_assoc_multi_ok"):
        multi(logits, pairs, count, T, D, np.zeros((5, D), np.float32), trk)
    with pytest.raises(PcrError, match="pcr_assoc_multi_ok"):
        multi(np.zeros(T * D + 1, np.float32), np.zeros((T * D + 1, 2), np.int32), 0, T, D, det, trk)      # cap > T * D
    with pytest.raises(PcrError, match="pcr_assoc_multi_ok"):
        multi(np.zeros(0, np.float32), np.zeros((0, 2), np.int32), 0, 600, 300, np.zeros((2, 300), np.float32),
              np.zeros((0, 600), np.float32))                                                                # T + 2 D > PCR_LSA_MAX
    cost = multi(logits, pairs, count, T, D, det, trk)
    with pytest.raises(PcrError, match="born_decision"):
        A.decode_assignment(cost, A.linear_assignment(cost), T, D, 2, 1, born_decision=2)
    with pytest.raises(PcrError, match="cost must be"):
        A.decode_assignment(cost, A.linear_assignment(cost), T, D, 2, 2)


# ---- 3. the model -----------------------------------------------------------------------------------------------------------
DEFAULT = dict(detection=("det_newborn", "det_false_positive"), tracking=())      # the reference's default set, unsorted


def toy():
    import bench
    import test_gpu_tracks as TT
    from pcr_amd import tracks as TR
    C, D, M, W, n = 16, 8, 6, 9, 128
    model, _ = bench.build_pt_model([n, 64, 32])
    frames = TT.toy_frames(3, M, n + 20, W, seed=31)
    with torch.no_grad():
        boxes0 = np.concatenate([frames[0][1], np.zeros((D - M, W), np.float32)])
        c0 = model.forward_inference_boxes(dev(frames[0][0]), dev(boxes0[:, :7].copy()), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])
    return model, frames, (lambda: TR.TrackBank(C, D, feat_shape=(64, n), box_width=W)), (C, D, M, W, n)


def det_values(f, M):
    """scripted costs (margin kind) of (det_false_positive, det_newborn) -- the sorted order -- per frame: frame 0 bears
    everything; in later frames both decisions cost 6 and 7, more than the toy head's matches (the test asserts that some match), but
    detection 1 is a false positive and detection 4 is born again, each cheaper than any match"""
    v = np.zeros((2, M), np.float32)
    v[0], v[1] = 5.0, -1.0 - 0.1 * np.arange(M)
    if f:
        v[0], v[1] = 7.0, 6.0
        v[0, 1], v[1, 4] = -50.0, -60.0
    return v


@gpu
def test_track_step_with_the_default_decisions_equals_the_pieces_driven_by_hand():
    model, frames, new_bank, (C, D, M, W, n) = toy()
    shift = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0], np.float32)
    back = np.array([1, 0, 0, -0.5, 0, 1, 0, 0.25, 0, 0, 1, 0], np.float32)
    pad = lambda a, fill: np.concatenate([a, np.full((D - M,) + a.shape[1:], fill, a.dtype)])
    a, b = new_bank(), new_bank()
    with torch.no_grad():
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            vals = dev(det_values(f, M))
            out = model.track_step(a, dev(pts), dev(boxes), dev(labels), dev(scores), carry=dev(shift), carry_inv=dev(back),
                                   crop_args=dict(seed=5 + f), frame_limit=3, suppress_threshold=0.15,
                                   decisions=dict(DEFAULT, det_values=vals))
            # the restatement's decode of this frame's matrix, fed to the second bank through the existing keywords
            cost = host(out["cost"])
            assert cost.shape == (C + 2 * D, D)
            col4row, row4col, _, _, info = AR.lsa(cost)
            want = R.decode(cost, col4row, row4col, C, D, 2, 0, born_dec=1, kill_dec=-1, solver_info=info)
            for k in ("track_to_det", "det_to_track", "det_decision", "track_decision", "born", "kill"):
                assert same_bits(host(out[k]), want[k]), (f, k)
            assert same_bits(host(out["decode_info"]), want["info"]) and want["info"].tolist() == [0, 0, 0, 0]
            boxes_p, labels_p, scores_p = dev(pad(boxes, 0)), dev(pad(labels, -1)), dev(pad(scores, 0))
            xyz, feats, lengths = model.forward_inference_boxes(dev(pts), boxes_p[:, :7].contiguous(), seed=5 + f)
            b.det_feats.copy_(feats)
            b.det_xyz.copy_(xyz)
            det_slot, det_id, bank_info = b.update((dev(want["track_to_det"]), dev(want["det_to_track"])),
                                                   dict(labels=labels_p, lengths=lengths, boxes=boxes_p, scores=scores_p),
                                                   born=dev(want["born"]), kill=dev(want["kill"]), carry=dev(shift),
                                                   frame_limit=3)
            b.suppress(0.15)
            assert same_bits(host(out["det_id"]), host(det_id)) and same_bits(host(out["det_slot"]), host(det_slot)), f
            for k, v in a.state().items():
                assert same_bits(host(v), host(b.state()[k])), (f, k)
            assert same_bits(host(a.feats), host(b.feats)) and same_bits(host(a.xyz), host(b.xyz)), f
            dd_ = want["det_decision"]
            if f == 0:
                assert dd_[:M].tolist() == [2] * M and host(det_id)[:M].tolist() == list(range(M))     # all newborn
            else:
                assert dd_[1] == 1 and dd_[4] == 2 and (dd_[:M] == 0).any()      # a false positive, a birth, matches
                assert host(det_id)[1] == -1 and host(det_id)[4] >= M
            assert (dd_[M:] != 0).all() and (host(det_id)[M:] == -1).all()       # the padding never joins a track


@gpu
def test_decisions_none_changes_nothing_and_the_errors_raise():
    from pcr_amd._lib import PcrError
    model, frames, new_bank, (C, D, M, W, n) = toy()
    a, b = new_bank(), new_bank()
    with torch.no_grad():
        for f, (pts, boxes, labels, scores) in enumerate(frames[:2]):
            args = (dev(pts), dev(boxes), dev(labels), dev(scores))
            x = model.track_step(a, *args, crop_args=dict(seed=5 + f))
            y = model.track_step(b, *args, crop_args=dict(seed=5 + f), decisions=None)
            assert sorted(x) == sorted(y) and "det_decision" not in x
            for k in x:
                assert same_bits(host(x[k]), host(y[k])), (f, k)
        args = (dev(frames[2][0]), dev(frames[2][1]), dev(frames[2][2]), dev(frames[2][3]))
        ones = torch.ones(M, dtype=torch.int32, device="cuda")
        with pytest.raises(PcrError, match="born / kill"):
            model.track_step(a, *args, decisions=dict(DEFAULT), born=ones)
        with pytest.raises(PcrError, match="det_values"):
            model.track_step(a, *args, decisions=dict(DEFAULT, det_values=torch.zeros((3, M), device="cuda")))
        with pytest.raises(PcrError, match="distance prior"):
            model.associate(a.feats, a.xyz, a.labels, a.lengths, a.det_feats, a.det_xyz, a.labels[:D], None,
                            decisions=dict(DEFAULT, kind="softmax"), dist=torch.zeros((C, D), device="cuda"))
        with pytest.raises(PcrError, match="track_miss"):
            model.track_step(a, *args, decisions=dict(DEFAULT), track_miss=torch.zeros(C, device="cuda"))
        with pytest.raises(PcrError, match="decisions must be"):
            model.track_step(a, *args, decisions=dict(DEFAULT, values=None))
        # associate with the decisions, softmax kind, on the bank's own rows: the decode is the restatement's
        out = model.associate(a.feats, a.xyz, a.labels, a.lengths, a.det_feats, a.det_xyz, dev(np.array([0, 1, 1, 0, 2, 1, -1, -1], np.int32)),
                              None, decisions=dict(detection=("det_newborn",), tracking=("track_false_positive", "track_false_negative"),
                                                   kind="softmax"))
        cost = host(out["cost"])
        assert cost.shape == (C + D, D + 2 * C)
        col4row, row4col, _, _, info = AR.lsa(cost)
        want = R.decode(cost, col4row, row4col, C, D, 1, 2, born_dec=0, kill_dec=1, solver_info=info)
        for k in ("track_to_det", "det_to_track", "det_decision", "track_decision", "born", "kill"):
            assert same_bits(host(out[k]), want[k]), k
        # an empty track side is no special case: every detection takes its decision
        out = model.associate(a.feats[:0], a.xyz[:0], a.labels[:0], None, a.det_feats, a.det_xyz, a.labels[:D], None,
                              decisions=dict(DEFAULT))
        cost = host(out["cost"])
        assert cost.shape == (2 * D, D) and out["track_to_det"].shape == (0,)
        col4row, row4col, _, _, info = AR.lsa(cost)
        want = R.decode(cost, col4row, row4col, 0, D, 2, 0, born_dec=1, solver_info=info)
        assert same_bits(host(out["det_decision"]), want["det_decision"]) and same_bits(host(out["born"]), want["born"])
        assert set(want["det_decision"].tolist()) <= {1, 2}


@gpu
def test_truth_works_unchanged_on_top_of_the_decisions():
    """truth= beside decisions= (here with a tracking decision that kills track slot 2 in frame 1) adds its own outputs and
    changes nothing else; the book is handed the decoded maps and masks, and force_truth still overrides them"""
    from pcr_amd import truth as TU
    model, frames, new_bank, (C, D, M, W, n) = toy()
    runs = []
    with torch.no_grad():
        for mode in ("plain", "truth", "forced"):
            bank = new_bank()
            book = TU.TruthBook(bank, D, 32) if mode != "plain" else None
            got = []
            for f, (pts, boxes, labels, scores) in enumerate(frames):
                trk = np.full((1, C), 50.0, np.float32)                          # dearer than two matches
                dv = det_values(0, M) if f == 0 else np.array([[7.0] * M, [6.0] * M], np.float32)
                if f == 1:
                    trk[0, 2] = -70.0                                            # track_false_positive, cheaper than its match
                truth = dict(book=book, boxes=dev(boxes), labels=dev(labels), ids=dev(np.arange(M, dtype=np.int32) + 3),
                             tte=dev(np.full(M, len(frames) - 1 - f, np.int32))) if book is not None else None
                out = model.track_step(bank, dev(pts), dev(boxes), dev(labels), dev(scores), crop_args=dict(seed=5 + f),
                                       frame_limit=3, truth=truth, force_truth=mode == "forced",
                                       decisions=dict(DEFAULT, tracking=("track_false_positive",),
                                                      det_values=dev(dv), track_values=dev(trk)))
                got.append(({k: host(v).copy() for k, v in out.items()}, {k: host(v).copy() for k, v in bank.state().items()}))
            runs.append(got)
    for f, ((o0, st0), (o1, st1), (o2, st2)) in enumerate(zip(*runs)):
        assert set(o1) - set(o0) == {"det_gt", "true_track_to_det", "true_det_to_track", "det_truth", "track_truth"}
        for k in o0:
            assert same_bits(o0[k], o1[k]), (f, k)
        for k in st0:
            assert same_bits(st0[k], st1[k]), (f, k)
        assert o0["cost"].shape == (C + 2 * D, D + C)
        if f == 1:
            assert o0["track_decision"][2] == 1 and o0["kill"][:M].tolist() == [int(s == 2) for s in range(M)]
            assert st0["ids"][2] != 2                                            # the slot's track was killed
            assert o2["kill"][2] == 1 and st2["ids"][2] == 2                     # forced: reported, but the truth keeps it alive
        for k in ("det_decision", "track_decision", "born", "kill", "decode_info"):
            assert k in o2


@gpu
def test_a_captured_frame_follows_new_decision_values():
    model, frames, new_bank, (C, D, M, W, n) = toy()
    bank = new_bank()
    pts, boxes, labels, scores = (dev(x) for x in frames[0])
    vals = dev(det_values(0, M))
    step = lambda: model.track_step(bank, pts, boxes, labels, scores, crop_args=dict(seed=5), suppress_threshold=None,
                                    decisions=dict(DEFAULT, det_values=vals))
    with torch.no_grad():
        eager = {k: host(v).copy() for k, v in step().items()}                   # the warm-up: everything is cached
        assert eager["det_decision"][:M].tolist() == [2] * M
        bank.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        bank.reset()
        graph.replay()
        torch.cuda.synchronize()
        for k in ("det_decision", "born", "det_id", "cost"):
            assert same_bits(host(outs[k]), eager[k]), k
        bank.reset()
        new = det_values(0, M)
        new[0, 2], new[1, 2] = -9.0, 9.0                                         # detection 2 is now a false positive
        vals.copy_(dev(new))
        graph.replay()
        torch.cuda.synchronize()
        assert host(outs["det_decision"])[:M].tolist() == [2, 2, 1, 2, 2, 2]
        assert host(outs["born"])[:M].tolist() == [1, 1, 0, 1, 1, 1] and host(outs["det_id"])[:M].tolist() == [0, 1, -1, 2, 3, 4]
