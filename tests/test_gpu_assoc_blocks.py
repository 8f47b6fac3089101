"""GPU: the block rule (include/pcr.h section A3; pcr_amd/associate.py linear_assignment_blocks / association_blocks;
ReIDNet.associate / track_step with by_class=True).  The kernel is compared bit for bit -- indices, duals and info -- with the
numpy restatement of tests/assoc_blocks_ref.py; the model's by_class route with the full solve on scripted frames."""
import numpy as np
import pytest
import torch

import assoc_blocks_ref as B
import assoc_ref as AR

gpu = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def float_case(R, C, seed):
    """a reference-shaped float matrix (fill off the class gate, N(0, 16) on it, N(0, 1) diagonals), cut to (R, C)"""
    n = (max(R, C) + 1) // 2
    return np.ascontiguousarray(AR.reference_case(n, n, seed)[0][:R, :C])


def solve(cost, rb, cb, G):
    from pcr_amd import associate as A
    out = A.linear_assignment_blocks(dev(cost), dev(np.asarray(rb, np.int32)), dev(np.asarray(cb, np.int32)), G,
                                     return_duals=True)
    torch.cuda.synchronize()
    return [host(x) for x in out]            # col4row, row4col, info, u, v


def assert_restated(cost, rb, cb, G, what=""):
    c4r, r4c, info, u, v = solve(cost, rb, cb, G)
    w4r, w4c, wu, wv, winfo = B.lsa_blocks(cost, rb, cb, G)
    assert same_bits(info, winfo), (what, info, winfo)
    assert same_bits(c4r, w4r) and same_bits(r4c, w4c), what
    assert same_bits(u, wu) and same_bits(v, wv), what
    return c4r, r4c, info, u, v


def both_costs(R, C, seed):
    return [("float", float_case(R, C, seed)), ("ties", AR.integer_case(R, C, 4, seed))]


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R,C", [(35, 35), (30, 41), (41, 30), (70, 100), (130, 90)])
def test_one_block_holding_everything_is_pcr_lsa(R, C):
    from pcr_amd import associate as A
    for name, cost in both_costs(R, C, seed=R + C):
        c4r, r4c, info, u, v = assert_restated(cost, np.zeros(R, np.int32), np.zeros(C, np.int32), 1, name)
        full = [host(x) for x in A.linear_assignment(dev(cost), return_duals=True)]
        assert same_bits(c4r, full[0][0]) and same_bits(r4c, full[1][0]) and same_bits(info, full[2]), name
        assert same_bits(u, full[3][0]) and same_bits(v, full[4][0]), name


def ids_of(n, sizes, seed, outside=()):
    """n ids: sizes[g] of them are g, the others cycle through `outside`; shuffled, so that blocks interleave"""
    ids = np.concatenate([np.zeros(0, np.int32)] + [np.full(s, g, np.int32) for g, s in enumerate(sizes)])
    rest = n - len(ids)
    assert rest >= 0 and (rest == 0 or outside)
    ids = np.concatenate([ids, np.resize(np.asarray(outside, np.int32), rest)]) if rest else ids
    return np.random.default_rng(seed).permutation(ids)


# (R, C, rows per block, columns per block): a block of 65 columns beside one with more rows than columns, a 1 x 1 block,
# an empty block, a block with rows but no columns and one with columns but no rows; the ids left over are -1 and G
EDGES = [(100, 110, (40, 30, 1, 0, 7, 0), (65, 12, 1, 0, 0, 5)),
         (64, 64, (64,), (64,)),                  # one full lane group
         (66, 3, (2, 60), (1, 2)),                # tall blocks: both transposed
         (5, 200, (2, 3), (130, 70)),             # wide blocks over three lane groups
         (0, 9, (), ()), (9, 0, (0, 0), (0, 0))]  # an empty side


@gpu
@pytest.mark.parametrize("R,C,rows,cols", EDGES)
def test_blocks_equal_the_restatement(R, C, rows, cols):
    G = max(len(rows), 1)
    rb, cb = ids_of(R, rows, 1, outside=(-1, G)), ids_of(C, cols, 2, outside=(G, -1, 1 << 20))
    for name, cost in both_costs(R, C, seed=7):
        c4r, r4c, info, u, v = assert_restated(cost, rb, cb, G, name)
        out_r, out_c = (rb < 0) | (rb >= G), (cb < 0) | (cb >= G)
        assert (c4r[out_r] == -1).all() and (r4c[out_c] == -1).all() and (u[out_r] == 0).all() and (v[out_c] == 0).all()
        assert (info == 0).all()
        for g in range(G):                       # the assignment stays inside its block and is as large as it can be
            got = c4r[rb == g]
            assert (cb[got[got >= 0]] == g).all() and (got >= 0).sum() == min((rb == g).sum(), (cb == g).sum())


@gpu
def test_contiguous_and_interleaved_ids_solve_the_same_sub_problems():
    cost = float_case(60, 60, seed=5)
    rb = np.arange(60, dtype=np.int32) % 3                # interleaved: block g holds rows g, g + 3, ...
    c4r, r4c, info, u, v = assert_restated(cost, rb, rb, 3)
    for g in range(3):
        idx = np.flatnonzero(rb == g)
        sub = solve(np.ascontiguousarray(cost[np.ix_(idx, idx)]), np.zeros(20, np.int32), np.zeros(20, np.int32), 1)
        assert same_bits(c4r[idx], idx[sub[0]].astype(np.int32)) and same_bits(u[idx], sub[3]) and same_bits(v[idx], sub[4])


@gpu
def test_a_block_beyond_lds_reads_global_memory_beside_staged_blocks():
    """R = C = 300: a 210 x 210 block (600 + 420 + 44 100 words) does not fit the 160 KiB and takes the gathered global
    path, the 50 x 30, 20 x 45 and 1 x 1 blocks beside it are staged"""
    rows, cols = (210, 50, 20, 1), (210, 30, 45, 1)
    rb, cb = ids_of(300, rows, 3, outside=(-1, 4)), ids_of(300, cols, 4, outside=(4, -1))
    for name, cost in both_costs(300, 300, seed=11):
        c4r, r4c, info, u, v = assert_restated(cost, rb, cb, 4, name)
        assert (info == 0).all() and (c4r[rb == 0] >= 0).all()


@gpu
def test_a_nan_fails_its_block_only_and_is_not_seen_outside_the_blocks():
    rb, cb = ids_of(40, (15, 12, 8), 5, outside=(-1,)), ids_of(50, (20, 10, 12), 6, outside=(3,))
    clean = float_case(40, 50, seed=9)
    ok = solve(clean, rb, cb, 3)
    r1, c1 = np.flatnonzero(rb == 1)[3], np.flatnonzero(cb == 1)[2]
    for bad in (np.nan, np.inf, -np.inf):
        cost = clean.copy()
        cost[r1, c1] = bad                                # inside block 1
        c4r, r4c, info, u, v = assert_restated(cost, rb, cb, 3)
        assert info.tolist() == [0, 1, 0]
        assert (c4r[rb == 1] == -1).all() and (r4c[cb == 1] == -1).all() and (u[rb == 1] == 0).all()
        for g in (0, 2):
            assert same_bits(c4r[rb == g], ok[0][rb == g]) and same_bits(v[cb == g], ok[4][cb == g])
    cost = clean.copy()
    cost[np.flatnonzero(rb == 0)[0], np.flatnonzero(cb == 2)[0]] = np.nan     # between two blocks
    cost[np.flatnonzero(rb == -1)[0], :] = np.nan                             # a row outside every block
    cost[:, np.flatnonzero(cb == 3)[0]] = np.inf                              # a column outside every block
    got = assert_restated(cost, rb, cb, 3)
    assert got[2].tolist() == [0, 0, 0]
    for a, b in zip(got, ok):
        assert same_bits(a, b)


@gpu
@pytest.mark.parametrize("reduce", [False, True])
def test_association_blocks_equal_the_restatement(reduce):
    from pcr_amd import associate as A
    tl, dl = np.array([0, 2, -1, 1, 5, 3, 2], np.int32), np.array([2, 2, 9, 0, -1], np.int32)
    for T, D in ((7, 5), (0, 5), (7, 0), (0, 0)):
        for dd in range(3):
            for td in range(3):
                de, te = (int(dd > 0), int(td > 0)) if reduce else (dd, td)
                rb, cb, G = A.association_blocks(dev(tl[:T]), dev(dl[:D]), T, D, dd, td, num_classes=3, reduce=reduce)
                wr, wc, wg = B.block_ids(tl[:T], dl[:D], T, D, de, te, num_classes=3)
                assert G == wg == 4 and same_bits(host(rb), wr) and same_bits(host(cb), wc), (T, D, dd, td)
    rb, cb, G = A.association_blocks(dev(tl.astype(np.int64)), dev(dl.astype(np.int64)), 7, 5, 1, 1, num_classes=32)
    assert G == 33 and host(rb)[:7].tolist() == [0, 2, 32, 1, 5, 3, 2]


@gpu
def test_argument_errors_raise_before_any_launch():
    from pcr_amd import associate as A
    from pcr_amd._lib import PcrError
    cost, ids = dev(np.zeros((4, 6), np.float32)), lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    with pytest.raises(PcrError, match="cost must be"):
        A.linear_assignment_blocks(cost.unsqueeze(0), ids(4), ids(6), 1)
    with pytest.raises(PcrError, match="row_block must be"):
        A.linear_assignment_blocks(cost, ids(6), ids(4), 1)
    with pytest.raises(PcrError, match="int32"):
        A.linear_assignment_blocks(cost, ids(4).long(), ids(6), 1)
    for G in (0, 34):
        with pytest.raises(PcrError, match="pcr_lsa_blocks_ok"):
            A.linear_assignment_blocks(cost, ids(4), ids(6), G)
    with pytest.raises(PcrError, match="pcr_lsa_blocks_ok"):
        A.linear_assignment_blocks(torch.zeros((1025, 2), device="cuda"), ids(1025), ids(2), 1)
    with pytest.raises(PcrError, match="out must hold"):
        A.linear_assignment_blocks(cost, ids(4), ids(6), 2, out=(ids(4), ids(6), ids(1)))
    with pytest.raises(PcrError, match="MI355X device tensor"):
        A.linear_assignment_blocks(cost.cpu(), ids(4), ids(6), 1)
    with pytest.raises(PcrError, match="labels must be"):
        A.association_blocks(ids(4), ids(6), 4, 5, 1, 1)
    with pytest.raises(PcrError, match="pcr_assoc_multi_ok"):
        A.association_blocks(ids(4), ids(6), 4, 6, 5, 0)
    for ncls in (0, 33):
        with pytest.raises(PcrError, match="pcr_assoc_multi_ok"):
            A.association_blocks(ids(4), ids(6), 4, 6, 1, 1, num_classes=ncls)
    with pytest.raises(PcrError, match="pcr_assoc_multi_ok"):
        A.association_blocks(ids(600), ids(300), 600, 300, 2, 0)                  # T + 2 D > PCR_LSA_MAX


# ---- 2. the model -----------------------------------------------------------------------------------------------------------
DEFAULT = dict(detection=("det_newborn", "det_false_positive"), tracking=())


@pytest.fixture(scope="module")
def toy():
    import test_gpu_decisions as TD
    return TD.toy()


def det_values(f, M):
    import test_gpu_decisions as TD
    return TD.det_values(f, M)


def run_frames(model, frames, bank, M, by_class, **args):
    """the scripted frames through track_step -> per frame (the returned dict, the bank's state, its features), on the host"""
    shift = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0], np.float32)
    back = np.array([1, 0, 0, -0.5, 0, 1, 0, 0.25, 0, 0, 1, 0], np.float32)
    got = []
    with torch.no_grad():
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            extra = dict(args)
            if extra.pop("decide", None):                 # the scripted detection decisions; a tracking decision dearer than a match
                names = extra.pop("names")
                extra["decisions"] = dict(names, det_values=dev(det_values(f, M)),
                                          track_values=dev(np.full((len(names["tracking"]), bank.capacity), 50.0, np.float32)))
            else:                                         # one decision per side, dearer than a match
                extra.update(track_miss=dev(np.full(bank.capacity, 6.0, np.float32)),
                             det_new=dev(np.full(bank.max_dets, 6.0, np.float32)))
            out = model.track_step(bank, dev(pts), dev(boxes), dev(labels), dev(scores), carry=dev(shift), carry_inv=dev(back),
                                   crop_args=dict(seed=5 + f), frame_limit=3, by_class=by_class, **extra)
            state = {k: host(v).copy() for k, v in bank.state().items()}
            state["feats"], state["xyz"] = host(bank.feats).copy(), host(bank.xyz).copy()
            got.append(({k: host(v).copy() for k, v in out.items()}, state))
    return got


ROUTES = {"one decision": {}, "one decision, live": dict(live_only=True),
          "default decisions": dict(decide=True, names=DEFAULT),
          "default decisions, live": dict(decide=True, names=DEFAULT, live_only=True),
          "two and one decisions": dict(decide=True, names=dict(DEFAULT, tracking=("track_false_positive",)))}


@gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_track_step_by_class_is_the_full_solve_bit_for_bit(toy, route):
    model, frames, new_bank, (C, D, M, W, n) = toy
    full = run_frames(model, frames, new_bank(), M, False, **ROUTES[route])
    blocks = run_frames(model, frames, new_bank(), M, True, **ROUTES[route])
    matched = 0
    for f, ((o0, s0), (o1, s1)) in enumerate(zip(full, blocks)):
        assert set(o1) - set(o0) == {"block_info"} and o1["block_info"].shape == (9,) and not o1["block_info"].any()
        assert o1["info"].shape == (1,) and o1["info"].dtype == np.int32
        for k in o0:
            assert same_bits(o0[k], o1[k]), (route, f, k)
        for k in s0:
            assert same_bits(s0[k], s1[k]), (route, f, k)
        matched += int((o1["det_to_track"] >= 0).sum())
    assert matched > 0                                    # the frames do associate: the comparison is not of empty maps


@gpu
def test_associate_by_class_is_the_full_solve_bit_for_bit(toy):
    model, frames, new_bank, (C, D, M, W, n) = toy
    bank = new_bank()
    run_frames(model, frames[:2], bank, M, False)                                 # a bank with tracks and free slots
    det_labels = dev(np.array([0, 1, 1, 0, 2, 1, -1, 11], np.int32))
    sets = [None, dict(DEFAULT), dict(detection=("det_newborn",), tracking=("track_false_positive", "track_false_negative"),
                                      kind="softmax"), dict(DEFAULT, tracking=("track_false_positive",), reduce=True)]
    with torch.no_grad():
        for ds in sets:
            for live in (False, True):
                args = (bank.feats, bank.xyz, bank.labels, bank.lengths, bank.det_feats, bank.det_xyz, det_labels, None)
                x = model.associate(*args, decisions=ds, live_only=live)
                y = model.associate(*args, decisions=ds, live_only=live, by_class=True)
                assert set(y) - set(x) == {"block_info"} and y["block_info"].shape == (9,)
                for k in x:
                    assert same_bits(host(x[k]), host(y[k])), (ds, live, k)
        y = model.associate(bank.feats[:0], bank.xyz[:0], bank.labels[:0], None, bank.det_feats, bank.det_xyz, det_labels, None,
                            by_class=True)
        assert host(y["block_info"]).tolist() == [0] * 9 and host(y["det_to_track"]).tolist() == [-1] * D


@gpu
def test_a_captured_frame_follows_new_labels(toy):
    """one graph, two replays: the second sees the first's tracks and detections whose labels were rewritten in place, so
    no detection may keep its own track; the full solve, run eagerly on the same inputs, is the yardstick"""
    model, frames, new_bank, (C, D, M, W, n) = toy
    pts, boxes, labels0, scores = frames[0]
    labels1 = ((labels0 + 1) % 3).astype(np.int32)
    bank, ref = new_bank(), new_bank()
    pts_d, boxes_d, labels_d, scores_d = dev(pts), dev(boxes), dev(labels0), dev(scores)
    vals = dev(det_values(0, M))
    step = lambda b, by_class: model.track_step(b, pts_d, boxes_d, labels_d, scores_d, crop_args=dict(seed=5),
                                                suppress_threshold=None, by_class=by_class,
                                                decisions=dict(DEFAULT, det_values=vals))
    later = np.array([[7.0] * M, [6.0] * M], np.float32)                         # both decisions dearer than a match
    want = []
    with torch.no_grad():
        for lab, v in ((labels0, det_values(0, M)), (labels1, later), (labels0, later)):
            labels_d.copy_(dev(lab))
            vals.copy_(dev(v))
            want.append({k: host(x).copy() for k, x in step(ref, False).items()})
        d2t = want[1]["det_to_track"][:M]                                         # the labels matter to this frame: matches,
        assert (d2t >= 0).any() and (d2t != want[0]["det_slot"][:M]).all()        # but no detection keeps its own track
        labels_d.copy_(dev(labels0))
        vals.copy_(dev(det_values(0, M)))
        step(bank, True)                                                          # the warm-up: everything is cached
        bank.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step(bank, True)
        bank.reset()
        for lab, v, w in ((labels0, det_values(0, M), want[0]), (labels1, later, want[1]), (labels0, later, want[2])):
            labels_d.copy_(dev(lab))
            vals.copy_(dev(v))
            graph.replay()
            torch.cuda.synchronize()
            for k in ("track_to_det", "det_to_track", "det_decision", "born", "det_id", "det_slot", "cost", "info"):
                assert same_bits(host(outs[k]), w[k]), k
            assert not host(outs["block_info"]).any()
