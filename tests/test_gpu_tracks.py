"""GPU: the track state (include/pcr.h section A5, pcr_amd/tracks.py, ReIDNet.track_step) against the numpy array form
of tests/track_ref.py.  Every comparison with the restatement is bit for bit, the distance included: the build's sqrtf
is the correctly rounded one (as numpy's float32 sqrt), so no 1-ulp allowance is needed."""
import numpy as np
import pytest
import torch

import nms_ref as NR
import track_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_state(got, want, what=""):
    for k in R.STATE:
        assert same_bits(host(got[k]), want[k]), "%s: state[%r] differs" % (what, k)


def run_plan(st, fr, **args):
    """the kernel IN PLACE on a device copy of st -> (state dict of device tensors, src, det_slot, det_id)"""
    from pcr_amd import tracks as T
    C, D = len(st["ids"]), len(fr["labels"])
    d = {k: dev(v) for k, v in st.items()}
    src = torch.full((C,), 99, dtype=torch.int32, device="cuda")
    det_slot, det_id = (torch.full((D,), 99, dtype=torch.int32, device="cuda") for _ in range(2))
    T.plan(d, dev(fr["track_to_det"]), dev(fr["det_to_track"]), dev(fr["labels"]), dev(fr["lengths"]), dev(fr["boxes"]),
           dev(fr["scores"]), src, det_slot, det_id, born=dev(fr["born"]), kill=dev(fr["kill"]),
           carry=dev(args.pop("carry", None)), **args)
    return d, src, det_slot, det_id


def check_plan(st, fr, **args):
    want, w_src, w_slot, w_id = R.plan_frame(R.copy_state(st), fr, **args)
    got, src, det_slot, det_id = run_plan(st, fr, **args)
    assert_state(got, want)
    assert same_bits(host(src), w_src) and same_bits(host(det_slot), w_slot) and same_bits(host(det_id), w_id)
    return want, w_src, w_slot


# ---- 1. plan ---------------------------------------------------------------------------------------------------------------
# (C, D, share of active slots, share of valid detections, share of active slots that are matched): between them they cross the 64-entry ballot word on the slot
# side and on the detection side, (64, 0) has no detection, (1000, 24) more than one wave's worth of words.  The shares
# leave more free slots than births, so nothing is dropped here.
PLAN_SHAPES = [(1, 1, 0.0, 1.0, 1.0), (1, 1, 1.0, 1.0, 1.0), (70, 67, 0.3, 0.6, 0.6), (130, 3, 0.6, 0.85, 0.02),
               (64, 0, 0.6, 0.85, 0.6), (1000, 24, 0.6, 0.85, 0.02)]


@pytest.mark.parametrize("masks", [True, False])
@pytest.mark.parametrize("C,D,p_active,p_valid,p_match", PLAN_SHAPES)
def test_plan_in_place_equals_the_restatement(C, D, p_active, p_valid, p_match, masks):
    for W, seed in ((9, 1), (7, 2)):
        g = np.random.default_rng([C, D, seed, int(masks)])
        st = R.random_state(g, C, W, p_active)
        fr = R.make_frame(g, st, D, W, masks=masks, p_valid=p_valid, p_match=p_match)
        carry = R.rigid(g)[0] if seed == 1 else None
        want, src, det_slot = check_plan(st, fr, carry=carry, frame_limit=3, reset_on_match=seed == 2)
        assert want["info"][0] == 0, "the case drops a birth: it belongs to the overflow test"
        if C >= 64:
            assert ((st["ids"] >= 0) & (want["ids"] < 0)).any()                  # some track died
        if C >= 64 and D >= 20:
            assert (src >= 0).any() and ((det_slot >= 0) & (st["ids"][np.maximum(det_slot, 0)] < 0)).any()   # a birth


def test_plan_flags_replace_all_and_no_propagation():
    g = np.random.default_rng(8)
    st = R.random_state(g, 70, 9, 0.5)
    fr = R.make_frame(g, st, 30, 9, p_valid=0.7)
    a = check_plan(st, fr, frame_limit=10, replace_all=True)[1]
    b = check_plan(st, fr, frame_limit=10, replace_all=False, propagate=False)[1]
    assert (a >= 0).sum() > (b >= 0).sum()                   # replace_all moves features that the length rule keeps


@pytest.mark.parametrize("case", ["all_free", "none_free", "fewer_free_than_births"])
def test_plan_reports_dropped_births(case):
    g = np.random.default_rng(4)
    C, D, p_active = {"all_free": (8, 20, 0.0), "none_free": (70, 30, 1.0), "fewer_free_than_births": (70, 40, 0.9)}[case]
    st = R.random_state(g, C, 9, p_active)
    fr = R.make_frame(g, st, D, 9, masks=False, p_match=0.1)
    n_free = int((st["ids"] < 0).sum())
    assert {"all_free": n_free == C, "none_free": n_free == 0, "fewer_free_than_births": 0 < n_free < D // 2}[case]
    want, src, det_slot = check_plan(st, fr, frame_limit=3)
    assert want["info"][0] > 0 and want["next_id"][0] == st["next_id"][0] + n_free
    assert ((det_slot >= 0) & (st["ids"][np.maximum(det_slot, 0)] < 0)).sum() == n_free


# ---- 2. move ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [((64, 128), (128, 3)), ((3, 5), (5, 3))])
def test_move_copies_the_named_rows_and_nothing_else(rows):
    from pcr_amd import tracks as T
    g = np.random.default_rng(6)
    C, D = 9, 5
    fs, xs = rows
    feats, xyz = g.standard_normal((C,) + fs).astype(np.float32), g.standard_normal((C,) + xs).astype(np.float32)
    det_f, det_x = g.standard_normal((D,) + fs).astype(np.float32), g.standard_normal((D,) + xs).astype(np.float32)
    src = np.array([2, -1, D, 0, 4, -5, D + 7, 4, 1], np.int32)                  # -1, D and beyond: the row keeps its bits
    want_f, want_x = R.move(src, det_f, det_x, feats, xyz)
    assert not same_bits(want_f, feats) and same_bits(want_f[[1, 2, 5, 6]], feats[[1, 2, 5, 6]])
    got_f, got_x = dev(feats), dev(xyz)
    T.move(dev(src), dev(det_f), dev(det_x), got_f, got_x)
    assert same_bits(host(got_f), want_f) and same_bits(host(got_x), want_x)
    # the same rows from a view that starts one float into its storage: the row size allows 16 bytes, the pointer does not
    n = det_f.size
    store = torch.zeros(n + 1, device="cuda")
    store[1:].copy_(dev(det_f).reshape(-1))
    view = store[1:].view((D,) + fs)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got_f, got_x = dev(feats), dev(xyz)
    T.move(dev(src), view, dev(det_x), got_f, got_x)
    assert same_bits(host(got_f), want_f) and same_bits(host(got_x), want_x)


# ---- 3. distance and propagation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_carry", [True, False])
@pytest.mark.parametrize("W", [9, 7])
def test_distance_and_propagation_bit_for_bit(W, with_carry):
    from pcr_amd import tracks as T
    g = np.random.default_rng([W, int(with_carry)])
    C, D = 70, 67
    st = R.random_state(g, C, W, 0.7)                        # coordinates to +-100
    dets = R.det_boxes(g, D, W)
    carry, carry_inv = R.rigid(g) if with_carry else (None, None)
    want = R.dist(st["boxes"], st["ids"], dets, carry_inv)
    got = host(T.distances(dev(st["boxes"]), dev(st["ids"]), dev(dets), dev(carry_inv)))
    assert same_bits(got, want)
    free = st["ids"] < 0
    assert free.any() and (got[free] == 0).all() and (got[~free] > 0).all() and got.max() > 100.0
    # every active track is missed and survives: its centre is propagated
    fr = R.make_frame(g, st, D, W, masks=False, junk=False, p_match=0.0)
    fr["labels"][:] = -1                                     # no births either
    want_st = check_plan(st, fr, carry=carry, frame_limit=100)[0]
    moved = ~free
    # (without a velocity and without a motion of the sensor the centre stays where it is)
    assert same_bits(want_st["boxes"][moved, :2], st["boxes"][moved, :2]) == (W == 7 and not with_carry)
    assert same_bits(want_st["boxes"][moved, 3:], st["boxes"][moved, 3:]) and same_bits(want_st["boxes"][free], st["boxes"][free])


# ---- 4. a sequence, eager and from one captured graph ------------------------------------------------------------------------
FEAT, THRESH, LIMIT = (3, 5), 0.1, 3


def sequence(C, D, W, frames, seed):
    """the frames and, after each, what the restatement holds: (frame, det feats, det xyz, carry, carry_inv, dist,
    det_slot, det_id, suppressed, state, feats, xyz)"""
    g = np.random.default_rng(seed)
    st = R.new_state(C, W)
    feats, xyz = np.zeros((C,) + FEAT, np.float32), np.zeros((C, FEAT[1], 3), np.float32)
    out = []
    for f in range(frames):
        fr = R.make_frame(g, st, D, W, p_valid=0.9, span=15.0)                   # crowded: the track NMS has work
        det_f = g.standard_normal((D,) + FEAT).astype(np.float32)
        det_x = g.standard_normal((D, FEAT[1], 3)).astype(np.float32)
        carry, carry_inv = R.rigid(g, span=1.0)
        dist = R.dist(st["boxes"], st["ids"], fr["boxes"], carry_inv)
        st, src, det_slot, det_id = R.plan_frame(st, fr, carry=carry, frame_limit=LIMIT)
        feats, xyz = R.move(src, det_f, det_x, feats, xyz)
        score = (st["steps"].astype(np.float32) + st["scores"]).astype(np.float32)
        sup = NR.track_nms(NR.nearest_bev(st["boxes"][:, :7]), st["labels"], score, THRESH).astype(np.int32)
        before = st
        st = R.retire(sup, st)
        out.append(dict(fr=fr, det_f=det_f, det_x=det_x, carry=carry, carry_inv=carry_inv, dist=dist, det_slot=det_slot,
                        det_id=det_id, sup=sup, st=st, feats=feats, xyz=xyz, dropped=int(st["info"][0]),
                        retired=int(((before["ids"] >= 0) & (st["ids"] < 0)).sum())))
    return out


def test_twelve_frames_eager_and_replayed_from_one_graph():
    from pcr_amd import tracks as T
    C, D, W = 40, 30, 9
    seq = sequence(C, D, W, 12, seed=12)
    assert sum(s["dropped"] > 0 for s in seq) >= 2 and sum(s["dropped"] == 0 for s in seq) >= 2     # capacity pressure
    assert sum(s["retired"] for s in seq) >= 3                                   # the track NMS retires tracks
    bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)
    names = ("track_to_det", "det_to_track", "labels", "lengths", "boxes", "scores", "born", "kill")
    S = {k: dev(seq[0]["fr"][k]) for k in names}                                # the static inputs of the capture
    S.update(det_f=dev(seq[0]["det_f"]), det_x=dev(seq[0]["det_x"]), carry=dev(seq[0]["carry"]),
             carry_inv=dev(seq[0]["carry_inv"]))

    def load(s):
        for k in names:
            S[k].copy_(dev(s["fr"][k]))
        for k in ("det_f", "det_x", "carry", "carry_inv"):
            S[k].copy_(dev(s[k]))

    def step():
        dist = bank.distances(S["boxes"], S["carry_inv"])
        det_slot, det_id, info = bank.update(
            (S["track_to_det"], S["det_to_track"]),
            dict(labels=S["labels"], lengths=S["lengths"], boxes=S["boxes"], scores=S["scores"], feats=S["det_f"], xyz=S["det_x"]),
            born=S["born"], kill=S["kill"], carry=S["carry"], frame_limit=LIMIT)
        return dist, det_slot, det_id, bank.suppress(THRESH)

    def snapshot(outs):
        return [host(t).copy() for t in outs] + [host(getattr(bank, k)).copy() for k in R.STATE] + \
               [host(bank.feats).copy(), host(bank.xyz).copy(), host(bank.track_scores()).copy()]

    eager = []
    for f, s in enumerate(seq):
        load(s)
        dist, det_slot, det_id, sup = step()
        assert same_bits(host(dist), s["dist"]), f
        assert same_bits(host(det_slot), s["det_slot"]) and same_bits(host(det_id), s["det_id"]), f
        assert same_bits(host(sup), s["sup"]), f
        assert_state(bank.state(), s["st"], "frame %d" % f)
        assert same_bits(host(bank.feats), s["feats"]) and same_bits(host(bank.xyz), s["xyz"]), f
        eager.append(snapshot((dist, det_slot, det_id, sup)))
    # the same frames from ONE captured graph (the eager run above was the warm-up: nothing is loaded inside the capture)
    bank.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    load(seq[0])
    with torch.cuda.graph(graph):                            # a device-to-host copy in here would fail the capture
        outs = step()
    bank.reset()                                             # (a capture records, it does not run)
    for f, s in enumerate(seq):
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(snapshot(outs), eager[f]):
            assert same_bits(a, b), f


# ---- 5. the whole frame on the toy model -------------------------------------------------------------------------------------
def toy_frames(n_frames, n_boxes, n_pts, W, seed):
    """objects (4 x 2 x 1.5 m box clouds) that drive along their velocity, half of it per frame -> per frame the sweep
    (n_boxes * n_pts, 3), boxes (n_boxes, W), labels, scores"""
    import crops_ref as CR
    from pcr_amd import testing as PT
    g = np.random.default_rng(seed)
    objs = PT.synthetic_clouds(n_boxes, n_pts, seed=seed, kind="box").numpy()
    centre = np.stack([np.array([12.0 * m - 30.0, 9.0 * (m % 2), 0.0]) + g.uniform(-1, 1, 3) for m in range(n_boxes)])
    vel = g.uniform(-2.0, 2.0, (n_boxes, 2))
    rz = g.uniform(-np.pi, np.pi, n_boxes)
    labels = np.array([0, 1, 1, 0, 2, 1, 0, 2][:n_boxes], np.int32)
    out = []
    for f in range(n_frames):
        c = centre + f * np.concatenate([vel / 2, np.zeros((n_boxes, 1))], 1)
        boxes = np.zeros((n_boxes, W), np.float32)
        boxes[:, :3] = c - np.array([0, 0, 0.5 * 1.5 * 1.01])
        boxes[:, 3:6] = np.array([2.0, 4.0, 1.5]) * 1.01
        boxes[:, 6], boxes[:, 7:9] = rz, vel
        pts = np.concatenate([CR.to_sensor(objs[m].astype(np.float64), c[m], rz[m]) for m in range(n_boxes)])
        out.append((pts[g.permutation(len(pts))].astype(np.float32), boxes, labels, g.uniform(0.3, 1.0, n_boxes).astype(np.float32)))
    return out


def test_track_step_equals_the_pieces_driven_by_hand():
    import bench
    from pcr_amd import tracks as T
    C, D, M, W, n = 16, 8, 6, 9, 128
    model, _ = bench.build_pt_model([n, 64, 32])
    frames = toy_frames(3, M, n + 20, W, seed=31)
    bank = T.TrackBank(C, D, feat_shape=(64, n), box_width=W)
    shift = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0], np.float32)     # previous frame -> current
    back = np.array([1, 0, 0, -0.5, 0, 1, 0, 0.25, 0, 0, 1, 0], np.float32)
    pad = lambda a, fill: np.concatenate([a, np.full((D - M,) + a.shape[1:], fill, a.dtype)])
    with torch.no_grad():
        c0 = model.forward_inference_boxes(dev(frames[0][0]), dev(pad(frames[0][1], 0)[:, :7].copy()), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])                      # every call below runs at one level
        level = model.precision_level()
        got = []
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            out = model.track_step(bank, dev(pts), dev(boxes), dev(labels), dev(scores), carry=dev(shift), carry_inv=dev(back),
                                   crop_args=dict(seed=5 + f), frame_limit=LIMIT, suppress_threshold=THRESH)
            got.append(({k: host(v).copy() for k, v in out.items() if v is not None},
                        {k: host(v).copy() for k, v in bank.state().items()}, host(bank.feats).copy(), host(bank.xyz).copy()))
        # the same frames through forward_inference_boxes, associate(dist=...) and the restatement
        st = R.new_state(C, W)
        feats, xyz = np.zeros((C, 64, n), np.float32), np.zeros((C, n, 3), np.float32)
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            boxes_p, labels_p, scores_p = pad(boxes, 0), pad(labels, -1), pad(scores, 0)
            dxyz, dh, dlen = model.forward_inference_boxes(dev(pts), dev(boxes_p[:, :7].copy()), seed=5 + f)
            dist = R.dist(st["boxes"], st["ids"], boxes_p, back)
            a = model.associate(dev(feats), dev(xyz), dev(st["labels"]), dev(st["lengths"]), dh, dxyz, dev(labels_p), dlen,
                                dist=dev(dist))
            o, gst, gfeats, gxyz = got[f]
            assert same_bits(o["dist"], dist) and same_bits(o["lengths"], host(dlen))
            for k in ("pairs", "count", "logits", "cost", "info", "track_to_det", "det_to_track"):
                assert same_bits(o[k], host(a[k])), (f, k)
            st, src, det_slot, det_id = R.plan(st, host(a["track_to_det"]), host(a["det_to_track"]), labels_p, host(dlen),
                                               boxes_p, scores_p, carry=shift, frame_limit=LIMIT)
            feats, xyz = R.move(src, host(dh), host(dxyz), feats, xyz)
            score = (st["steps"].astype(np.float32) + st["scores"]).astype(np.float32)
            st = R.retire(NR.track_nms(NR.nearest_bev(st["boxes"][:, :7]), st["labels"], score, THRESH), st)
            assert same_bits(o["det_slot"], det_slot) and same_bits(o["det_id"], det_id), f
            assert same_bits(o["bank_info"], st["info"]), f
            for k in R.STATE:
                assert same_bits(gst[k], st[k]), (f, k)
            assert same_bits(gfeats, feats) and same_bits(gxyz, xyz), f
            assert (det_slot[M:] == -1).all() and (det_id[M:] == -1).all()       # the padding never joins a track
            if f == 0:
                assert det_id[:M].tolist() == list(range(M)) and (host(dlen)[:M] == n + 20).all()    # every detection is born
                assert st["info"][0] == 0
            else:
                assert int(o["count"][0]) > 0                                       # tracks and detections share classes
        assert model.precision_level() == level
    assert (st["ids"] >= 0).sum() >= M
