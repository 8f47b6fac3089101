"""GPU: scoring against ground truth (include/pcr.h section A7, pcr_amd/truth.py, ReIDNet.track_step(truth=...)) against
the numpy array form of tests/truth_ref.py.  Every comparison with the restatement is bit for bit, the cost included:
the build's sqrtf is the correctly rounded one (as numpy's float32 sqrt), and the assignment is pcr_lsa_f32's, which
equals assoc_ref.lsa bit for bit."""
import numpy as np
import pytest
import torch

import nms_ref as NR
import track_ref as TR
import truth_ref as R

pytestmark = pytest.mark.gpu

OUTPUTS = ("det_gt", "true_t2d", "true_d2t", "det_truth", "track_truth")
BOOK = ("slot_gt", "slot_tte", "gt_last", "stats")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def gpu_cost(c, kind):
    """the cost on the device (through nearest_bev + iou_bev for the IoU kind) and the restatement's -> (device, numpy)"""
    from pcr_amd import nms as N
    from pcr_amd import truth as T
    iou_d = iou_h = None
    if kind == "iou":
        iou_d = N.iou_bev(N.nearest_bev(dev(c["det_boxes"][:, :7])), N.nearest_bev(dev(c["gt_boxes"][:, :7])), kind="axis")
        iou_h = NR.iou_axis(NR.nearest_bev(c["det_boxes"][:, :7]), NR.nearest_bev(c["gt_boxes"][:, :7])).astype(np.float32)
        iou_h = iou_h.reshape(len(c["det_labels"]), len(c["gt_labels"]))
    got = T.cost(dev(c["det_boxes"]), dev(c["det_labels"]), dev(c["gt_boxes"]), dev(c["gt_labels"]), dev(c["gt_ids"]), c["gt_cap"],
                 iou=iou_d)
    return got, R.cost(c["det_boxes"], c["det_labels"], c["gt_boxes"], c["gt_labels"], c["gt_ids"], c["gt_cap"], iou=iou_h)


def run_frame(c, kind, thresh, skip_empty=True, forced=False):
    """cost, assignment, decide, (the restatement's plan and a retirement), record on the device and by the restatement;
    asserts bit equality at every step -> the restatement's (book, outputs)"""
    from pcr_amd import associate as A
    from pcr_amd import truth as T
    st, fr, gt_cap = c["st"], c["fr"], c["gt_cap"]
    C, D, G = len(st["ids"]), len(c["det_labels"]), len(c["gt_labels"])
    cost_d, cost_h = gpu_cost(c, kind)
    assert same_bits(host(cost_d), cost_h)
    col_d, row_d, info_d = A.linear_assignment(cost_d)
    col, row, info = R.lsa_maps(cost_h)
    assert same_bits(host(col_d[0]), col) and same_bits(host(row_d[0]), row) and same_bits(host(info_d), info)
    want_book, want = R.decide(c["book"], st["ids"], col, row, info, cost_h, thresh, c["gt_labels"], c["gt_ids"], gt_cap,
                               c["det_labels"], fr["track_to_det"], fr["det_to_track"], fr["born"], fr["kill"],
                               skip_empty=skip_empty, forced=forced)
    t = {k: dev(c["book"][k]) for k in BOOK}
    t.update(ids=dev(st["ids"]), col4row=col_d[0].contiguous(), row4col=row_d[0].contiguous(), info=info_d, cost=cost_d,
             thresh=dev(np.array([thresh], np.float32)), gt_labels=dev(c["gt_labels"]), gt_ids=dev(c["gt_ids"]),
             gt_tte=dev(c["gt_tte"]), det_labels=dev(c["det_labels"]), track_to_det=dev(fr["track_to_det"]),
             det_to_track=dev(fr["det_to_track"]), born=dev(fr["born"]), kill=dev(fr["kill"]))
    for k in OUTPUTS:
        t[k] = torch.full((C if k in ("true_t2d", "track_truth") else D,), 99, dtype=torch.int32, device="cuda")
    T.decide(t, gt_cap, skip_empty=skip_empty, forced=forced)
    for k in OUTPUTS:
        assert same_bits(host(t[k]), want[k]), k
    for k in BOOK:
        assert same_bits(host(t[k]), want_book[k]), k
    # the frame's update by the restatement of A5, then a retirement: record reads the ids as they are after both
    new, src, det_slot, det_id = TR.plan_frame(TR.copy_state(st), fr, frame_limit=3)
    g = np.random.default_rng(C + D + G)
    new = TR.retire((g.random(C) < 0.1).astype(np.int32), new)
    want_book = R.record(want_book, new["ids"], want["track_truth"], want["det_gt"], det_slot, det_id, c["gt_labels"], c["gt_ids"],
                         c["gt_tte"], gt_cap, c["det_labels"])
    for k in ("col4row", "row4col", "info", "cost", "thresh", "track_to_det", "det_to_track", "born", "kill", "true_t2d",
              "true_d2t", "det_truth"):
        del t[k]
    t.update(ids=dev(new["ids"]), det_slot=dev(det_slot), det_id=dev(det_id))
    T.record(t, gt_cap)
    for k in BOOK:
        assert same_bits(host(t[k]), want_book[k]), k
    return want_book, want, (new, det_slot, det_id)


# ---- 1. cost, decide, record ------------------------------------------------------------------------------------------------
# the shapes cross the 64-entry word on every side; each of D and G is zero in one of them; (1000, 24, 30) gives every
# wave of decide's join more than one detection
SHAPES = [(1, 1, 1), (70, 67, 66), (130, 3, 5), (64, 0, 4), (40, 12, 0), (1000, 24, 30)]


@pytest.mark.parametrize("masks", [True, False])
@pytest.mark.parametrize("C,D,G", SHAPES)
def test_cost_decide_record_equal_the_restatement(C, D, G, masks):
    seen = 0
    # both widths with both kinds, and skip_empty on and off with each kind
    for W, kind, thresh, skip in ((9, "centre", 2.0, True), (7, "iou", -0.3, False), (7, "centre", 2.0, False),
                                  (9, "iou", -0.3, True)):
        g = np.random.default_rng([C, D, G, W, int(masks), int(kind == "iou")])
        c = R.random_case(g, C, D, G, W, masks=masks)
        book, out, (new, det_slot, det_id) = run_frame(c, kind, thresh, skip_empty=skip)
        seen += int((out["det_gt"] >= 0).sum())
        if (C, D, G) == (70, 67, 66):
            assert (out["true_d2t"] >= 0).sum() >= 2 and (out["det_truth"] == 1).sum() >= 2 and (out["det_truth"] == 2).sum() >= 2
            assert set(out["track_truth"].tolist()) == {-1, 0, 1, 2}
            held = c["book"]["slot_gt"][(c["st"]["ids"] >= 0) & (c["book"]["slot_gt"] >= 0)]
            assert len(held) > len(set(held.tolist()))                          # an id that two slots hold
            assert book["stats"][R.SWITCHES] > c["book"]["stats"][R.SWITCHES]
    if min(D, G) >= 24:
        assert seen >= 16
    if min(D, G) == 0:
        assert seen == 0


def test_the_filler_writes_device_addresses_and_nulls():
    """abi.fill over pcr_truth on device tensors at C = 4, D = 3, G = 2: every field holds its tensor's address; an empty
    tensor (D = 0) and a None are NULL; a scalar field is not touched"""
    from pcr_amd import abi
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")     # noqa: E731
    f32 = lambda *s: torch.zeros(s, device="cuda")                       # noqa: E731
    for C, D, G in ((4, 3, 2), (4, 0, 2)):
        sizes = dict(ids=C, slot_gt=C, slot_tte=C, gt_last=8, stats=24, col4row=D, row4col=G, info=1, cost=D * G, thresh=1,
                     gt_labels=G, gt_ids=G, gt_tte=G, det_labels=D, track_to_det=C, det_to_track=D, born=D, kill=C,
                     det_gt=D, true_t2d=C, true_d2t=D, det_truth=D, track_truth=C, det_slot=D, det_id=D)
        assert set(sizes) == set(abi.TruthParams.ELEM)
        t = {k: (f32(D, G) if k == "cost" else f32(1) if k == "thresh" else i32(n)) for k, n in sizes.items()}
        t["born"] = t["kill"] = None
        p = abi.TruthParams()
        p.C, p.D, p.G = C, D, G
        assert abi.fill(p, t, sizes, required=("ids",), who="test") is p
        assert (p.C, p.D, p.G) == (C, D, G)
        for k, x in t.items():
            want = x.data_ptr() if x is not None and x.numel() else None
            assert getattr(p, k) == want, (k, D)
            assert (want is None) == (k in ("born", "kill") or sizes[k] == 0), (k, D)
    with pytest.raises(Exception, match="cost must be a torch.float32 tensor"):
        abi.fill(abi.TruthParams(), dict(cost=f32(3, 2).double()), sizes, who="test")


def test_book_matches_by_iou_through_its_own_buffers():
    """TruthBook(kind="iou"): nearest_bev + iou_bev(kind="axis") into the book's buffers, the threshold held negated"""
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    g = np.random.default_rng(23)
    C, D, G, W = 70, 67, 66, 9
    c = R.random_case(g, C, D, G, W)
    book = TU.TruthBook(T.TrackBank(C, D, feat_shape=(3, 5), box_width=W), G + 3, c["gt_cap"], kind="iou", thresh=0.3)
    assert host(book.thresh).tolist() == [np.float32(-0.3)]
    col, row, info = book.match(dev(c["det_boxes"]), dev(c["det_labels"]),
                                dict(boxes=dev(c["gt_boxes"]), labels=dev(c["gt_labels"]), ids=dev(c["gt_ids"]), tte=dev(c["gt_tte"])))
    pad = lambda a, fill: np.concatenate([a, np.full((3,) + a.shape[1:], fill, a.dtype)])
    gb, gl, gi = pad(c["gt_boxes"], 0), pad(c["gt_labels"], -1), pad(c["gt_ids"], -1)
    iou = NR.iou_axis(NR.nearest_bev(c["det_boxes"][:, :7]), NR.nearest_bev(gb[:, :7])).astype(np.float32).reshape(D, G + 3)
    want = R.cost(c["det_boxes"], c["det_labels"], gb, gl, gi, c["gt_cap"], iou=iou)
    assert same_bits(host(book.cost), want)
    wcol, wrow, winfo = R.lsa_maps(want)
    assert same_bits(host(col), wcol) and same_bits(host(row), wrow) and same_bits(host(info), winfo)
    assert (want[:, G:] == 10000.0).all() and (want < -0.3).sum() >= 8            # the padding is flat, real overlaps exist


def test_forced_decisions_count_as_their_own_truth():
    g = np.random.default_rng(21)
    c = R.random_case(g, 70, 67, 66, 9)
    c["book"]["stats"][:] = 0
    book, out, _ = run_frame(c, "centre", 2.0, skip_empty=False, forced=True)
    for k in range(5):
        gt, correct, pred = book["stats"][3 * k:3 * k + 3]
        assert gt == correct == pred and gt > 0


def test_padding_an_id_at_gt_cap_and_a_nan_box_behave_as_written():
    g = np.random.default_rng(22)
    c = R.random_case(g, 70, 67, 66, 9)
    # every detection sits exactly on a ground-truth box of its class: each valid pair would be a true positive
    n = 60
    c["det_boxes"][:n, :2] = c["gt_boxes"][:n, :2]
    c["det_labels"][:n] = np.where(c["gt_labels"][:n] >= 0, c["gt_labels"][:n], 1)
    c["det_labels"][5] = -1                                                       # a padded detection on a valid box
    assert c["gt_ids"][0] == c["gt_cap"] and c["gt_ids"][1] == -1 and (c["gt_labels"][:n] < 0).sum() >= 3
    c["fr"]["labels"] = c["det_labels"]
    book, out, _ = run_frame(c, "centre", 2.0)
    ok = R.gt_valid(c["gt_labels"], c["gt_ids"], c["gt_cap"])
    for d in range(n):
        assert (out["det_gt"][d] == d) == bool(ok[d] and d != 5), d              # padding on either side is no true positive
    assert out["det_truth"][5] == -1 and out["det_truth"][0] == 2 and out["det_truth"][1] == 2
    c["det_boxes"][7, 0] = np.nan                                                 # info == 1: no true positive at all
    book, out, _ = run_frame(c, "centre", 2.0)
    assert (out["det_gt"] == -1).all() and (out["true_t2d"] == -1).all() and (out["det_truth"][c["det_labels"] >= 0] == 2).all()
    assert book["stats"][R.TP] == c["book"]["stats"][R.TP]


# ---- 2. a sequence, eager and from one captured graph ------------------------------------------------------------------------
FEAT, NMS_THRESH, LIMIT = (3, 5), 0.1, 3


def sequence(C, D, G, W, frames, seed):
    """a scripted scene with a head's mistakes and, after each frame, what the restatements hold"""
    sc = R.Scene(n_obj=14, frames=frames, D=D, G=G, W=W, seed=seed)
    g = np.random.default_rng(seed + 50)
    st, book = TR.new_state(C, W), R.new_book(C, sc.gt_cap)
    out = []
    for f in range(frames):
        fr = sc.frame(f)
        dl, gl, gi = fr["det_labels"], fr["gt_labels"], fr["gt_ids"]
        cost = R.cost(fr["det_boxes"], dl, fr["gt_boxes"], gl, gi, sc.gt_cap)
        col, row, info = R.lsa_maps(cost)
        tr = R.truth(book, st["ids"], col, row, info, cost, sc.thresh, gl, gi, sc.gt_cap, dl)
        t2d, d2t, born, kill = R.corrupt(g, tr, st["ids"], dl)
        book, tr = R.decide(book, st["ids"], col, row, info, cost, sc.thresh, gl, gi, sc.gt_cap, dl, t2d, d2t, born, kill)
        lengths = g.integers(1, 6, D).astype(np.int32)
        st, src, det_slot, det_id = TR.plan(st, t2d, d2t, dl, lengths, fr["det_boxes"], fr["det_scores"], born=born, kill=kill,
                                            frame_limit=LIMIT)
        score = (st["steps"].astype(np.float32) + st["scores"]).astype(np.float32)
        st = TR.retire(NR.track_nms(NR.nearest_bev(st["boxes"][:, :7]), st["labels"], score, NMS_THRESH).astype(np.int32), st)
        book = R.record(book, st["ids"], tr["track_truth"], tr["det_gt"], det_slot, det_id, gl, gi, fr["gt_tte"], sc.gt_cap, dl)
        out.append(dict(fr=fr, t2d=t2d, d2t=d2t, born=born, kill=kill, lengths=lengths, truth=tr, book=book, st=st,
                        det_f=g.standard_normal((D,) + FEAT).astype(np.float32),
                        det_x=g.standard_normal((D, FEAT[1], 3)).astype(np.float32)))
    return sc, out


def test_twelve_frames_eager_and_replayed_from_one_graph():
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    C, D, G, W = 26, 12, 12, 9
    sc, seq = sequence(C, D, G, W, 12, seed=3)
    assert seq[-1]["book"]["stats"][R.SWITCHES] >= 1 and (seq[-1]["book"]["stats"][:15:3] > 0).all()
    bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)
    book = TU.TruthBook(bank, G, sc.gt_cap, kind="centre", thresh=sc.thresh)
    frame_keys = ("det_boxes", "det_labels", "det_scores", "gt_boxes", "gt_labels", "gt_ids", "gt_tte")
    own_keys = ("t2d", "d2t", "born", "kill", "lengths", "det_f", "det_x")
    S = {k: dev(seq[0]["fr"][k]) for k in frame_keys}                           # the static inputs of the capture
    S.update({k: dev(seq[0][k]) for k in own_keys})

    def load(s):
        for k in frame_keys:
            S[k].copy_(dev(s["fr"][k]))
        for k in own_keys:
            S[k].copy_(dev(s[k]))

    def step():
        book.match(S["det_boxes"], S["det_labels"], dict(boxes=S["gt_boxes"], labels=S["gt_labels"], ids=S["gt_ids"], tte=S["gt_tte"]))
        out = book.decide((S["t2d"], S["d2t"]), S["det_labels"], born=S["born"], kill=S["kill"])
        det_slot, det_id, info = bank.update(
            (S["t2d"], S["d2t"]), dict(labels=S["det_labels"], lengths=S["lengths"], boxes=S["det_boxes"], scores=S["det_scores"],
                                       feats=S["det_f"], xyz=S["det_x"]), born=S["born"], kill=S["kill"], frame_limit=LIMIT)
        bank.suppress(NMS_THRESH)
        book.record(det_slot, det_id)
        return out

    def snapshot(out):
        return [host(out[k]).copy() for k in sorted(out)] + [host(getattr(book, k)).copy() for k in BOOK] + \
               [host(getattr(bank, k)).copy() for k in TR.STATE] + [host(bank.feats).copy()]

    names = dict(det_gt="det_gt", true_track_to_det="true_t2d", true_det_to_track="true_d2t", det_truth="det_truth",
                 track_truth="track_truth")
    eager = []
    for f, s in enumerate(seq):
        load(s)
        out = step()
        for k, r in names.items():
            assert same_bits(host(out[k]), s["truth"][r]), (f, k)
        for k in BOOK:
            assert same_bits(host(getattr(book, k)), s["book"][k]), (f, k)
        for k in TR.STATE:
            assert same_bits(host(getattr(bank, k)), s["st"][k]), (f, k)
        eager.append(snapshot(out))
    m, want = book.metrics(), R.metrics(seq[-1]["book"]["stats"])
    assert m == want and m["frames"] == 12 and m["tp"] + m["fn"] == m["gt_total"]
    # the same frames from ONE captured graph (the eager run above was the warm-up)
    bank.reset()
    book.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    load(seq[0])
    with torch.cuda.graph(graph):                            # a device-to-host copy in here would fail the capture
        out = step()
    bank.reset()                                             # (a capture records, it does not run)
    book.reset()
    for f, s in enumerate(seq):
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(snapshot(out), eager[f]):
            assert same_bits(a, b), f
    # thresh is re-read from the device: the same graph with a threshold no pair meets finds no true positive
    book.thresh.fill_(-1.0)
    tp = int(host(book.stats)[R.TP])
    load(seq[-1])
    graph.replay()
    torch.cuda.synchronize()
    assert (host(out["det_gt"]) == -1).all() and int(host(book.stats)[R.TP]) == tp and len(seq[-1]["fr"]["pairs"]) > 0


# ---- 3. the whole frame on the toy model -------------------------------------------------------------------------------------
def toy_model_and_frames(n_frames, M, W, n):
    import bench
    from test_gpu_tracks import toy_frames
    model, _ = bench.build_pt_model([n, 64, 32])
    return model, toy_frames(n_frames, M, n + 20, W, seed=31)


def test_track_step_with_truth_leaves_every_output_and_the_bank_as_they_were():
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    C, D, M, W, n = 16, 8, 6, 9, 128
    model, frames = toy_model_and_frames(3, M, W, n)
    runs = []
    with torch.no_grad():
        c0 = model.forward_inference_boxes(dev(frames[0][0]), dev(np.concatenate([frames[0][1], np.zeros((D - M, W), np.float32)])[:, :7].copy()), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])
        for with_truth in (False, True):
            bank = T.TrackBank(C, D, feat_shape=(64, n), box_width=W)
            book = TU.TruthBook(bank, D, 32) if with_truth else None
            got = []
            for f, (pts, boxes, labels, scores) in enumerate(frames):
                truth = dict(book=book, boxes=dev(boxes), labels=dev(labels), ids=dev(np.arange(M, dtype=np.int32) + 3),
                             tte=dev(np.full(M, len(frames) - 1 - f, np.int32))) if with_truth else None
                out = model.track_step(bank, dev(pts), dev(boxes), dev(labels), dev(scores), crop_args=dict(seed=5 + f),
                                       frame_limit=LIMIT, suppress_threshold=NMS_THRESH, truth=truth)
                got.append(({k: host(v).copy() for k, v in out.items() if v is not None},
                            {k: host(v).copy() for k, v in bank.state().items()}, host(bank.feats).copy(), host(bank.xyz).copy()))
            runs.append(got)
            if with_truth:
                m = book.metrics()
                assert m["frames"] == 3 and m["tp"] == 3 * M and m["fp"] == m["fn"] == 0      # the detections ARE the ground truth
    for (o0, st0, f0, x0), (o1, st1, f1, x1) in zip(*runs):
        assert set(o1) - set(o0) == {"det_gt", "true_track_to_det", "true_det_to_track", "det_truth", "track_truth"}
        for k in o0:
            assert same_bits(o0[k], o1[k]), k
        for k in st0:
            assert same_bits(st0[k], st1[k]), k
        assert same_bits(f0, f1) and same_bits(x0, x1)
        assert o1["det_gt"][:M].tolist() == list(range(M)) and (o1["det_gt"][M:] == -1).all()


def test_forced_truth_keeps_every_id_on_a_scripted_scene():
    """the detections are the ground-truth boxes, shuffled; some are dropped, and as many false boxes are added (3 m beside
    a dropped object, beyond the 2 m threshold), so a frame holds as many valid detections as ground-truth boxes"""
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    C, D, M, W, n, n_frames = 16, 8, 6, 9, 128, 8
    model, frames = toy_model_and_frames(n_frames, M, W, n)
    g = np.random.default_rng(17)
    gt_ids = (np.arange(M, dtype=np.int32) * 5 + 2)
    bank = T.TrackBank(C, D, feat_shape=(64, n), box_width=W)
    book = TU.TruthBook(bank, D, 40, kind="centre", thresh=2.0)
    seen = {}                                                # ground-truth id -> the tracker ids it was given
    last_seen = {}
    with torch.no_grad():
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            dropped = {f % M, (f + 3) % M} if f % 3 == 2 else ({f % M} if f else set())      # never twice in a row
            keep = [m for m in range(M) if m not in dropped]
            false = boxes[sorted(dropped)].copy()
            false[:, 1] += 3.0
            det = np.concatenate([boxes[keep], false])
            det_l = np.concatenate([labels[keep], labels[sorted(dropped)]]).astype(np.int32)
            owner = np.array(keep + [-1] * len(dropped))
            order = g.permutation(len(det))
            det, det_l, owner = det[order], det_l[order], owner[order]
            out = model.track_step(bank, dev(pts), dev(det), dev(det_l), dev(scores[:len(det)]), crop_args=dict(seed=5 + f),
                                   frame_limit=LIMIT, suppress_threshold=NMS_THRESH, force_truth=True,
                                   truth=dict(book=book, boxes=dev(boxes), labels=dev(labels), ids=dev(gt_ids),
                                              tte=dev(np.full(M, n_frames - 1 - f, np.int32))))
            det_gt, det_id = host(out["det_gt"]), host(out["det_id"])
            assert det_gt[:len(det)].tolist() == owner.tolist(), f
            for d, m in enumerate(owner):
                if m >= 0:
                    assert det_id[d] >= 0, (f, d)
                    assert f - last_seen.get(m, f) <= LIMIT
                    seen.setdefault(int(gt_ids[m]), set()).add(int(det_id[d]))
                    last_seen[m] = f
                else:
                    assert det_id[d] == -1, (f, d)            # a false box is neither matched nor born
    m = book.metrics()
    assert m["switches"] == 0 and m["untracked"] == 0 and m["frames"] == n_frames
    assert sorted(seen) == gt_ids.tolist() and all(len(v) == 1 for v in seen.values())      # one tracker id per object
    assert m["fp"] == m["fn"] > 0 and m["tp"] + m["fn"] == m["gt_total"] == n_frames * M
    for k in R.KINDS:
        assert m[k + "_gt"] == m[k + "_correct"] == m[k + "_num_pred"], k
    assert m["det_match_gt"] > 0 and m["det_newborn_gt"] == M and m["det_false_positive_gt"] > 0 and m["track_false_negative_gt"] > 0
