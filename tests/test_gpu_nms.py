"""GPU: nearest_bev / iou_bev / nms / suppress_tracks and the mmdet3d.ops wrappers against the numpy restatements
(tests/nms_ref.py).  The axis-aligned values, the ranking, the kept lists and the track mask are compared exactly; the
rotated overlap within 4 x d32, d32 being the float32-against-float64 difference of the restatements on the same pairs
(tests/test_nms_cpu.py measures and records it: 4.38e-06), with the kernels' own (cos, sin) table as the float32
restatement's input."""
import numpy as np
import pytest
import torch

import nms_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. nearest_bev and the pairwise overlaps ---------------------------------------------------------------------------
def test_nearest_bev_bit_for_bit():
    from pcr_amd import nms as M
    boxes7 = R.track_case(200)[0]
    boxes7[:8, 6] = [0.0, np.pi / 4, -np.pi / 4, np.pi / 2, 3 * np.pi / 4, -3.0, 7.0, np.float32(np.pi / 4) + 1e-6]
    out = torch.full((200, 5), float("nan"), device="cuda")
    assert M.nearest_bev(dev(boxes7), out=out) is out
    assert same_bits(host(out), R.nearest_bev(boxes7))
    assert tuple(M.nearest_bev(dev(boxes7[:0])).shape) == (0, 5)


_ref = {}


def reference(shape):
    """the case, the restatements' answers (float32 ones with the DEVICE's frames) and d32, once per module run"""
    if shape not in _ref:
        from pcr_amd import nms as M
        a, b, where = R.iou_case(*shape)
        fa, fb = host(M.bev_frames(dev(a))), host(M.bev_frames(dev(b)))
        want = {k: R.iou_matrix(a, b, k, np.float32, fa, fb) for k in R.KINDS}
        d32 = max(float(np.abs(R.iou_matrix(a, b, k, np.float32).astype(np.float64) - R.iou_matrix(a, b, k, np.float64)).max())
                  for k in ("rotated",))
        _ref[shape] = (a, b, where, fa, fb, want, d32)
    return _ref[shape]


def d32_of_the_set():
    return max(reference(s)[6] for s in R.IOU_SHAPES)


@pytest.mark.parametrize("shape", R.IOU_SHAPES, ids=lambda s: "%dx%d" % s)
def test_iou_bev(shape):
    from pcr_amd import nms as M
    a, b, where, fa, fb, want, _ = reference(shape)
    # the frames are cosf / sinf of the angle: each side is good to 2 ulp of a value below 1, so they meet within 4
    assert np.abs(fa - R.frames_of(a, np.float32)).max() <= 4 * 2.0 ** -24
    assert np.abs(fb - R.frames_of(b, np.float32)).max() <= 4 * 2.0 ** -24
    got = {}
    for kind in R.KINDS:
        out = torch.full(shape, float("nan"), device="cuda")                # poisoned: every element must be written
        assert M.iou_bev(dev(a), dev(b), kind=kind, out=out) is out
        got[kind] = host(out)
        again = M.iou_bev(dev(a), dev(b), kind=kind)
        assert same_bits(host(again), got[kind]), "%s: two runs differ" % kind
    assert same_bits(got["axis"], want["axis"])
    d32 = d32_of_the_set()
    assert 0 < d32 < 1e-4, d32
    err_iou = float(np.abs(got["rotated"].astype(np.float64) - want["rotated"]).max())
    err_ov = float(np.abs(got["overlap"].astype(np.float64) - want["overlap"]).max())
    print("shape %s: d32 = %.3g, |iou - restatement| = %.3g, |overlap - restatement| = %.3g" % (shape, d32, err_iou, err_ov))
    assert err_iou <= 4 * d32 and err_ov <= 4 * d32
    for name, (i, j) in where.items():
        if name in ("identical", "identical_axis"):
            assert abs(got["rotated"][i, j] - 1.0) < 1e-5
        if name in ("disjoint", "touching_edge", "zero_area_point"):
            assert got["rotated"][i, j] == 0.0 and got["overlap"][i, j] == 0.0
        if name == "zero_area_line":                                        # collinear points: rounding of the fan sum only
            assert got["overlap"][i, j] < 1e-6
        if name == "square_turned_45":
            assert abs(got["overlap"][i, j] - 8 * (np.sqrt(2) - 1)) < 1e-5


def test_boxes_iou_bev_wrapper_and_empty_sides():
    from mmdet3d import ops
    from pcr_amd import nms as M
    a, b = reference((15, 17))[:2]
    got = ops.boxes_iou_bev(dev(a), dev(b))
    assert got.dtype == torch.float32 and tuple(got.shape) == (15, 17) and got.is_cuda
    assert torch.equal(got, M.iou_bev(dev(a), dev(b), kind="rotated"))
    assert tuple(ops.boxes_iou_bev(dev(a[:0]), dev(b)).shape) == (0, 17) and tuple(M.iou_bev(dev(a), dev(b[:0])).shape) == (15, 0)


# ---- 2. greedy NMS ------------------------------------------------------------------------------------------------------
def run_nms(boxes, scores, thresh, kind, pre_max=None):
    from pcr_amd import nms as M
    N = len(boxes)
    out = tuple(torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (N, 1, 1, N))
    got = M.nms(dev(boxes), dev(scores), thresh, kind=kind, pre_max=pre_max, out=out, return_order=True)
    assert all(g is o for g, o in zip(got, out))
    keep, count, info, order = (host(t) for t in got)
    return order, keep, int(count[0]), int(info[0])


def check_nms(boxes, scores, thresh, kind, iou, pre_max=None, want_keep=None):
    order, keep, count, info = run_nms(boxes, scores, thresh, kind, pre_max)
    w_order, w_keep, w_count, w_info = R.nms(boxes, scores, thresh, kind, pre_max, iou=iou)
    assert np.array_equal(order, w_order), "order"
    assert (count, info) == (w_count, w_info), "count / info"
    assert np.array_equal(keep, w_keep), "keep"
    if want_keep is not None:
        assert keep[:count].tolist() == want_keep
    return keep, count


@pytest.mark.parametrize("kind", ["axis", "rotated"])
@pytest.mark.parametrize("N", R.NMS_SIZES)
def test_nms(N, kind):
    boxes, scores, thresh, iou = R.nms_case(N, kind)
    if N == 0:
        from pcr_amd import nms as M
        keep, count, info, order = M.nms(dev(boxes), dev(scores), thresh, kind=kind, return_order=True)
        assert tuple(keep.shape) == (0,) and tuple(order.shape) == (0,) and int(count) == 0 and int(info) == 0
        return
    keep, count = check_nms(boxes, scores, thresh, kind, iou)
    assert 0 < count and (count < N or N < 63)
    if N == 130:
        check_nms(boxes, scores, thresh, kind, iou, pre_max=100)
        check_nms(boxes, scores, thresh, kind, iou, pre_max=500)              # more than there are: all take part


@pytest.mark.parametrize("kind", ["axis", "rotated"])
def test_nms_named_cases(kind):
    cases = R.named_nms_cases(kind)
    for name, (boxes, scores, thresh, iou, want) in cases.items():
        keep, count = check_nms(boxes, scores, thresh, kind, iou, want_keep=want)
    boxes, scores, thresh, iou, _ = cases["chain"]                              # greedy keeps A and C; the pairwise rule does not
    from pcr_amd import nms as M
    sup = M.track_nms(dev(boxes), dev(np.zeros(3, np.int32)), dev(scores), thresh)
    assert host(sup).tolist() == [0, 1, 1]


@pytest.mark.parametrize("kind", ["axis", "rotated"])
def test_nms_reports_nan_scores_and_non_finite_boxes(kind):
    boxes, scores, thresh, iou = R.nms_case(65, kind)
    s = scores.copy()
    s[7] = np.nan
    order, keep, count, info = run_nms(boxes, s, thresh, kind)
    assert info == 1 and count == 0 and (keep == -1).all() and np.array_equal(order, R.rank_order(s)) and order[-1] == 7
    b = boxes.copy()
    last = R.rank_order(scores)[64]
    b[last, 2] = np.inf
    assert run_nms(b, scores, thresh, kind)[3] == 1
    check_nms(b, scores, thresh, kind, iou, pre_max=64)                         # the box does not take part: not looked at
    b = boxes.copy()
    b[3, 4] = np.nan                                                            # the angle counts for the rotated kind only
    assert run_nms(b, scores, thresh, kind)[3] == (1 if kind == "rotated" else 0)


def test_nms_threshold_as_a_device_tensor():
    from pcr_amd import nms as M
    boxes, scores, thresh, _ = R.nms_case(130, "axis")
    t = torch.tensor([thresh], dtype=torch.float32, device="cuda")
    a = M.nms(dev(boxes), dev(scores), t, kind="axis")
    b = M.nms(dev(boxes), dev(scores), thresh, kind="axis")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 3. the tracker's rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 64, 65, 200])
def test_suppress_tracks(N):
    from pcr_amd import nms as M
    boxes7, classes, scores = R.track_case(N)
    want = R.track_nms(R.nearest_bev(boxes7), classes, scores, 0.1)
    out = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    got = M.suppress_tracks(dev(boxes7), dev(classes), dev(scores), 0.1, out=out)
    assert got is out and np.array_equal(host(out), want)
    got64 = M.suppress_tracks(dev(boxes7), dev(classes.astype(np.int64)), dev(scores), 0.1)          # the tracker's int64
    assert torch.equal(got64, out)
    assert N < 64 or 0 < want.sum() < N


# ---- 4. the reference's signatures ------------------------------------------------------------------------------------------
def test_mmdet3d_ops_signatures():
    from mmdet3d import ops
    from pcr_amd._lib import PcrError
    for kind, fn in (("rotated", ops.nms_gpu), ("axis", ops.nms_normal_gpu)):
        boxes, scores, thresh, iou = R.nms_case(130, kind)
        _, w_keep, w_count, _ = R.nms(boxes, scores, thresh, kind, iou=iou)
        keep = fn(dev(boxes), dev(scores), thresh)
        assert keep.dtype == torch.int64 and keep.is_cuda and keep.dim() == 1 and keep.is_contiguous()
        assert host(keep).tolist() == w_keep[:w_count].tolist()
    boxes, scores, thresh, iou = R.nms_case(130, "rotated")
    _, w_keep, w_count, _ = R.nms(boxes, scores, thresh, "rotated", 100, iou=iou)
    assert w_count > 5
    keep = ops.nms_gpu(dev(boxes), dev(scores), thresh, pre_maxsize=100, post_max_size=5)
    assert keep.dtype == torch.int64 and host(keep).tolist() == w_keep[:5].tolist()
    keep = ops.nms_gpu(dev(boxes), dev(scores), thresh, pre_maxsize=100, post_max_size=1000)
    assert host(keep).tolist() == w_keep[:w_count].tolist()
    none = ops.nms_gpu(dev(boxes), dev(scores), thresh, pre_maxsize=0)             # the reference's order[:0]
    assert none.dtype == torch.int64 and tuple(none.shape) == (0,) and none.is_cuda
    bad = scores.copy()
    bad[3] = np.nan
    with pytest.raises(PcrError):
        ops.nms_gpu(dev(boxes), dev(bad), thresh)
    empty = ops.nms_gpu(dev(boxes[:0]), dev(scores[:0]), thresh)
    assert empty.dtype == torch.int64 and tuple(empty.shape) == (0,)
    xywhr = np.array([[1.0, 2.0, 2.0, 4.0, 0.5]], np.float32)
    assert host(ops.xywhr2xyxyr(dev(xywhr))).tolist() == [[0.0, 0.0, 2.0, 4.0, 0.5]]


# ---- 5. capture -----------------------------------------------------------------------------------------------------------
def test_the_frame_steps_in_one_captured_graph():
    from pcr_amd import nms as M
    NT, ND = 65, 130
    frames = []
    for seed in (0, 1):
        boxes7, classes, tscores = R.track_case(NT, seed)
        dboxes, dscores, thresh, iou = R.nms_case(ND, "rotated", seed)
        frames.append((boxes7, classes, tscores, dboxes, dscores, np.array([thresh], np.float32), iou))
    a, b = frames
    boxes7, classes, tscores, dboxes, dscores, thr = [dev(x) for x in a[:6]]
    t_thr = torch.tensor([0.1], dtype=torch.float32, device="cuda")
    outs = lambda: (torch.empty((NT, 5), device="cuda"), torch.empty((NT,), dtype=torch.int32, device="cuda"),
                    tuple(torch.empty((n,), dtype=torch.int32, device="cuda") for n in (ND, 1, 1, ND)))

    def steps(o):
        M.nearest_bev(boxes7, out=o[0])
        M.suppress_tracks(boxes7, classes, tscores, t_thr, out=o[1])     # allocates its BEV boxes inside the capture
        M.nms(dboxes, dscores, thr, kind="rotated", out=o[2], return_order=True)

    o = outs()
    steps(o)                                                        # warm: the workspace is cached outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # a device-to-host copy in here would fail the capture
        steps(o)
    for x, y in zip((boxes7, classes, tscores, dboxes, dscores, thr), b[:6]):
        x.copy_(dev(y))
    t_thr.fill_(0.3)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (o[0], o[1], *o[2])]
    e = outs()
    steps(e)
    torch.cuda.synchronize()
    for g_, e_ in zip(got, (e[0], e[1], *e[2])):
        assert torch.equal(g_.view(torch.int32), e_.view(torch.int32))
    assert np.array_equal(host(got[1]), R.track_nms(R.nearest_bev(b[0]), b[1], b[2], 0.3))
    w_order, w_keep, w_count, w_info = R.nms(b[3], b[4], float(b[5][0]), "rotated", iou=b[6])
    assert np.array_equal(host(got[5]), w_order) and np.array_equal(host(got[2]), w_keep) and int(got[3]) == w_count
    first = R.nms(a[3], a[4], float(a[5][0]), "rotated", iou=a[6])
    assert not np.array_equal(first[1], w_keep)                     # the two frames differ where it matters
    assert not np.array_equal(R.track_nms(R.nearest_bev(a[0]), a[1], a[2], 0.1), host(got[1]))
