"""Bird's-eye-view box overlap and duplicate suppression on the device (include/pcr.h section A4, csrc/nms_kernels.hip).

The reference's tracker leaves the device twice per frame for the same operation, overlap between BEV boxes followed by
suppression: the track NMS (`VirtualTracker.non_max_suppression`, trackers/deprecated/virtual_tracker.py:232-259, a
`torch.where` with a data-dependent shape) and the detection NMS of `ops/iou3d` (iou3d_utils.py:23-68: the whole mask is
copied to the host and swept there).  Here each step is a fixed-shape launch without a host read and with the same bits
on every run, so both can be captured in a HIP graph with the rest of the frame.  INTEGRATION.md ("2d. Duplicate
suppression") has the mapping; `mmdet3d.ops.nms_gpu` / `nms_normal_gpu` / `boxes_iou_bev` wrap these with the
reference's signatures.

Workspaces and the one-element threshold tensors made from Python floats are cached (per device and N, per device and
value; at most 64 values, further ones get a tensor per call -- a caller that varies the threshold passes a device
tensor).  A cached tensor is used by every call of that key, in stream order: calls that share a key belong on one stream.
A capture must find its entries in the cache -- run the call once eagerly first, as with any launch that is captured.
"""
import torch

from . import _lib as L

KINDS = {"axis": 0, "rotated": 1, "overlap": 2}

_WS = {}          # (device index, N) -> uint8 workspace of pcr_nms_ws_bytes(N)
_THRESH = {}      # (device index, value) -> (1,) float32


_THRESH_MAX = 64  # distinct Python-float thresholds kept per process; a caller that sweeps more passes a device tensor


_WHO = "pcr_amd.nms"


def _cached(table, key, make):
    t = table.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise L.PcrError("pcr_amd.nms: nothing is cached for %r yet; run the call once outside the capture" % (key,))
        t = table[key] = make()
    return t


def _thresh(thresh, device):
    """a Python number -> its cached (1,) device tensor; a device tensor of one float32 is taken as it is (and re-read by
    every replay of a captured launch)"""
    if isinstance(thresh, torch.Tensor):
        thresh = L.tensor(thresh, _WHO, "thresh", torch.float32, numel=1)
        L.require_cuda(thresh)
        return thresh
    v = float(thresh)
    make = lambda: torch.full((1,), v, dtype=torch.float32, device=device)
    if (device.index, v) not in _THRESH and len(_THRESH) >= _THRESH_MAX:
        # the cache is full and is never evicted (a captured graph may hold an entry's address): this value gets a tensor of
        # its own, which an eager call simply drops afterwards
        if torch.cuda.is_current_stream_capturing():
            raise L.PcrError("pcr_amd.nms: more than %d distinct float thresholds; pass a device tensor" % _THRESH_MAX)
        return make()
    return _cached(_THRESH, (device.index, v), make)


def _boxes(t, width, name):
    return L.tensor(t, _WHO, name, torch.float32, shape=(None, width), copy=True)


def nms_ok(N):
    """whether pcr_nms_f32 / pcr_track_nms_f32 take N boxes"""
    return bool(L.load().pcr_nms_ok(int(N)))


def nearest_bev(boxes7, out=None):
    """boxes7 (N, 7) [x, y, z, w, l, h, rz] -> (N, 5) [x1, y1, x2, y2, 0]: LiDARInstance3DBoxes.nearest_bev (the box
    turned to the nearer axis) with a zero angle column, so that the result goes to every op here as it is"""
    boxes7 = _boxes(boxes7, 7, "boxes7")
    N = boxes7.shape[0]
    out = L.out_tensor(out, _WHO, "out", torch.float32, (N, 5), boxes7.device)
    L.require_cuda(boxes7, out)
    L.run.pcr_nearest_bev_f32(boxes7, out, N, L.stream_ptr())
    return out


def bev_frames(boxes5, out=None):
    """boxes5 (N, 5) -> (N, 2) float32 = (cos(angle), sin(angle)) as the rotated kernels evaluate them"""
    boxes5 = _boxes(boxes5, 5, "boxes5")
    N = boxes5.shape[0]
    out = L.out_tensor(out, _WHO, "out", torch.float32, (N, 2), boxes5.device)
    L.require_cuda(boxes5, out)
    L.run.pcr_bev_frames_f32(boxes5, out, N, L.stream_ptr())
    return out


def iou_bev(a, b, kind="rotated", out=None):
    """a (A, 5), b (B, 5) [x1, y1, x2, y2, angle] -> (A, B) float32, every element written.

    kind  "rotated" (iou3d's boxes_iou_bev) | "axis" (iou_normal: the angle is ignored) | "overlap" (the area of the
          rotated intersection only, iou3d's boxes_overlap_bev)"""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
    a, b = _boxes(a, 5, "a"), _boxes(b, 5, "b")
    A, B = a.shape[0], b.shape[0]
    out = L.out_tensor(out, _WHO, "out", torch.float32, (A, B), a.device)
    L.require_cuda(a, b, out)
    L.run.pcr_iou_bev_f32(a, b, out, A, B, KINDS[kind], L.stream_ptr())
    return out


def nms(boxes5, scores, thresh, kind="rotated", pre_max=None, out=None, return_order=False):
    """Greedy NMS without a host read: boxes5 (N, 5), scores (N,) -> keep (N,), count (1,), info (1,) int32
    [, order (N,) int32].

    keep    the original indices of the kept boxes, best score first, padded with -1
    count   how many of them there are
    info    0; 1 = a NaN score or a non-finite box: keep is all -1 and count 0
    order   the ranking itself: indices by descending score, equal scores lowest index first
    kind    "rotated" (the reference's nms_gpu) | "axis" (nms_normal_gpu)
    thresh  a Python float, or a (1,) float32 device tensor that a replayed graph re-reads
    pre_max only the pre_max best scores take part (the reference's pre_maxsize); None = all
    out     (keep, count, info[, order]) to write into"""
    if kind not in ("rotated", "axis"):
        raise ValueError("kind must be 'rotated' or 'axis', got %r" % (kind,))
    boxes5 = _boxes(boxes5, 5, "boxes5")
    N = boxes5.shape[0]
    scores = L.tensor(scores, _WHO, "scores", torch.float32, shape=(N,), copy=True)
    L.require(nms_ok(N), "nms", "N=%d is out of range (pcr_nms_ok)", N)
    dev, i32 = boxes5.device, torch.int32
    if out is not None:
        L.require(len(out) >= 3, _WHO, "out must be (keep (N,), count (1,), info (1,)[, order (N,)])")
        keep = L.tensor(out[0], _WHO, "out[0] (keep)", i32, shape=(N,))
        count, info = L.tensor(out[1], _WHO, "out[1] (count)", i32, numel=1), L.tensor(out[2], _WHO, "out[2] (info)", i32, numel=1)
        order = out[3] if len(out) > 3 else None
    else:
        keep = torch.empty((N,), dtype=i32, device=dev)
        both = torch.empty((2,), dtype=i32, device=dev)                   # adjacent: one read fetches both
        count, info, order = both[0:1], both[1:2], None
    order = L.out_tensor(order, _WHO, "out[3] (order)", i32, (N,), dev)
    L.require_cuda(boxes5, scores, keep, count, info, order)
    if N == 0:                           # the entry launches nothing for no boxes: nothing is kept
        count.zero_()
        info.zero_()
    else:
        ws = _cached(_WS, (dev.index, N),
                     lambda: torch.empty((L.load().pcr_nms_ws_bytes(N),), dtype=torch.uint8, device=dev))
        L.run.pcr_nms_f32(boxes5, scores, _thresh(thresh, dev), order, keep, count, info, L.ptr(ws), N, KINDS[kind],
                          0 if pre_max is None else max(int(pre_max), 0), L.stream_ptr())
    return (keep, count, info, order) if return_order else (keep, count, info)


def track_nms(boxes5, classes, scores, thresh, out=None):
    """The tracker's pairwise rule on BEV boxes (N, 5) (the angle is ignored) -> suppressed (N,) int32, 0 or 1: for every
    i < j of one class with iou_normal > thresh, i is suppressed if scores[i] - scores[j] <= 0, otherwise j."""
    boxes5 = _boxes(boxes5, 5, "boxes5")
    N = boxes5.shape[0]
    classes = L.tensor(classes, _WHO, "classes", torch.int32, shape=(N,), cast_int64=True, copy=True)    # the tracker's is int64
    scores = L.tensor(scores, _WHO, "scores", torch.float32, shape=(N,), copy=True)
    L.require(nms_ok(N), "track_nms", "N=%d is out of range (pcr_nms_ok)", N)
    out = L.out_tensor(out, _WHO, "out", torch.int32, (N,), boxes5.device)
    L.require_cuda(boxes5, classes, scores, out)
    L.run.pcr_track_nms_f32(boxes5, classes, scores, _thresh(thresh, boxes5.device), out, N,
                            L.stream_ptr())
    return out


def suppress_tracks(boxes7, classes, scores, thresh, out=None):
    """VirtualTracker.non_max_suppression's decision for the active tracks, as a fixed-shape mask: boxes7 (N, 7) the
    tracks' last boxes, classes (N,), scores (N,) the track scores (the reference's `len(det_bboxes) + scores[-1]`, which
    stays with the caller), thresh its suppress_threshold -> suppressed (N,) int32.  Pruning `activeTracks` by the mask
    stays with the caller too."""
    return track_nms(nearest_bev(boxes7), classes, scores, thresh, out=out)
