"""`boxes_iou_bev`, `nms_gpu` and `nms_normal_gpu` of the reference's `mmdet3d/ops/iou3d` (iou3d_utils.py:6-68) over the
C ABI in include/pcr.h (section A4): the reference's signatures and return types.  Device tensors only: a host tensor
raises PcrError, as every op here.

The two NMS functions return int64 indices of a data-dependent length, as the reference does; that signature forces ONE
host read (the number of kept boxes), which is all that leaves the device -- the mask and the sweep stay there.  A
caller that wants no host read at all (a captured frame) uses `pcr_amd.nms.nms`, which returns the fixed-shape
(keep, count, info) these are cut from.

Where they differ from the reference: at most 4096 boxes (PCR_NMS_MAX; the check is on N, also when pre_maxsize is
smaller -- the reference has no limit), a NaN score or a non-finite box raises PcrError instead of returning indices,
and equal scores are ranked lowest index first."""
import torch

from pcr_amd import _lib as L
from pcr_amd import nms as _nms


def boxes_iou_bev(boxes_a, boxes_b):
    """boxes_a (M, 5), boxes_b (N, 5) [x1, y1, x2, y2, ry] -> the rotated BEV IoU of every pair, (M, N) float32"""
    L.require_cuda(boxes_a, boxes_b)
    with torch.cuda.device(boxes_a.device):
        return _nms.iou_bev(boxes_a, boxes_b, kind="rotated")


def _kept(boxes, scores, thresh, kind, pre_max):
    L.require_cuda(boxes, scores)
    with torch.cuda.device(boxes.device):
        if pre_max is not None and pre_max <= 0:                          # the reference's order[:0]: no box takes part
            return torch.empty((0,), dtype=torch.int64, device=boxes.device)
        keep, count, info = _nms.nms(boxes, scores, thresh, kind=kind, pre_max=pre_max)
        n, bad = torch.cat([count, info]).tolist()                    # the one host read
        if bad:
            raise L.PcrError("%s: a score is NaN or a box is not finite" % ("nms_gpu" if kind == "rotated" else "nms_normal_gpu"))
        return keep[:n].to(torch.int64)


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """Rotated NMS.  boxes (N, 5) [x1, y1, x2, y2, ry], scores (N,), thresh a float -> the kept indices, best score first,
    int64 on the boxes' device.  pre_maxsize: only that many of the best scores take part; post_max_size: at most that
    many indices are returned.  Equal scores are ranked lowest index first (the reference's sort leaves them
    unspecified).  N <= 4096; a NaN score or a non-finite box raises PcrError.  Reads the number of kept boxes from the
    device once (see the module's text; `pcr_amd.nms.nms` does not)."""
    keep = _kept(boxes, scores, thresh, "rotated", pre_maxsize)
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


def nms_normal_gpu(boxes, scores, thresh):
    """Axis-aligned NMS (the angle column is ignored).  boxes (N, 5), scores (N,), thresh a float -> the kept indices,
    best score first, int64.  N <= 4096; a NaN score or a non-finite box raises PcrError.  Reads the number of kept
    boxes from the device once, as nms_gpu."""
    return _kept(boxes, scores, thresh, "axis", None)


def xywhr2xyxyr(boxes_xywhr):
    """(N, 5) [x, y, w, h, r] -> (N, 5) [x - w/2, y - h/2, x + w/2, y + h/2, r]: the box format the ops above take
    (the reference keeps this helper in core/bbox/structures/utils.py:71-89; box3d_nms's callers need it)"""
    xy, half, r = boxes_xywhr[:, 0:2], boxes_xywhr[:, 2:4] / 2, boxes_xywhr[:, 4:5]
    return torch.cat([xy - half, xy + half, r], dim=1)
