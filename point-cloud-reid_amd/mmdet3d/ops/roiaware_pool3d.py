"""The two point-in-box ops of the reference's `mmdet3d/ops/roiaware_pool3d` (points_in_boxes.py:6-49, 83-122) over
the C ABI in include/pcr.h: same signatures, assertions and return shapes.  `points_in_boxes_cpu` and `RoIAwarePool3d`
are not part of this tree.  Device tensors only: a host tensor raises PcrError, as every op here."""
import torch

from pcr_amd import _lib as L


def _check(points, boxes):
    assert boxes.shape[0] == points.shape[0], (
        f"Points and boxes should have the same batch size, got {boxes.shape[0]} and {points.shape[0]}")
    assert boxes.shape[2] == 7, f"boxes dimension should be 7, got unexpected shape {boxes.shape[2]}"
    assert points.shape[2] == 3, f"points dimension should be 3, got unexpected shape {points.shape[2]}"
    if not (points.is_cuda and boxes.is_cuda):
        L.require_cuda(points, boxes)
    assert points.device == boxes.device, "Points and boxes should be put on the same device"


def points_in_boxes_gpu(points, boxes):
    """points (B, M, 3) [x, y, z] and boxes (B, T, 7) [x, y, z, w, l, h, ry] in LiDAR coordinates, (x, y, z) the bottom
    centre -> box_idxs_of_pts (B, M) int32: the first box that holds the point, background = -1"""
    _check(points, boxes)
    batch_size, num_points, _ = points.shape
    with torch.cuda.device(points.device):
        points, boxes = points.contiguous(), boxes.contiguous()
        L.require_cuda(points, boxes)
        L.require_f32(points, boxes)
        box_idxs_of_pts = torch.empty((batch_size, num_points), dtype=torch.int, device=points.device)
        L.run.pcr_points_in_boxes_f32(points, boxes, box_idxs_of_pts, batch_size, num_points, boxes.shape[1],
                                      L.stream_ptr())
    return box_idxs_of_pts


def points_in_boxes_batch(points, boxes):
    """points (B, M, 3), boxes (B, T, 7) as above -> box_idxs_of_pts (B, M, T) int32, 1 where box t holds point m"""
    _check(points, boxes)
    batch_size, num_points, _ = points.shape
    num_boxes = boxes.shape[1]
    with torch.cuda.device(points.device):
        points, boxes = points.contiguous(), boxes.contiguous()
        L.require_cuda(points, boxes)
        L.require_f32(points, boxes)
        box_idxs_of_pts = torch.empty((batch_size, num_points, num_boxes), dtype=torch.int, device=points.device)
        L.run.pcr_points_in_boxes_batch_f32(points, boxes, box_idxs_of_pts, batch_size, num_points, num_boxes,
                                            L.stream_ptr())
    return box_idxs_of_pts
