"""`mmdet3d.ops` names used by the point-cloud ReID hot path (reference: mmdet3d/ops/__init__.py).
The reference's detection-only ops (spconv, voxelization, bev_pool, paconv, sync-BN) and its re-exports of
mmcv.ops are intentionally absent.  Of its roiaware_pool3d directory the two point-in-box ops the
tracker's crop step stands on (points_in_boxes_gpu, points_in_boxes_batch) are here; points_in_boxes_cpu and
RoIAwarePool3d are not.  Of iou3d the three ops the tracker's frame meets are here (boxes_iou_bev, nms_gpu,
nms_normal_gpu, with the xywhr2xyxyr helper their callers use): the overlap, the mask and the greedy sweep run on the
device (pcr_amd.nms)."""
from .point_ops import (FurthestPointSampling, FurthestPointSamplingWithDist, BallQuery, KNN, GatherPoints,
                        GroupingOperation, ThreeNN, ThreeInterpolate, furthest_point_sample,
                        furthest_point_sample_with_dist, ball_query, ball_query_cnt, knn, gather_points, grouping_operation,
                        three_nn, three_interpolate)

from .roiaware_pool3d import points_in_boxes_batch, points_in_boxes_gpu

from .iou3d import boxes_iou_bev, nms_gpu, nms_normal_gpu, xywhr2xyxyr

from .pointnet_modules import (SA_MODULES, GroupAll, PointFPModule, PointSAModule, PointSAModuleMSG, Points_Sampler,
                               QueryAndGroup, build_sa_module, calc_square_dist)

__all__ = ["SA_MODULES", "GroupAll", "PointFPModule", "PointSAModule", "PointSAModuleMSG", "Points_Sampler",
           "QueryAndGroup", "build_sa_module", "furthest_point_sample", "furthest_point_sample_with_dist", "ball_query", "knn", "gather_points",
           "grouping_operation", "three_nn", "three_interpolate", "points_in_boxes_gpu", "points_in_boxes_batch",
           "boxes_iou_bev", "nms_gpu", "nms_normal_gpu", "xywhr2xyxyr"]
