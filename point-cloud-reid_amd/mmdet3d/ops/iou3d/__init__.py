from .iou3d_utils import boxes_iou_bev, nms_gpu, nms_normal_gpu, xywhr2xyxyr

__all__ = ["boxes_iou_bev", "nms_gpu", "nms_normal_gpu", "xywhr2xyxyr"]
