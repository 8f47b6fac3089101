"""Per-box object clouds cut from a LiDAR sweep on the device (include/pcr.h section A2, csrc/crop_kernels.hip).

`crops_from_boxes` is the step in front of `ReIDNet.forward_inference`: the reference's tracker builds its `(M, n, 3)`
batch with `interpolate_per_frame` + `get_input_batch` (mmdet3d/models/trackers/deprecated/pc_utils.py:31-96: a `(P, T)`
membership tensor, a Python loop over the boxes, a padded batch, a batched affine and one host `torch.randint` per box);
here it is one launch with a fixed output shape, no host read and the same bits on every run, so it can be captured in
a HIP graph together with everything behind it.  INTEGRATION.md ("from a sweep and boxes") has the mapping.
"""
import torch

from . import _lib as L

_WHO = "pcr_amd.crops"
FRAMES = {"sensor": 0, "centred": 1, "box": 2}
RULES = {"tracker": 0, "dataset": 1}


def crop_boxes_ok(P, M, n, stride=3):
    """whether pcr_crop_boxes_f32 takes the launch shape (P sweep points of `stride` floats, M boxes, n samples)"""
    return bool(L.load().pcr_crop_boxes_ok(int(P), int(M), int(n), int(stride)))


def box_frames(boxes, out=None):
    """boxes (T, 7) -> (T, 2) float32 = (cos(rz + pi/2), sin(rz + pi/2)) as the kernels evaluate them"""
    boxes = L.tensor(boxes, _WHO, "boxes", torch.float32, shape=(None, 7))
    T = boxes.shape[0]
    out = L.out_tensor(out, _WHO, "out", torch.float32, (T, 2), boxes.device)
    L.require_cuda(boxes, out)
    L.run.pcr_box_frames_f32(boxes, out, T, L.stream_ptr())
    return out


def crops_from_boxes(points, boxes, n, frame="box", rule="tracker", rand=None, seed=None, z_is_centre=False,
                     return_frames=False, out=None):
    """points (P, C >= 3) float32 sweep (xyz first), boxes (M, 7) [x, y, z, w, l, h, rz] -> clouds (M, n, 3) float32,
    lengths (M,) int32 [, frames (M, 2)].

    frame  "sensor" | "centred" | "box": coordinates as read / minus the box's gravity centre / in the box frame
    rule   "tracker" (empty box -> zeros, otherwise n draws with replacement) | "dataset" (subsamplePC: fewer than 3
           points -> zeros, exactly n -> the points in sweep order, otherwise n draws)
    rand   (M, n) int32 device tensor of random words (read as 32 unsigned bits); without it the kernel's own
           counter-based generator is keyed by (seed, box, slot)
    seed   a device int64 tensor of one element (read at run time: bump it in place between replays of a captured
           graph) or a Python int; None = 0
    z_is_centre  boxes[:, 2] is the gravity centre instead of the bottom face
    out    (clouds, lengths[, frames]) to write into, so that a captured graph owns no allocation
    """
    if frame not in FRAMES:
        raise ValueError("frame must be one of %s, got %r" % (sorted(FRAMES), frame))
    if rule not in RULES:
        raise ValueError("rule must be one of %s, got %r" % (sorted(RULES), rule))
    seed_t = seed if isinstance(seed, torch.Tensor) else None
    points = L.tensor(points, _WHO, "points", torch.float32, shape=(None, None))
    L.require(points.shape[1] >= 3, _WHO, "points must be (P, C >= 3), got %s", tuple(points.shape))
    boxes = L.tensor(boxes, _WHO, "boxes", torch.float32, shape=(None, 7))
    P, stride = points.shape
    M, n = boxes.shape[0], int(n)
    rand = L.tensor(rand, _WHO, "rand", torch.int32, shape=(M, n), optional=True)
    if not crop_boxes_ok(P, M, n, stride):
        raise L.PcrError("crops_from_boxes: launch shape P=%d M=%d n=%d stride=%d is out of range (pcr_crop_boxes_ok)"
                         % (P, M, n, stride))
    dev = points.device
    if seed_t is not None:
        if seed_t.dtype != torch.int64 or seed_t.numel() != 1:
            raise L.PcrError("seed must be a device int64 tensor of one element or a Python int")
    elif seed is not None:
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        seed_t = torch.full((1,), s - (1 << 64) if s >= (1 << 63) else s, dtype=torch.int64, device=dev)
    L.require(out is None or len(out) >= 2, _WHO, "out must be (clouds, lengths[, frames])")
    clouds = L.out_tensor(None if out is None else out[0], _WHO, "out[0] (clouds)", torch.float32, (M, n, 3), dev)
    lengths = L.out_tensor(None if out is None else out[1], _WHO, "out[1] (lengths)", torch.int32, (M,), dev)
    L.require_cuda(points, boxes, rand, seed_t, clouds, lengths)
    L.run.pcr_crop_boxes_f32(points, stride, boxes, rand, L.ptr(seed_t), clouds, lengths, P, M, n, FRAMES[frame],
                             RULES[rule], int(bool(z_is_centre)), L.stream_ptr())
    if return_frames:
        fr = box_frames(boxes, out[2] if out is not None and len(out) > 2 else None)
        return clouds, lengths, fr
    return clouds, lengths
