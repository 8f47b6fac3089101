"""CPU: the crop / points-in-boxes entry points exist and refuse what they must (no launch without a GPU), and the numpy
restatement the GPU tests compare against (tests/crops_ref.py) obeys the rules include/pcr.h states."""
import ctypes
import re

import numpy as np
import pytest

import crops_ref as R

NEW_SYMBOLS = ("pcr_points_in_boxes_batch_f32", "pcr_points_in_boxes_f32", "pcr_crop_boxes_f32", "pcr_crop_boxes_ok",
               "pcr_box_frames_f32")


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header_int(name):
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_abi_is_17(lib):
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
    assert lib.pcr_abi_version() == 17


def test_crop_boxes_ok_range(lib):
    ok = lib.pcr_crop_boxes_ok
    for stride in range(3, 9):
        assert ok(1 << 20, 4096, 4096, stride) == 1
    assert ok(0, 0, 1, 3) == 1 and ok(0, 100, 128, 3) == 1 and ok(52022, 0, 128, 5) == 1 and ok(1, 1, 1, 3) == 1
    maxp, maxm = header_int("PCR_CROP_MAX_POINTS"), header_int("PCR_CROP_MAX_BOXES")
    maxn, maxs = header_int("PCR_CROP_MAX_SAMPLES"), header_int("PCR_CROP_MAX_STRIDE")
    # the header derives the bound on P from the LDS count table: one word per 64 points + 64 scratch words in 160 KiB
    assert maxp == 64 * (160 * 1024 // 4 - 64)
    assert maxp >= 1 << 20 and maxm >= 4096 and maxn >= 4096 and maxs >= 8
    assert ok(maxp, maxm, maxn, maxs) == 1
    assert ok(maxp + 1, 1, 128, 3) == 0 and ok(-1, 1, 128, 3) == 0
    assert ok(1000, maxm + 1, 128, 3) == 0 and ok(1000, -1, 128, 3) == 0
    assert ok(1000, 1, maxn + 1, 3) == 0 and ok(1000, 1, 0, 3) == 0
    assert ok(1000, 1, 128, 2) == 0 and ok(1000, 1, 128, maxs + 1) == 0


def test_null_and_out_of_range_arguments_return_invalid(lib):
    INVALID = 1
    assert lib.pcr_box_frames_f32(None, None, 4, None) == INVALID
    assert lib.pcr_box_frames_f32(None, None, -1, None) == INVALID
    assert lib.pcr_points_in_boxes_batch_f32(None, None, None, 1, 8, 2, None) == INVALID
    assert lib.pcr_points_in_boxes_batch_f32(None, None, None, -1, 8, 2, None) == INVALID
    assert lib.pcr_points_in_boxes_f32(None, None, None, 1, 8, 2, None) == INVALID
    crop = lib.pcr_crop_boxes_f32
    assert crop(None, 3, None, None, None, None, None, 8, 2, 4, 2, 0, 0, None) == INVALID
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int * 64)()
    p, i = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    # (host pointers: each call below must be refused before anything is launched)
    assert crop(p, 2, p, None, None, p, i, 8, 2, 4, 2, 0, 0, None) == INVALID            # stride
    assert crop(p, 3, p, None, None, p, i, 8, 2, 0, 2, 0, 0, None) == INVALID            # n
    assert crop(p, 3, p, None, None, p, i, 8, 2, 4, 3, 0, 0, None) == INVALID            # frame
    assert crop(p, 3, p, None, None, p, i, 8, 2, 4, 2, 2, 0, None) == INVALID            # rule
    assert crop(p, 3, p, None, None, p, i, header_int("PCR_CROP_MAX_POINTS") + 1, 2, 4, 2, 0, 0, None) == INVALID
    assert crop(p, 3, p, None, None, None, i, 8, 2, 4, 2, 0, 0, None) == INVALID         # clouds
    assert crop(p, 3, p, None, None, p, None, 8, 2, 4, 2, 0, 0, None) == INVALID         # lengths
    # nothing to do is not an error and launches nothing
    assert crop(None, 3, None, None, None, None, None, 0, 0, 4, 2, 0, 0, None) == 0
    assert lib.pcr_box_frames_f32(None, None, 0, None) == 0
    assert lib.pcr_points_in_boxes_batch_f32(None, None, None, 0, 8, 2, None) == 0
    assert lib.pcr_points_in_boxes_f32(None, None, None, 1, 0, 2, None) == 0


def test_host_tensors_raise_from_all_three_entry_points():
    import torch
    from mmdet3d import ops
    from pcr_amd import crops
    from pcr_amd._lib import PcrError
    pts, boxes = torch.zeros(1, 8, 3), torch.zeros(1, 2, 7)
    with pytest.raises(PcrError):
        ops.points_in_boxes_gpu(pts, boxes)
    with pytest.raises(PcrError):
        ops.points_in_boxes_batch(pts, boxes)
    with pytest.raises(PcrError):
        crops.crops_from_boxes(pts[0], boxes[0], 4)
    import bench
    model, _ = bench.build_pt_model([128, 64, 32], device="cpu")
    with pytest.raises(PcrError):
        model.forward_inference_boxes(pts[0], boxes[0])
    assert "points_in_boxes_gpu" in ops.__all__ and "points_in_boxes_batch" in ops.__all__


# ---- 2. the restatement ---------------------------------------------------------------------------------------------
UNIT = np.array([[1.0, 0.0]], np.float32)          # frames handed in: local_x = sx, local_y = sy


def _inside(pt, box, frames=UNIT, z_is_centre=False):
    c, ln = R.crop_boxes(np.array([pt], np.float32), np.array([box], np.float32), 1, frames=frames, z_is_centre=z_is_centre)
    return int(ln[0])


def test_boundary_rules_on_dyadic_coordinates():
    box = [8.0, -4.0, 1.0, 2.0, 4.0, 1.5, 0.25]       # w = 2 (y), l = 4 (x), bottom z = 1, top z = 2.5, cz = 1.75
    assert _inside([8.0, -4.0, 1.75], box) == 1
    assert _inside([8.0, -4.0, 1.0], box) == 1 and _inside([8.0, -4.0, 2.5], box) == 1        # both z faces are inside
    assert _inside([8.0, -4.0, 0.9999999], box) == 0 and _inside([8.0, -4.0, 2.5000002], box) == 0
    assert _inside([10.0, -4.0, 1.75], box) == 0 and _inside([6.0, -4.0, 1.75], box) == 0     # local_x == +-l/2: outside
    assert _inside([9.999999, -4.0, 1.75], box) == 1 and _inside([6.000001, -4.0, 1.75], box) == 1
    assert _inside([8.0, -3.0, 1.75], box) == 0 and _inside([8.0, -5.0, 1.75], box) == 0      # local_y == +-w/2: outside
    assert _inside([8.0, -3.0000002, 1.75], box) == 1 and _inside([8.0, -4.9999995, 1.75], box) == 1
    # gravity-centre boxes: the same box with z = cz
    cbox = list(box)
    cbox[2] = 1.75
    assert _inside([8.0, -4.0, 1.0], cbox, z_is_centre=True) == 1 and _inside([8.0, -4.0, 2.5], cbox, z_is_centre=True) == 1
    assert _inside([8.0, -4.0, 2.5000002], cbox, z_is_centre=True) == 0
    # the batch / first-box forms agree with it (numpy's own frames: rz = -pi/2 gives rot = 0)
    boxes = np.array([[box, box]], np.float32)
    boxes[0, :, 6] = -np.pi / 2
    pts = np.array([[[8.0, -4.0, 1.0], [30.0, 0.0, 1.75]]], np.float32)
    assert R.points_in_boxes_batch(pts, boxes).tolist() == [[[1, 1], [0, 0]]]
    assert R.points_in_boxes_gpu(pts, boxes).tolist() == [[0, -1]]


def test_sampler_index():
    for ln in (1, 2, 3, 1 << 20):
        j = R.sample_index(np.array([0, 1, 1 << 31, (1 << 32) - 1], np.uint32), ln)
        assert j.tolist() == [0, 0, ln >> 1, ln - 1]
        assert j.max() < ln
    # the generator: 32-bit words, fixed by (seed, box, slot); a known answer pins the hash pcr.h writes down
    w = R.crop_words(0, 0, 4)
    assert w.dtype == np.uint32 and len(set(R.crop_words(5, 3, 4096).tolist())) == 4096

    def mix(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    seed, m, s = 0x123456789ABCDEF0, 7, 11
    want = mix(mix(mix(mix((seed & 0xFFFFFFFF) ^ 0x9E3779B9) ^ (seed >> 32)) ^ m) ^ s)
    assert int(R.crop_words(seed, m, 12)[s]) == want
    assert int(R.crop_words(seed - (1 << 64), m, 12)[s]) == want        # an int64 seed is read as its 64 bits
    assert not np.array_equal(R.crop_words(1, 0, 64), R.crop_words(2, 0, 64))
    assert not np.array_equal(R.crop_words(1, 0, 64), R.crop_words(1, 1, 64))


def test_rules():
    g = np.random.default_rng(0)
    box = np.array([0.0, 0.0, -1.0, 2.0, 4.0, 2.0, 0.0], np.float32)
    n = 8
    for ln in (0, 1, 2, 3, n - 1, n, n + 1):
        pts = np.concatenate([R.points_inside(box, ln, g), np.array([[100.0, 0.0, 0.0]], np.float32)])
        rand = g.integers(0, 1 << 32, (1, n), dtype=np.uint64).astype(np.uint32).view(np.int32)
        ct, lt = R.crop_boxes(pts, box[None], n, frame="sensor", rule="tracker", rand=rand)
        cd, ld = R.crop_boxes(pts, box[None], n, frame="sensor", rule="dataset", rand=rand)
        assert lt[0] == ln and ld[0] == ln
        drawn = pts[R.sample_index(rand.view(np.uint32)[0], ln).astype(np.int64)] if ln else np.zeros((n, 3), np.float32)
        assert np.array_equal(ct[0], drawn)                              # tracker: zeros only for an empty box
        if ln <= 2:
            assert not cd.any()                                          # dataset: fewer than three points -> zeros
        elif ln == n:
            assert np.array_equal(cd[0], pts[:n])                        # exactly n -> the points in sweep order
        else:
            assert np.array_equal(cd[0], drawn)
    # the in-kernel generator and a caller's words are the same path
    pts = R.points_inside(box, 5, g)
    words = R.crop_words(9, 0, n).view(np.int32)[None]
    assert np.array_equal(R.crop_boxes(pts, box[None], n, seed=9)[0], R.crop_boxes(pts, box[None], n, rand=words)[0])


def test_frame_statement_of_integration_md():
    """INTEGRATION.md, "from a sweep and boxes": for the tracker's Depth-mode boxes D = [X, Y, Zc, xs, ys, zs, yaw]
    (DepthInstance3DBoxes(origin=(0.5, 0.5, 0.5))) and Depth-mode points p, calling the crop with
        points = (p_y, -p_x, p_z),  boxes = [Y, -X, Zc, ys, xs, zs, yaw],  z_is_centre=True,  frame="box"
    selects what interpolate_per_frame selects and returns its `centered` coordinates with no permutation or sign:
    restated here with numpy from depth_box3d.py:256-282 (the swap), box_3d_mode.py:125-128 (the box conversion) and
    pc_utils.py:8-27, 61-75 (the inverse of [Rz(-yaw) | centre], z-axis case of axis_angle_to_matrix)."""
    g = np.random.default_rng(3)
    M = 6
    D = np.stack([g.uniform(-20, 20, M), g.uniform(-20, 20, M), g.uniform(-1, 1, M), g.uniform(3.5, 5.5, M),
                  g.uniform(1.5, 2.5, M), g.uniform(1.4, 2.0, M), g.uniform(-np.pi, np.pi, M)], axis=1)
    p = np.concatenate([D[m, :3] + g.uniform(-3.5, 3.5, (200, 3)) for m in range(M)])

    def reference(m):
        """float64: (inside, centered, distance to the nearest face) of Depth box m for all Depth points p"""
        X, Y, Zc, xs, ys, zs, yaw = D[m]
        pl = np.stack([p[:, 1], -p[:, 0], p[:, 2]], axis=1)               # depth_box3d.py:270-272
        bx, by, bz, w, l, h = Y, -X, Zc - zs / 2, ys, xs, zs              # origin (0.5,0.5,0.5) -> bottom; rt_mat, size swap
        cz = bz + h / 2
        rot = yaw + np.pi / 2
        sx, sy = pl[:, 0] - bx, pl[:, 1] - by
        lx, ly = sx * np.cos(rot) - sy * np.sin(rot), sx * np.sin(rot) + sy * np.cos(rot)
        inside = (np.abs(pl[:, 2] - cz) <= h / 2) & (lx > -l / 2) & (lx < l / 2) & (ly > -w / 2) & (ly < w / 2)
        margin = np.minimum.reduce([np.abs(np.abs(pl[:, 2] - cz) - h / 2), np.abs(np.abs(lx) - l / 2), np.abs(np.abs(ly) - w / 2)])
        Rm = np.array([[np.cos(-yaw), -np.sin(-yaw), 0.0], [np.sin(-yaw), np.cos(-yaw), 0.0], [0.0, 0.0, 1.0]])
        A = np.eye(4)                                                     # rotation = -rot, translation = centre
        A[:3, :3], A[:3, 3] = Rm, D[m, :3]
        centered = (np.linalg.inv(A) @ np.concatenate([p, np.ones((len(p), 1))], axis=1).T).T[:, :3]
        return inside, centered, margin

    # float32 rounding may decide a point within 1e-4 m of a face either way: such points are not part of the statement
    keep = np.all([reference(m)[2] > 1e-4 for m in range(M)], axis=0)
    p = p[keep]
    assert len(p) > 1000
    ours_pts = np.stack([p[:, 1], -p[:, 0], p[:, 2]], axis=1).astype(np.float32)
    ours_boxes = np.stack([D[:, 1], -D[:, 0], D[:, 2], D[:, 4], D[:, 3], D[:, 5], D[:, 6]], axis=1).astype(np.float32)
    n = 64
    rand = g.integers(0, 1 << 32, (M, n), dtype=np.uint64).astype(np.uint32).view(np.int32)
    clouds, lengths = R.crop_boxes(ours_pts, ours_boxes, n, frame="box", rand=rand, z_is_centre=True)
    for m in range(M):
        inside, centered, _ = reference(m)
        idx = np.nonzero(inside)[0]
        assert lengths[m] == idx.size and idx.size > 0
        pick = idx[R.sample_index(rand.view(np.uint32)[m], idx.size).astype(np.int64)]
        assert np.abs(clouds[m] - centered[pick]).max() < 1e-4        # same points, same axes, same signs
