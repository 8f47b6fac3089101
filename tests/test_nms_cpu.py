"""CPU: the section-A4 entry points (BEV overlap, NMS, track suppression) exist and refuse what they must, and the numpy
restatements the GPU tests compare against (tests/nms_ref.py) are right: the float64 restatement of the reference's
rotated overlap agrees with an independent method (Sutherland-Hodgman clipping, written here), the sweep agrees with a
plain greedy loop, and the NMS inputs keep every IoU away from their threshold.

d32, the largest |IoU(float32 restatement) - IoU(float64 restatement)| over the case set (the yardstick of the GPU
tolerance, 4 x d32): 4.38e-06 (numpy 2.2, x86-64; the pair behind it: two 2 x 5 m boxes 80 m from the origin, IoU 0.247).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import nms_ref as R
from conftest import ROOT

NEW_SYMBOLS = ("pcr_nearest_bev_f32", "pcr_bev_frames_f32", "pcr_iou_bev_f32", "pcr_nms_ok", "pcr_nms_ws_bytes",
               "pcr_nms_f32", "pcr_track_nms_f32")
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_abi_is_17(lib):
    from pcr_amd import abi
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
        assert re.search(r"\b%s\s*\(" % s, header), "include/pcr.h does not declare %s" % s
        assert s in abi.SIGNATURES
        assert "f" not in abi.kinds(abi.SIGNATURES[s])[1] and "l" not in abi.kinds(abi.SIGNATURES[s])[1]
    assert lib.pcr_abi_version() == 17
    assert (header_int("PCR_IOU_AXIS"), header_int("PCR_IOU_ROTATED"), header_int("PCR_IOU_OVERLAP")) == (0, 1, 2)


def test_ok_ranges_and_workspace_size(lib):
    top = header_int("PCR_NMS_MAX")
    assert top == 4096
    ok, ws = lib.pcr_nms_ok, lib.pcr_nms_ws_bytes
    assert ok(0) == 1 and ok(1) == 1 and ok(top) == 1 and ok(top + 1) == 0 and ok(-1) == 0
    assert ws(-1) == 0 and ws(top + 1) == 0
    for N in (1, 64, 65, 1000, top):
        nb = (N + 63) // 64
        assert ws(N) >= 32 * N + 8 * N * nb, "no room for the ranked table and the mask at N = %d" % N
    assert ws(top) < 2 ** 31


def test_null_and_out_of_range_arguments_return_invalid(lib):
    fbuf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    p, i = ctypes.cast(fbuf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    # (host pointers: each call below must be refused before anything is launched)
    near, frames, iou = lib.pcr_nearest_bev_f32, lib.pcr_bev_frames_f32, lib.pcr_iou_bev_f32
    for fn in (near, frames):
        assert fn(None, None, 4, None) == INVALID and fn(p, None, 4, None) == INVALID and fn(None, p, 4, None) == INVALID
        assert fn(p, p, -1, None) == INVALID
        assert fn(None, None, 0, None) == 0
    top = header_int("PCR_IOU_MAX_BOXES")
    assert iou(None, p, p, 2, 2, 1, None) == INVALID and iou(p, None, p, 2, 2, 1, None) == INVALID
    assert iou(p, p, None, 2, 2, 1, None) == INVALID
    assert iou(p, p, p, 2, 2, 3, None) == INVALID and iou(p, p, p, 2, 2, -1, None) == INVALID          # kind
    assert iou(p, p, p, -1, 2, 1, None) == INVALID and iou(p, p, p, 2, top + 1, 1, None) == INVALID
    assert iou(None, None, None, 0, 5, 1, None) == 0 and iou(None, None, None, 5, 0, 0, None) == 0
    nms = lib.pcr_nms_f32
    good = [p, p, p, i, i, i, i, p]
    for k in range(len(good)):
        args = list(good)
        args[k] = None
        assert nms(*args, 4, 1, 0, None) == INVALID, "NULL argument %d" % k
    assert nms(*good, 4097, 1, 0, None) == INVALID and nms(*good, -1, 1, 0, None) == INVALID
    assert nms(*good, 4, 2, 0, None) == INVALID and nms(*good, 4, -1, 0, None) == INVALID              # kind: no OVERLAP
    assert nms(*good[:7], ctypes.c_void_p(p.value + 4), 4, 1, 0, None) == INVALID                      # ws alignment
    assert nms(*([None] * 8), 0, 1, 0, None) == 0
    trk = lib.pcr_track_nms_f32
    good = [p, i, p, p, i]
    for k in range(len(good)):
        args = list(good)
        args[k] = None
        assert trk(*args, 4, None) == INVALID, "NULL argument %d" % k
    assert trk(*good, 4097, None) == INVALID and trk(*good, -1, None) == INVALID
    assert trk(*([None] * 5), 0, None) == 0


def test_host_tensors_raise_from_every_entry_point():
    import torch
    from mmdet3d import ops
    from pcr_amd import nms as M
    from pcr_amd._lib import PcrError
    b5, b7, s, c = torch.zeros(3, 5), torch.zeros(3, 7), torch.zeros(3), torch.zeros(3, dtype=torch.int32)
    for call in (lambda: M.nearest_bev(b7), lambda: M.bev_frames(b5), lambda: M.iou_bev(b5, b5),
                 lambda: M.nms(b5, s, 0.5), lambda: M.track_nms(b5, c, s, 0.5), lambda: M.suppress_tracks(b7, c, s, 0.5),
                 lambda: ops.boxes_iou_bev(b5, b5), lambda: ops.nms_gpu(b5, s, 0.5), lambda: ops.nms_normal_gpu(b5, s, 0.5)):
        with pytest.raises(PcrError):
            call()
    assert set(("boxes_iou_bev", "nms_gpu", "nms_normal_gpu")) <= set(ops.__all__)
    want = np.array([[0, 0, 2, 4, 0.5]], np.float32)
    assert np.array_equal(ops.xywhr2xyxyr(torch.tensor([[1.0, 2.0, 2.0, 4.0, 0.5]])).numpy(), want)


# ---- 2. the rotated overlap against exact geometry ---------------------------------------------------------------------
def corners64(box):
    x1, y1, x2, y2, ang = (float(v) for v in box)
    cx, cy, c, s = (x1 + x2) / 2, (y1 + y2) / 2, np.cos(ang), np.sin(ang)
    # the reference's rotation (rotate_around_center): it turns by -angle; both boxes turn the same way
    return [((x - cx) * c + (y - cy) * s + cx, -(x - cx) * s + (y - cy) * c + cy)
            for x, y in ((x1, y1), (x2, y1), (x2, y2), (x1, y2))]


def polygon_area(poly):
    return 0.5 * sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1]
                     for k in range(len(poly)))


def clip_area(box_a, box_b):
    """Sutherland-Hodgman: the subject polygon a clipped by every edge of the convex polygon b, float64"""
    subject, clip = corners64(box_a), corners64(box_b)
    if polygon_area(clip) < 0:
        clip = clip[::-1]
    if abs(polygon_area(clip)) == 0 or abs(polygon_area(subject)) == 0:
        return 0.0
    for k in range(4):
        (ex1, ey1), (ex2, ey2) = clip[k], clip[(k + 1) % 4]
        side = lambda p: (ex2 - ex1) * (p[1] - ey1) - (ey2 - ey1) * (p[0] - ex1)        # >= 0: inside (left of the edge)
        out = []
        for m in range(len(subject)):
            cur, prev = subject[m], subject[m - 1]
            dc, dp = side(cur), side(prev)
            if (dc >= 0) != (dp >= 0):
                t = dp / (dp - dc)
                out.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
            if dc >= 0:
                out.append(cur)
        subject = out
        if not subject:
            return 0.0
    return abs(polygon_area(subject))


def near_degenerate(box_a, box_b, band=1e-4):
    """a corner of one box within `band` of the other's boundary line segments: where MARGIN decides, not geometry"""
    for p, q in ((corners64(box_a), corners64(box_b)), (corners64(box_b), corners64(box_a))):
        for (x, y) in p:
            for k in range(4):
                (x1, y1), (x2, y2) = q[k], q[(k + 1) % 4]
                dx, dy = x2 - x1, y2 - y1
                L2 = dx * dx + dy * dy
                t = 0.0 if L2 == 0 else min(1.0, max(0.0, ((x - x1) * dx + (y - y1) * dy) / L2))
                if np.hypot(x - (x1 + t * dx), y - (y1 + t * dy)) < band:
                    return True
    return False


@pytest.fixture(scope="module")
def pair_set():
    """every pair of the GPU test's matrices, flattened: (a, b, named {index: name}, overlap64, overlap32); a named box
    met with another pair's named box is marked "mixed": neither a random case nor one with a known answer"""
    aa, bb, named = [], [], {}
    for A, B in R.IOU_SHAPES:
        a, b, where = R.iou_case(A, B)
        ii, jj = np.repeat(np.arange(A), B), np.tile(np.arange(B), A)
        base = sum(len(x) for x in aa)
        for i in {i for i, _ in where.values()}:
            for j in {j for _, j in where.values()}:
                named[base + i * B + j] = "mixed"
        for name, (i, j) in where.items():
            named[base + i * B + j] = name
        aa.append(a[ii])
        bb.append(b[jj])
    a, b = np.concatenate(aa), np.concatenate(bb)
    o64 = R.overlap_pairs(a, b, R.frames_of(a, np.float64), R.frames_of(b, np.float64), np.float64)
    o32 = R.overlap_pairs(a, b, R.frames_of(a, np.float32), R.frames_of(b, np.float32), np.float32)
    return a, b, named, o64, o32


def test_float64_restatement_agrees_with_polygon_clipping(pair_set):
    a, b, named, (area64, cnt), _ = pair_set
    compared_by_name = {n: c for n, _, _, c in R.SPECIAL}
    assert set(named.values()) == set(compared_by_name) | {"mixed"}           # every named pair is in the set
    compared_by_name["mixed"] = False
    assert cnt.max() <= R.SLOTS
    random_n = random_out = checked = 0
    worst = 0.0
    for p in np.nonzero((cnt > 0) | np.isin(np.arange(len(a)), list(named)))[0]:       # cnt == 0 pairs: see below
        if p in named:
            if not compared_by_name[named[p]]:
                continue
        else:
            random_n += 1
            if near_degenerate(a[p], b[p]):
                random_out += 1
                continue
        exact = clip_area(a[p], b[p])
        worst = max(worst, abs(area64[p] - exact))
        assert abs(area64[p] - exact) <= 1e-9 * max(1.0, exact), (named.get(p, "random"), p, area64[p], exact)
        checked += 1
    # pairs without a polygon point: disjoint by the restatement; exact geometry must agree on a sample of the closest
    far = np.nonzero(cnt == 0)[0]
    d = np.hypot((a[far, 0] + a[far, 2] - b[far, 0] - b[far, 2]) / 2, (a[far, 1] + a[far, 3] - b[far, 1] - b[far, 3]) / 2)
    for p in far[np.argsort(d)[:300]]:
        if p not in named and not near_degenerate(a[p], b[p]):
            assert clip_area(a[p], b[p]) <= 1e-12, p
    print("clipping: %d pairs compared, worst |area64 - exact| = %.3g; %d of %d random overlapping pairs excluded"
          % (checked, worst, random_out, random_n))
    assert checked >= 100 and random_n >= 100
    assert random_out <= 0.05 * random_n, "too many excluded: %d of %d" % (random_out, random_n)


def test_named_pairs_have_the_values_geometry_gives(pair_set):
    a, b, named, (area64, cnt), (area32, _) = pair_set
    by_name = {name: p for p, name in named.items()}
    want = {"disjoint": 0.0, "contained": 2.0, "square_turned_45": 8 * (np.sqrt(2) - 1), "crossing_plus": 1.0,
            "zero_area_line": 0.0, "zero_area_point": 0.0, "identical": 10.0, "identical_axis": 10.0,
            "touching_edge": 0.0, "shared_edge_part": 0.0}
    for name, v in want.items():
        assert abs(area64[by_name[name]] - v) < 1e-9, (name, area64[by_name[name]], v)
        assert abs(area32[by_name[name]] - v) < 1e-4, (name, area32[by_name[name]], v)
    assert cnt[by_name["square_turned_45"]] == 8                                # eight crossings, no corner inside


def test_float32_against_float64_restatement_d32(pair_set):
    a, b, named, (area64, _), (area32, _) = pair_set
    assert area32.dtype == np.float32 and area64.dtype == np.float64
    s = lambda x, T: ((x[:, 2].astype(T) - x[:, 0].astype(T)) * (x[:, 3].astype(T) - x[:, 1].astype(T)))
    iou = lambda ov, T: ov / np.fmax(s(a, T) + s(b, T) - ov, T(R.EPS))
    diff = np.abs(iou(area32, np.float32).astype(np.float64) - iou(area64, np.float64))
    d32 = float(diff.max())
    p = int(diff.argmax())
    print("d32 = %.3g at pair %d (%s): a = %s b = %s iou64 = %.6f" % (d32, p, named.get(p, "random"), a[p], b[p],
                                                                     iou(area64, np.float64)[p]))
    assert np.isfinite(d32)


# ---- 3. ranking, sweep, track rule -------------------------------------------------------------------------------------
def test_ranking_rule():
    s = np.array([0.5, np.nan, 0.75, 0.5, -0.0, 0.0, np.nan, 0.75], np.float32)
    assert R.rank_order(s).tolist() == [2, 7, 0, 3, 4, 5, 1, 6]               # ties by index, -0 == +0, NaNs last
    g = np.random.default_rng(0)
    s = g.integers(0, 9, 200).astype(np.float32)
    assert R.rank_order(s).tolist() == np.argsort(-s, kind="stable").tolist()


@pytest.mark.parametrize("kind", ["axis", "rotated"])
def test_nms_inputs_keep_clear_of_the_threshold_and_sweep_equals_plain_greedy(kind):
    """runs every generator the GPU test uses (they assert the 1e-3 gap themselves) and checks the mask + sweep
    restatement against the textbook loop on the same thresholded matrix"""
    cases = [R.nms_case(N, kind) + (None,) for N in R.NMS_SIZES] + list(R.named_nms_cases(kind).values())
    kept_some = suppressed_some = 0
    for boxes, scores, thresh, iou, want in cases:
        m = R.iou64(boxes, kind)
        N = len(boxes)
        vals = m[np.triu_indices(N, 1)]
        assert not len(vals) or np.abs(vals - thresh).min() > R.GAP
        for pre_max in (None, 100) if N == 130 else (None,):
            order, keep, count, info = R.nms(boxes, scores, thresh, kind, pre_max, iou=iou)
            assert info == 0 and sorted(order.tolist()) == list(range(N)) and (keep[count:] == -1).all()
            used = order if pre_max is None else order[:pre_max]
            assert keep[:count].tolist() == R.greedy_plain(m > thresh, used)
            if want is not None:
                assert keep[:count].tolist() == want
            kept_some += count > 0
            suppressed_some += count < len(used)
    assert kept_some >= 10 and suppressed_some >= 6
    chain = R.named_nms_cases(kind)["chain"]
    assert R.track_nms(chain[0], [0, 0, 0], chain[1], chain[2]).tolist() == [0, 1, 1]      # the pairwise rule: not greedy's


def test_nan_scores_and_non_finite_boxes_are_reported():
    boxes, scores, thresh, _ = R.nms_case(65, "axis")
    s = scores.copy()
    s[7] = np.nan
    order, keep, count, info = R.nms(boxes, s, thresh)
    assert info == 1 and count == 0 and (keep == -1).all() and order[-1] == 7
    b = boxes.copy()
    b[R.rank_order(scores)[64], 2] = np.inf
    assert R.nms(b, scores, thresh)[3] == 1 and R.nms(b, scores, thresh, pre_max=64)[3] == 0   # unused: not looked at
    b = boxes.copy()
    b[3, 4] = np.nan
    assert R.nms(b, scores, thresh, "axis")[3] == 0 and R.nms(b, scores, thresh, "rotated", iou=np.zeros((65, 65)))[3] == 1


def test_track_rule_literally():
    for N in (1, 2, 64, 65, 200):
        boxes7, classes, scores = R.track_case(N)
        b5 = R.nearest_bev(boxes7)
        thresh = 0.1
        iou = R.iou_axis(b5, b5)
        want = np.zeros(N, np.int32)
        for i in range(N):
            for j in range(i + 1, N):
                if classes[i] == classes[j] and iou[i, j] > np.float32(thresh):
                    if scores[i] - scores[j] <= 0:
                        want[i] = 1
                    else:
                        want[j] = 1
        got = R.track_nms(b5, classes, scores, thresh)
        assert np.array_equal(got, want)
        if N >= 64:
            assert 0 < got.sum() < N
            eq = [(i, j) for i in range(N) for j in range(i + 1, N) if classes[i] == classes[j]
                  and iou[i, j] > np.float32(thresh) and scores[i] == scores[j]]
            assert eq, "no pair of equal scores: the <= 0 side is not exercised"


def test_nearest_bev_against_the_formula_in_float64():
    boxes7 = R.track_case(200)[0]
    boxes7[:8, 6] = [0.0, np.pi / 4, -np.pi / 4, np.pi / 2, 3 * np.pi / 4, -3.0, 7.0, np.float32(np.pi / 4) + 1e-6]
    got = R.nearest_bev(boxes7)
    b = boxes7.astype(np.float64)
    r = np.abs(b[:, 6] - np.floor(b[:, 6] / np.pi + 0.5) * np.pi)
    clear = np.abs(r - np.pi / 4) > 1e-5                                        # away from the switch, both agree
    sw = r > np.pi / 4
    w, l = np.where(sw, b[:, 4], b[:, 3]), np.where(sw, b[:, 3], b[:, 4])
    want = np.stack([b[:, 0] - w / 2, b[:, 1] - l / 2, b[:, 0] + w / 2, b[:, 1] + l / 2, 0 * w], 1)
    assert clear.sum() >= 195 and sw[clear].any() and (~sw[clear]).any()
    assert np.abs(got[clear] - want[clear]).max() < 1e-5
