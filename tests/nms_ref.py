"""numpy restatements of include/pcr.h section A4 (BEV overlap and suppression) and the case generators the CPU and the
GPU tests share.

float32, operation for operation, meant to equal the kernels bit for bit: `nearest_bev`, `iou_axis`, `rank_order`,
`nms` (mask + sweep) and `track_nms`.  The rotated overlap has two restatements of the reference's algorithm
(ops/iou3d/src/iou3d_kernel.cu:127-251), both `overlap_pairs`: dtype float32 with the (cos, sin) table as an input -- on
the GPU that table comes from pcr_bev_frames_f32, so the only operations left to differ are atan2 and nothing else --
and dtype float64 with its own trigonometry.  Everything is vectorised over the pairs; the per-pair control flow of the
reference (appends, the bubble sort's bounds) is carried by masks.
"""
import numpy as np

F = np.float32
EPS = 1e-8            # iou3d_kernel.cu:16
MARGIN = 1e-5         # :56
SLOTS = 24            # 16 crossings + 8 corners
KINDS = ("axis", "rotated", "overlap")


# ---- float32, bit for bit -------------------------------------------------------------------------------------------
def nearest_bev(boxes7):
    b = np.asarray(boxes7, F).reshape(-1, 7)
    pi, quarter, half, two = F(np.pi), F(np.pi / 4), F(0.5), F(2)
    rz = b[:, 6]
    r = np.abs(rz - np.floor(rz / pi + half) * pi)
    swap = r > quarter
    w, l = np.where(swap, b[:, 4], b[:, 3]), np.where(swap, b[:, 3], b[:, 4])
    out = np.stack([b[:, 0] - w / two, b[:, 1] - l / two, b[:, 0] + w / two, b[:, 1] + l / two, np.zeros_like(rz)], 1)
    assert out.dtype == F
    return out


def iou_axis(a, b):
    """iou_normal of every pair: a (A, >=4), b (B, >=4) -> (A, B) float32"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    A, B = a[:, None, :], b[None, :, :]
    with np.errstate(all="ignore"):
        left, right = np.fmax(A[..., 0], B[..., 0]), np.fmin(A[..., 2], B[..., 2])
        top, bottom = np.fmax(A[..., 1], B[..., 1]), np.fmin(A[..., 3], B[..., 3])
        width, height = np.fmax(right - left, F(0)), np.fmax(bottom - top, F(0))
        inter = width * height
        sa = (A[..., 2] - A[..., 0]) * (A[..., 3] - A[..., 1])
        sb = (B[..., 2] - B[..., 0]) * (B[..., 3] - B[..., 1])
        out = inter / np.fmax(sa + sb - inter, F(EPS))
    assert out.dtype == F
    return out


def rank_order(scores):
    """-> order (N,) int32: indices by descending score, equal scores lowest index first, NaNs last by index"""
    s = np.asarray(scores, F)
    N = len(s)
    idx = np.arange(N)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        before = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (idx[None, :] < idx[:, None]))
    before = np.where(nan[:, None], ~nan[None, :] | (idx[None, :] < idx[:, None]), before)
    order = np.empty(N, np.int32)
    order[before.sum(1)] = idx
    return order


def nms(boxes5, scores, thresh, kind="axis", pre_max=None, iou=None):
    """-> order (N,), keep (N,) padded with -1, count, info.  The reference's mask words and its sweep
    (iou3d_kernel.cu:284-333, iou3d.cpp:128-143).  iou: the (N, N) matrix over the ORIGINAL indices to threshold (the
    rotated kind: the caller chooses the restatement); None = iou_axis."""
    boxes5, scores = np.asarray(boxes5, F).reshape(-1, 5), np.asarray(scores, F)
    N = len(scores)
    order = rank_order(scores)
    n = N if pre_max is None or pre_max <= 0 or pre_max >= N else int(pre_max)
    used = boxes5[order[:n]]
    cols = 5 if kind == "rotated" else 4
    if np.isnan(scores).any() or not np.isfinite(used[:, :cols]).all():
        return order, np.full(N, -1, np.int32), 0, 1
    m = iou_axis(used, used) if iou is None else np.asarray(iou)[np.ix_(order[:n], order[:n])]
    over = (m > (F(thresh) if m.dtype == F else float(F(thresh)))) & np.triu(np.ones((n, n), bool), 1)
    nb = (n + 63) // 64
    padded = np.zeros((n, nb * 64), np.uint64)
    padded[:, :n] = over
    words = (padded.reshape(n, nb, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    remv = np.zeros(nb, np.uint64)
    keep = []
    for i in range(n):
        blk, bit = i // 64, np.uint64(i % 64)
        if not (remv[blk] >> bit) & np.uint64(1):
            keep.append(order[i])
            remv[blk:] |= words[i, blk:]
    out = np.full(N, -1, np.int32)
    out[:len(keep)] = keep
    return order, out, len(keep), 0


def greedy_plain(over, order):
    """the textbook O(N^2) greedy loop on a boolean overlap matrix over original indices (the sweep is checked against it)"""
    keep = []
    for i in order:
        if not any(over[k, i] or over[i, k] for k in keep):
            keep.append(int(i))
    return keep


def track_nms(boxes5, classes, scores, thresh):
    """-> suppressed (N,) int32 (virtual_tracker.py:249-255 on iou_normal)"""
    b, c, s = np.asarray(boxes5, F).reshape(-1, 5), np.asarray(classes), np.asarray(scores, F)
    N = len(s)
    hit = (iou_axis(b, b) > F(thresh)) & np.triu(np.ones((N, N), bool), 1) & (c[:, None] == c[None, :])
    d = s[:, None] - s[None, :]
    return ((hit & (d <= 0)).any(1) | (hit & (d > 0)).any(0)).astype(np.int32)


# ---- the rotated overlap, float32 or float64 ------------------------------------------------------------------------
def frames_of(boxes5, T):
    ang = np.asarray(boxes5, F)[:, 4].astype(T)
    return np.stack([np.cos(ang), np.sin(ang)], 1).astype(T)


def _rot(cx, cy, c, s, x, y):
    return (x - cx) * c + (y - cy) * s + cx, -(x - cx) * s + (y - cy) * c + cy


def _cross3(p1, p2, p0):
    return (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])


def _in_box(x1, y1, x2, y2, c, s, p, T):
    two, margin = T(2), T(MARGIN)
    cx, cy = (x1 + x2) / two, (y1 + y2) / two
    ac, as_ = c, -s
    rx = (p[0] - cx) * ac + (p[1] - cy) * as_ + cx
    ry = -(p[0] - cx) * as_ + (p[1] - cy) * ac + cy
    return (rx > x1 - margin) & (rx < x2 + margin) & (ry > y1 - margin) & (ry < y2 + margin)


def _intersection(p1, p0, q1, q0, T):
    rect = (np.fmin(p0[0], p1[0]) <= np.fmax(q0[0], q1[0])) & (np.fmin(q0[0], q1[0]) <= np.fmax(p0[0], p1[0])) & \
           (np.fmin(p0[1], p1[1]) <= np.fmax(q0[1], q1[1])) & (np.fmin(q0[1], q1[1]) <= np.fmax(p0[1], p1[1]))
    s1, s2, s3, s4 = _cross3(q0, p1, p0), _cross3(p1, q1, p0), _cross3(p0, q1, q0), _cross3(q1, p1, q0)
    ok = rect & (s1 * s2 > 0) & (s3 * s4 > 0)
    s5 = _cross3(q1, p1, p0)
    main = np.abs(s5 - s1) > T(EPS)
    xm, ym = (s5 * q0[0] - s1 * q1[0]) / (s5 - s1), (s5 * q0[1] - s1 * q1[1]) / (s5 - s1)
    a0, b0, c0 = p0[1] - p1[1], p1[0] - p0[0], p0[0] * p1[1] - p1[0] * p0[1]
    a1, b1, c1 = q0[1] - q1[1], q1[0] - q0[0], q0[0] * q1[1] - q1[0] * q0[1]
    D = a0 * b1 - a1 * b0
    xa, ya = (b0 * c1 - b1 * c0) / D, (a1 * c0 - a0 * c1) / D
    return ok, np.where(main, xm, xa), np.where(main, ym, ya)


def overlap_pairs(a, b, fa, fb, T=F):
    """box_overlap of pair p = (a[p], b[p]): a, b (P, >=4) boxes, fa, fb (P, 2) their (cos, sin) -> (area (P,), cnt (P,))
    in dtype T, the reference's algorithm step by step (the steps are named in include/pcr.h)"""
    a, b, fa, fb = (np.asarray(x, F).astype(T) if x.dtype != T else x for x in map(np.asarray, (a, b, fa, fb)))
    P = len(a)
    two = T(2)
    with np.errstate(all="ignore"):
        ax1, ay1, ax2, ay2 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        bx1, by1, bx2, by2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        acx, acy, bcx, bcy = (ax1 + ax2) / two, (ay1 + ay2) / two, (bx1 + bx2) / two, (by1 + by2) / two
        ca = [_rot(acx, acy, fa[:, 0], fa[:, 1], x, y) for x, y in ((ax1, ay1), (ax2, ay1), (ax2, ay2), (ax1, ay2))]
        cb = [_rot(bcx, bcy, fb[:, 0], fb[:, 1], x, y) for x, y in ((bx1, by1), (bx2, by1), (bx2, by2), (bx1, by2))]
        ca.append(ca[0])
        cb.append(cb[0])
        px, py = np.zeros((P, SLOTS), T), np.zeros((P, SLOTS), T)
        cnt = np.zeros(P, np.int64)
        sx, sy = np.zeros(P, T), np.zeros(P, T)

        def append(flag, x, y):
            nonlocal sx, sy
            k = np.nonzero(flag)[0]
            px[k, cnt[k]], py[k, cnt[k]] = x[k], y[k]
            cnt[k] += 1
            sx, sy = np.where(flag, sx + x, sx), np.where(flag, sy + y, sy)

        for i in range(4):
            for j in range(4):
                append(*_intersection(ca[i + 1], ca[i], cb[j + 1], cb[j], T))
        for k in range(4):
            append(_in_box(ax1, ay1, ax2, ay2, fa[:, 0], fa[:, 1], cb[k], T), *cb[k])
            append(_in_box(bx1, by1, bx2, by2, fb[:, 0], fb[:, 1], ca[k], T), *ca[k])
        cx, cy = sx / cnt.astype(T), sy / cnt.astype(T)
        ang = np.arctan2(py - cy[:, None], px - cx[:, None])
        assert ang.dtype == T
        m = int(cnt.max()) if P else 0
        for j in range(m - 1):
            for i in range(m - j - 1):
                sw = (i < cnt - j - 1) & (ang[:, i] > ang[:, i + 1])
                for arr in (px, py, ang):
                    lo, hi = arr[:, i].copy(), arr[:, i + 1].copy()
                    arr[:, i], arr[:, i + 1] = np.where(sw, hi, lo), np.where(sw, lo, hi)
        x0, y0 = px[:, 0], py[:, 0]
        area = np.zeros(P, T)
        for k in range(m - 1):
            term = (px[:, k] - x0) * (py[:, k + 1] - y0) - (py[:, k] - y0) * (px[:, k + 1] - x0)
            area = np.where(k < cnt - 1, area + term, area)
        area = np.where(cnt == 0, T(0), np.abs(area) / two)
    assert area.dtype == T
    return area, cnt


def iou_matrix(a, b, kind, T=F, fa=None, fb=None):
    """(A, B) matrix of `kind` in dtype T ("axis" is float32 only); fa / fb: the (cos, sin) tables, None = numpy's own"""
    if kind == "axis":
        return iou_axis(a, b)
    a, b = np.asarray(a, F), np.asarray(b, F)
    A, B = len(a), len(b)
    fa = frames_of(a, T) if fa is None else np.asarray(fa).astype(T)
    fb = frames_of(b, T) if fb is None else np.asarray(fb).astype(T)
    ii, jj = np.repeat(np.arange(A), B), np.tile(np.arange(B), A)
    # pairs whose circumscribed circles are a metre apart have no crossing and no corner inside: exactly 0 either way
    ca, cb = (a[:, :2].astype(np.float64) + a[:, 2:4]) / 2, (b[:, :2].astype(np.float64) + b[:, 2:4]) / 2
    ra, rb = np.hypot(*(a[:, 2:4] - a[:, :2]).astype(np.float64).T) / 2, np.hypot(*(b[:, 2:4] - b[:, :2]).astype(np.float64).T) / 2
    near = np.hypot(*(ca[ii] - cb[jj]).T) <= ra[ii] + rb[jj] + 1.0
    ii, jj = ii[near], jj[near]
    area = np.zeros((A, B), T)
    area[ii, jj] = overlap_pairs(a[ii].astype(T), b[jj].astype(T), fa[ii], fb[jj], T)[0]
    if kind == "overlap":
        return area
    aT, bT = a.astype(T), b.astype(T)
    sa = ((aT[:, 2] - aT[:, 0]) * (aT[:, 3] - aT[:, 1]))[:, None]
    sb = ((bT[:, 2] - bT[:, 0]) * (bT[:, 3] - bT[:, 1]))[None, :]
    with np.errstate(all="ignore"):
        out = area / np.fmax(sa + sb - area, T(EPS))
    assert out.dtype == T
    return out


# ---- case generators ----------------------------------------------------------------------------------------------------
def xyxyr(cx, cy, w, l, ang):
    cx, cy, w, l, ang = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (cx, cy, w, l, ang)))
    return np.stack([cx - w / 2, cy - l / 2, cx + w / 2, cy + l / 2, ang], -1).astype(F)


def street_boxes(n, seed, spread=150.0):
    """street-sized boxes 0 .. spread m from the origin, any heading"""
    g = np.random.default_rng(seed)
    rad, phi = g.uniform(0, spread, n), g.uniform(0, 2 * np.pi, n)
    return xyxyr(rad * np.cos(phi), rad * np.sin(phi), g.uniform(0.5, 3.0, n), g.uniform(0.5, 12.0, n),
                 g.uniform(-np.pi, np.pi, n))


def near_copies(boxes, seed, shift=1.5):
    """one box near each given box: shifted by ~shift m, resized, turned -- pairs that overlap more often than not"""
    g = np.random.default_rng(seed)
    n = len(boxes)
    b = boxes.astype(np.float64)
    cx, cy, w, l = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return xyxyr(cx + g.normal(0, shift, n), cy + g.normal(0, shift, n), w * g.uniform(0.7, 1.3, n), l * g.uniform(0.7, 1.3, n),
                 b[:, 4] + g.normal(0, 0.6, n))


# named pairs: (name, box a, box b, compared with exact geometry?)  The excluded ones are the cases where the reference's
# MARGIN / EPS rules differ from exact geometry by design: its strict crossing test finds nothing on coincident edges and
# what it returns hangs on which corners the 1e-5 margin lets in.
SPECIAL = [
    ("disjoint", xyxyr(0, 0, 2, 4, 0.3), xyxyr(30, -20, 2, 4, -1.0), True),
    ("contained", xyxyr(5, 5, 4, 8, 0.4), xyxyr(5.2, 4.9, 1, 2, 1.1), True),
    ("square_turned_45", xyxyr(-3, 2, 2, 2, 0.0), xyxyr(-3, 2, 2, 2, np.pi / 4), True),
    ("crossing_plus", xyxyr(1, 1, 1, 6, 0.0), xyxyr(1, 1, 6, 1, 0.0), True),
    ("zero_area_line", xyxyr(0, 0, 0, 4, 0.2), xyxyr(0.1, 0, 2, 2, 0.7), True),
    ("zero_area_point", xyxyr(0, 0, 0, 0, 0.0), xyxyr(0, 0, 2, 2, 0.5), True),
    ("touching_edge", xyxyr(0, 0, 2, 4, 0.0), xyxyr(2, 0, 2, 4, 0.0), False),
    ("identical", xyxyr(4, -6, 2, 5, 0.6), xyxyr(4, -6, 2, 5, 0.6), False),
    ("identical_axis", xyxyr(4, -6, 2, 5, 0.0), xyxyr(4, -6, 2, 5, 0.0), False),
    ("corner_on_edge", xyxyr(0, 0, 2, 2, 0.0), xyxyr(1 + np.sqrt(0.5) * 2, 0, 2, 2, np.pi / 4), False),
    ("shared_edge_part", xyxyr(0, 0, 2, 2, 0.0), xyxyr(0.5, 2, 1, 2, 0.0), False),
]


def iou_case(A, B, seed=0):
    """a (A, 5), b (B, 5): random street boxes; b_j has a near copy among a where there is room; the named pairs sit on
    the diagonal from the end (a[A-1-k], b[B-1-k]) where there is room for them.  -> a, b, {name: (i, j)}"""
    b = street_boxes(B, seed * 2 + 1)
    a = street_boxes(A, seed * 2 + 2)
    m = min(A, B)
    a[:m] = near_copies(b[:m], seed * 2 + 3)
    where = {}
    if m > len(SPECIAL):
        for k, (name, sa, sb, _) in enumerate(SPECIAL):
            a[A - 1 - k], b[B - 1 - k] = sa, sb
            where[name] = (A - 1 - k, B - 1 - k)
    return a, b, where


IOU_SHAPES = [(1, 1), (15, 17), (64, 64), (65, 130)]
NMS_SIZES = [0, 1, 2, 63, 64, 65, 130, 1000]
GAP = 1e-3


def nms_case(N, kind, seed=0, thresh=None):
    """boxes (N, 5), scores (N,), thresh, iou (N, N) float64 (None for the axis kind: its restatement is exact) for an NMS
    test: clusters of near copies so that a good share is suppressed, scores with ties.  Asserts, in float64, that no
    pair's IoU lies within GAP of the threshold -- a condition on the INPUTS, under which the kept list is demanded
    exactly.  If a draw violates it the threshold moves to the middle of the widest gap near the wanted value."""
    g = np.random.default_rng(1000 * N + seed + (7 if kind == "rotated" else 0))
    base = street_boxes(max(1, (N + 2) // 3), 31 * N + seed, spread=40.0 + N / 4)
    boxes = np.concatenate([base, near_copies(base, seed + 1, 0.4), near_copies(base, seed + 2, 0.8)])[:N]
    if kind == "axis":
        boxes[:, 4] = 0
    scores = (g.integers(0, max(2, N // 2), N) / F(max(2, N // 2))).astype(F)          # ties in plenty
    return check_gap(boxes, scores, 0.3 if thresh is None else thresh, kind)


def iou64(boxes, kind):
    if kind == "axis":
        return iou_axis(boxes, boxes).astype(np.float64)
    return iou_matrix(boxes, boxes, "rotated", np.float64)


def check_gap(boxes, scores, thresh, kind):
    boxes, scores = np.asarray(boxes, F).reshape(-1, 5), np.asarray(scores, F)
    m = iou64(boxes, kind)
    vals = m[np.triu_indices(len(boxes), 1)]
    t = float(F(thresh))
    if len(vals) and np.abs(vals - t).min() <= GAP:                                     # move into the widest gap nearby
        v = np.sort(np.concatenate([vals[(vals > t - 0.1) & (vals < t + 0.1)], [t - 0.1, t + 0.1]]))
        k = int(np.argmax(np.diff(v)))
        t = float(F((v[k] + v[k + 1]) / 2))
    assert not len(vals) or np.abs(vals - t).min() > GAP, "an IoU lies within %g of the threshold %g" % (GAP, t)
    return boxes, scores, t, (None if kind == "axis" else m)


def named_nms_cases(kind):
    """{name: (boxes, scores, thresh, iou64 | None, expected keep)}"""
    ang = 0.0 if kind == "axis" else 0.5
    same = np.repeat(xyxyr(3, -2, 2, 4.5, ang)[None], 70, 0)
    apart = xyxyr(np.arange(70) * 9.0, np.arange(70) % 5 * 14.0, 2, 4.5, ang)
    g = np.random.default_rng(5)
    s70 = g.permutation(70).astype(F)
    chain = xyxyr([0.0, 0.9, 1.8], [0, 0, 0], 2, 4.5, 0.0)                   # A-B 0.38, B-C 0.38, A-C 0.05
    out = {
        "all_identical": (same, s70, 0.5, [int(np.argmax(s70))]),
        "all_disjoint": (apart, s70, 0.1, np.argsort(-s70).tolist()),
        "equal_scores": (apart, np.ones(70, F), 0.1, list(range(70))),
        "chain": (chain, np.array([3, 2, 1], F), 0.25, [0, 2]),
    }
    return {k: check_gap(b, s, t, kind) + (want,) for k, (b, s, t, want) in out.items()}


def track_case(N, seed=0):
    """boxes7 (N, 7), classes (N,) int32, scores (N,): clusters of near tracks, mixed classes, many equal scores"""
    g = np.random.default_rng(77 * N + seed)
    n0 = max(1, (N + 2) // 3)
    c = np.stack([g.uniform(-30, 30, n0), g.uniform(-30, 30, n0), g.uniform(-1, 1, n0), g.uniform(1.5, 2.5, n0),
                  g.uniform(3.5, 5.5, n0), g.uniform(1.4, 2.0, n0), g.uniform(-4, 4, n0)], 1)
    boxes = np.concatenate([c, c, c])[:N]
    boxes[:, :2] += g.normal(0, 0.5, (N, 2))
    boxes[:, 6] += g.normal(0, 0.2, N)
    classes = np.concatenate([g.integers(0, 3, n0)] * 3)[:N].astype(np.int32)
    classes[g.random(N) < 0.2] = 5                                                      # some copies change class
    scores = g.integers(1, 4, N).astype(F) + g.integers(0, 2, N).astype(F) / F(2)      # the tracker's len + score, ties
    return boxes.astype(F), classes, scores
