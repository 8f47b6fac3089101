"""numpy restatement of the association step (include/pcr.h section A3): what the GPU tests compare
pcr_assoc_pairs_i32 / pcr_assoc_cost_f32 / pcr_lsa_f32 against, bit for bit.

compare_pairs restates get_labels_to_compare (trackers/deprecated/tracking_point_reid.py:15-33), association_cost the
layout of get_cost_mat_margin with one tracking and one detection decision (tracking_association.py:22-53, :126-128),
lsa the rules pcr.h writes down for the assignment: every operation on np.float32 scalars / arrays, so each is rounded
to binary32 and nothing is contracted.
"""
import numpy as np

F = np.float32


def compare_pairs(track_labels, det_labels, track_lengths=None, det_lengths=None, min_points=2, num_classes=8, cap=None):
    """-> pairs (cap, 2) int32 padded with (0, 0), count (the true number of pairs)"""
    tl, dl = np.asarray(track_labels).astype(np.int64), np.asarray(det_labels).astype(np.int64)
    tok, dok = np.ones(tl.shape, bool), np.ones(dl.shape, bool)
    if track_lengths is not None:
        tok = np.asarray(track_lengths) >= min_points
    if det_lengths is not None:
        dok = np.asarray(det_lengths) >= min_points
    rows = []
    for x in range(num_classes):
        ts, ds = np.nonzero((tl == x) & tok)[0], np.nonzero((dl == x) & dok)[0]
        if len(ts) and len(ds):
            rows.append(np.stack([np.repeat(ts, len(ds)), np.tile(ds, len(ts))], axis=1))
    listed = np.concatenate(rows) if rows else np.zeros((0, 2), np.int64)
    count = len(listed)
    cap = len(tl) * len(dl) if cap is None else cap
    pairs = np.zeros((cap, 2), np.int32)
    pairs[:min(count, cap)] = listed[:cap]
    return pairs, count


def association_cost(logits, pairs, count, T, D, track_miss=None, det_new=None, dist=None, dist_max=22.0,
                     dist_penalty=3.0, fill=10000.0):
    """-> (T + D, D + T) float32"""
    cost = np.full((T + D, D + T), F(fill), F)
    k = min(int(count), len(pairs))
    t, d = pairs[:k, 0].astype(np.int64), pairs[:k, 1].astype(np.int64)
    val = -np.asarray(logits, F)[:k]
    if dist is not None:
        far = np.asarray(dist, F)[t, d] > F(dist_max)
        val = np.where(far, val + F(dist_penalty), val).astype(F)
    cost[t, d] = val
    cost[T + d, D + t] = val
    cost[np.arange(T), D + np.arange(T)] = F(0) if track_miss is None else np.asarray(track_miss, F)
    cost[T + np.arange(D), np.arange(D)] = F(0) if det_new is None else np.asarray(det_new, F)
    return cost


def lsa(cost, count_steps=False):
    """cost (R, C) -> col4row (R,) int32, row4col (C,) int32, u (R,) f32, v (C,) f32, info [, search steps]"""
    cost = np.ascontiguousarray(cost, F)
    R, C = cost.shape
    if not np.isfinite(cost).all():
        out = (np.full(R, -1, np.int32), np.full(C, -1, np.int32), np.zeros(R, F), np.zeros(C, F), 1)
        return out + (0,) if count_steps else out
    tr = R > C
    c = np.ascontiguousarray(cost.T) if tr else cost
    nr, nc = c.shape
    u, v = np.zeros(nr, F), np.zeros(nc, F)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    steps = 0
    for cur in range(nr):
        short = np.full(nc, np.inf, F)
        pred = np.full(nc, -1, np.int64)
        done = np.zeros(nc, bool)
        minv, i, sink = F(0), cur, -1
        for _ in range(nc):
            steps += 1
            r = ((c[i] - u[i]) - v) + minv
            upd = ~done & (r < short)
            short[upd] = r[upd]
            pred[upd] = i
            open_ = np.flatnonzero(~done)
            j = open_[np.argmin(short[open_])]           # the first (lowest-index) occurrence of the minimum
            minv = short[j]
            done[j] = True
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        assert sink >= 0
        u[cur] = u[cur] + minv
        dj = np.flatnonzero(done)
        delta = minv - short[dj]
        has_row = dj != sink
        u[row4col[dj[has_row]]] += delta[has_row]
        v[dj] -= delta
        j = sink
        while True:
            i = pred[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if tr:
        out = (row4col.astype(np.int32), col4row.astype(np.int32), v, u, 0)
    else:
        out = (col4row.astype(np.int32), row4col.astype(np.int32), u, v, 0)
    return out + (steps,) if count_steps else out


def decode(col4row, row4col, T, D):
    """assignment of the augmented (T + D, D + T) problem -> track_to_det (T,), det_to_track (D,), -1 = none"""
    c, r = np.asarray(col4row)[:T], np.asarray(row4col)[:D]
    return np.where((c >= 0) & (c < D), c, -1), np.where((r >= 0) & (r < T), r, -1)


# ---- generators shared by the fixture tool, the tests and the bench -----------------------------------------------------
def reference_case(T, D, seed, classes=4, fill=10000.0, sigma=4.0):
    """a cost matrix built the way the reference builds it: random labels in `classes` classes, logits ~ N(0, sigma^2) on
    the class-gated pairs, N(0, 1) miss / new diagonals -> (cost, logits, pairs, count, track_miss, det_new, labels)"""
    g = np.random.default_rng(seed)
    tl, dl = g.integers(0, classes, T), g.integers(0, classes, D)
    pairs, count = compare_pairs(tl, dl, num_classes=classes)
    logits = (g.standard_normal(len(pairs)) * sigma).astype(F)
    miss, new = g.standard_normal(T).astype(F), g.standard_normal(D).astype(F)
    cost = association_cost(logits, pairs, count, T, D, miss, new, fill=fill)
    return cost, logits, pairs, count, miss, new, (tl, dl)


def integer_case(R, C, high, seed):
    return np.random.default_rng(seed).integers(0, high, (R, C)).astype(F)
