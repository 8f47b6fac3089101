"""numpy restatement of association with any set of decisions (include/pcr.h section A3, "Any set of decisions"): what the
tests compare pcr_assoc_cost_multi_f32 / pcr_assoc_decode_i32 against.

cost_multi restates get_cost_mat_margin / get_cost_mat_softmax (trackers/deprecated/tracking_association.py:22-98) and
TrackingAssociatorMax.get_cost_mat_margin (:319-363); decode restates :146-245 with pcr.h's two deliberate differences
(a void assignment is dropped and counted instead of ending the process; the repair picks one object after the other).
The margin matrix is float32 operation by operation (bit for bit the kernel's); the softmax matrix is float64 throughout
and rounded to float32 once (the kernel is compared with a tolerance).  The assignment comes from assoc_ref.lsa.
"""
import numpy as np

F = np.float32


def shape(T, D, dd, td, reduce=False):
    de, te = (int(dd > 0), int(td > 0)) if reduce else (dd, td)
    return T + de * D, D + te * T


def _dec(values, k, n):
    return np.zeros((k, n), F) if values is None else np.asarray(values, F).reshape(k, n)


def cost_multi(logits, pairs, count, T, D, det_dec=None, trk_dec=None, dd=None, td=None, kind="margin", reduce=False,
               dist=None, dist_max=22.0, dist_penalty=3.0, fill=10000.0):
    """-> cost (R, C) float32 [, det_choice (D,), trk_choice (T,) under reduce]"""
    dd = (0 if det_dec is None else len(det_dec)) if dd is None else dd
    td = (0 if trk_dec is None else len(trk_dec)) if td is None else td
    det_dec, trk_dec = _dec(det_dec, dd, D), _dec(trk_dec, td, T)
    assert kind in ("margin", "softmax") and not (kind == "softmax" and (reduce or dist is not None))
    k = min(int(count), len(pairs))
    t, d = np.asarray(pairs)[:k, 0].astype(np.int64), np.asarray(pairs)[:k, 1].astype(np.int64)
    ok = (t >= 0) & (t < T) & (d >= 0) & (d < D)
    t, d, lg = t[ok], d[ok], np.asarray(logits, F)[:k][ok]
    det_choice, trk_choice = np.zeros(D, np.int32), np.zeros(T, np.int32)
    if kind == "margin":
        val = -lg
        if dist is not None:
            far = np.asarray(dist, F)[t, d] > F(dist_max)
            val = np.where(far, val + F(dist_penalty), val).astype(F)
        if reduce:                       # np.argmin: the first (lowest-index) minimum
            if dd:
                det_choice = np.argmin(det_dec, axis=0).astype(np.int32)
                det_dec = det_dec[det_choice, np.arange(D)][None]
            if td:
                trk_choice = np.argmin(trk_dec, axis=0).astype(np.int32)
                trk_dec = trk_dec[trk_choice, np.arange(T)][None]
        det_val, trk_val = det_dec, trk_dec
    else:
        score = np.full((T, D), -np.inf)
        score[t, d] = lg.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):    # (an object with an empty set: 0 / 0, never read)
            rows = np.concatenate([score, trk_dec.T.astype(np.float64)], axis=1)            # (T, D + td)
            cols = np.concatenate([score, det_dec.astype(np.float64)], axis=0)              # (T + dd, D)
            rmax = rows.max(axis=1, keepdims=True) if rows.shape[1] else np.zeros((T, 1))
            cmax = cols.max(axis=0, keepdims=True) if cols.shape[0] else np.zeros((1, D))
            er, ec = np.exp(rows - rmax), np.exp(cols - cmax)
            er[np.isneginf(rows)], ec[np.isneginf(cols)] = 0.0, 0.0
            p_row, p_col = er / er.sum(axis=1, keepdims=True), ec / ec.sum(axis=0, keepdims=True)
        val = (-np.maximum(p_row[t, d], p_col[t, d])).astype(F)
        det_val, trk_val = (-p_col[T:]).astype(F), (-p_row[:, D:].T).astype(F)
    de, te = len(det_val), len(trk_val)
    R, C = T + de * D, D + te * T
    cost = np.full((R, C), F(fill), F)
    cost[t, d] = val
    for i in range(de):
        for j in range(te):
            cost[T + i * D + d, D + j * T + t] = val
    for i in range(de):
        cost[T + i * D + np.arange(D), np.arange(D)] = det_val[i]
    for j in range(te):
        cost[np.arange(T), D + j * T + np.arange(T)] = trk_val[j]
    return (cost, det_choice, trk_choice) if reduce else cost


def _argmin(values, free):
    """the free index of least value, lowest index on ties; -1 if none is free"""
    idx = np.flatnonzero(free)
    return int(idx[np.argmin(values[idx])]) if len(idx) else -1


def decode(cost, col4row, row4col, T, D, dd, td, fill=10000.0, choices=None, born_dec=-1, kill_dec=-1, solver_info=0):
    """-> dict of track_to_det (T,), det_to_track (D,), det_decision (D,), track_decision (T,), born (D,), kill (T,),
    info (4,), all int32"""
    reduce = choices is not None
    R, C = shape(T, D, dd, td, reduce)
    te = td > 0
    cost = np.asarray(cost, F).reshape(R, C)
    info = np.zeros(4, np.int32)
    info[0] = solver_info
    c4r, r4c = np.full(R, -1, np.int64), np.full(C, -1, np.int64)
    if not solver_info:
        for r in range(R):
            c = int(np.asarray(col4row).reshape(-1)[r])
            if not 0 <= c < C:
                continue
            if cost[r, c] == F(fill):
                info[1] += 1
                continue
            if te and r >= T and c >= D:
                continue
            c4r[r], r4c[c] = c, r
        if te:
            for t in range(T):
                if c4r[t] >= 0:
                    continue
                c = _argmin(cost[t], r4c < 0)
                if c < 0 or cost[t, c] == F(fill):
                    continue
                c4r[t], r4c[c] = c, t
                info[2] += 1
            for d in range(D):
                if r4c[d] >= 0:
                    continue
                r = _argmin(cost[:, d], c4r < 0)
                if r < 0 or cost[r, d] == F(fill):
                    continue
                c4r[r], r4c[d] = d, r
                info[3] += 1
    t2d, d2t = np.full(T, -1, np.int32), np.full(D, -1, np.int32)
    tdec, ddec = np.full(T, 1 + td, np.int32), np.full(D, 1 + dd, np.int32)
    for t in range(T):
        c = c4r[t]
        if 0 <= c < D:
            t2d[t], tdec[t] = c, 0
        elif c >= D:
            tdec[t] = 1 + (choices[1][t] if reduce else (c - D) // T)
    for d in range(D):
        r = r4c[d]
        if 0 <= r < T:
            d2t[d], ddec[d] = r, 0
        elif r >= T:
            ddec[d] = 1 + (choices[0][d] if reduce else (r - T) // D)
    born = (ddec == 1 + born_dec).astype(np.int32) if born_dec >= 0 else np.zeros(D, np.int32)
    kill = (tdec == 1 + kill_dec).astype(np.int32) if kill_dec >= 0 else np.zeros(T, np.int32)
    return dict(track_to_det=t2d, det_to_track=d2t, det_decision=ddec, track_decision=tdec, born=born, kill=kill, info=info)


def decision_lists(out, det_names, trk_names):
    """decode's arrays as the reference's dict of index lists (sorted ascending), for comparison with the golden"""
    lists = {"det_match": np.flatnonzero(out["det_decision"] == 0), "track_match": np.flatnonzero(out["track_decision"] == 0)}
    for i, k in enumerate(det_names):
        lists[k] = np.flatnonzero(out["det_decision"] == 1 + i)
    for j, k in enumerate(trk_names):
        lists[k] = np.flatnonzero(out["track_decision"] == 1 + j)
    lists["det_unmatched"] = np.flatnonzero(out["det_decision"] == 1 + len(det_names))
    lists["track_unmatched"] = np.flatnonzero(out["track_decision"] == 1 + len(trk_names))
    return lists


# ---- generator shared by the tests and the bench -------------------------------------------------------------------------
def random_case(T, D, dd, td, seed, classes=3, sigma=4.0, dense=False):
    """random labels in `classes` classes (dense: one class), logits ~ N(0, sigma^2) on the class-gated pairs, N(0, 1) decision
    values -> (logits, pairs, count, det_dec (dd, D), trk_dec (td, T))"""
    import assoc_ref
    g = np.random.default_rng(seed)
    classes = 1 if dense else classes
    tl, dl = g.integers(0, classes, T), g.integers(0, classes, D)
    pairs, count = assoc_ref.compare_pairs(tl, dl, num_classes=classes)
    logits = (g.standard_normal(len(pairs)) * sigma).astype(F)
    return logits, pairs, count, g.standard_normal((dd, D)).astype(F), g.standard_normal((td, T)).astype(F)
