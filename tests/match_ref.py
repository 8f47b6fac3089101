"""CPU restatement (numpy) of include/pcr.h section A13: the validation table a batch of pairs adds to, its flag word,
and the dicts of pcr_amd.metrics derived from a table.  Written from the header's rules, row by row; the kernels
(csrc/match_kernels.hip) must equal `table_of` / `objects_of` bit for bit, and the derived dicts must equal
pcr_amd.metrics on the same rows.

The derivation here does not share code with pcr_amd/matchbook.py: a subset's six counters are expanded back into the 0 / 1
prediction and target arrays they count, and the reference's formulas (datasets/utils.py:254-277) are applied to those
arrays in float32.

`fault=` plants one deliberate error, for the tests that show the comparison would catch it."""
import itertools

import numpy as np

CELLS, KEY_BINS, PTS_BINS = 6, 64, 32
ALL, CLS0, CLSMAX, PTS, VIS, OBJ, TABLE = 0, 6, 390, 774, 6918, 31494, 31498
INFO_NAN, INFO_GT, INFO_CLS, INFO_PTS, INFO_VIS = 1, 2, 4, 8, 16
CELL_GT = (1.0, 1.0, 0.0, 0.0, -1.0, -1.0)                  # the target and the prediction a cell counts
CELL_PRED = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)


def pts_bin(n):
    """0 for 0 points, 1 + floor(log2 n) otherwise, in integer arithmetic"""
    return int(n).bit_length()


def table_of(logit, gt, cls, num_points, vis, count=None, fault=None):
    """-> (table (TABLE,) int64, info) of ONE pcr_match_record_i64 launch over these rows on an empty table"""
    logit, gt = np.asarray(logit, np.float32), np.asarray(gt, np.float32)
    cls, num_points, vis = (np.asarray(a).reshape(-1, 2).astype(np.int64) for a in (cls, num_points, vis))
    P = logit.shape[0]
    n = P if count is None else min(max(int(count), 0), P)
    if fault == "count":
        n = P
    table, info = np.zeros(TABLE, np.int64), 0
    for i in range(n):
        g = {1.0: 0, 0.0: 1, -1.0: 2}.get(float(gt[i]), -1)
        if g < 0:
            info |= INFO_GT
            continue
        x = logit[i]
        if x != x:
            info |= INFO_NAN
        pred = 1 if x > 0 else 0
        cell = 2 * g + pred
        if fault == "swap_cells":
            cell = 3 * pred + g                              # [pred][gt] in place of [gt][pred]
        table[ALL + cell] += 1
        c0, c1 = int(cls[i, 0]), int(cls[i, 1])
        if -1 <= c0 <= 62 and -1 <= c1 <= 62:
            table[CLS0 + (c0 + 1) * CELLS + cell] += 1
            table[CLSMAX + (max(c0, c1) + 1) * CELLS + cell] += 1
        else:
            info |= INFO_CLS
        n0, n1 = int(num_points[i, 0]), int(num_points[i, 1])
        if n0 >= 0 and n1 >= 0:
            lo, hi = pts_bin(min(n0, n1)), pts_bin(max(n0, n1))
            if fault == "swap_lohi":
                lo, hi = hi, lo
            table[PTS + (PTS_BINS * lo + hi) * CELLS + cell] += 1
        else:
            info |= INFO_PTS
        v0, v1 = int(vis[i, 0]), int(vis[i, 1])
        if -1 <= v0 <= 62 and -1 <= v1 <= 62:
            table[VIS + (KEY_BINS * (min(v0, v1) + 1) + max(v0, v1) + 1) * CELLS + cell] += 1
        else:
            info |= INFO_VIS
    return table, info


def objects_of(cls_logits=None, cls_gt=None, fp_logits=None, fp_gt=None, count=None, period=None):
    """-> (the four object counters, info) of ONE pcr_match_record_objects_i64 launch"""
    M = len(cls_gt) if cls_gt is not None else len(fp_gt)
    period = M if period is None else period
    live = period if count is None else min(max(int(count), 0), period)
    out, info = np.zeros(4, np.int64), 0
    for m in range(M):
        if m % period >= live:
            continue
        if cls_logits is not None:
            row = np.asarray(cls_logits[m], np.float32)
            nan = np.nonzero(row != row)[0]
            arg = int(nan[0]) if nan.size else int(np.nonzero(row == row.max())[0][0])
            if nan.size:
                info |= INFO_NAN
            out[1] += 1
            out[0] += int(arg == int(cls_gt[m]))
        if fp_logits is not None:
            x = np.float32(fp_logits[m])
            if x != x:
                info |= INFO_NAN
            out[3] += 1
            out[2] += int((1.0 if x > 0 else 0.0) == float(fp_gt[m]))
    return out, info


# ---- a table -> the dicts of pcr_amd.metrics --------------------------------------------------------------------------------
def _arrays(n):
    """the predictions and targets six counters stand for, as float32 arrays"""
    n = [int(v) for v in n]
    return (np.repeat(np.asarray(CELL_PRED, np.float32), n), np.repeat(np.asarray(CELL_GT, np.float32), n))


def _sum(a):
    return np.float32(a.sum(dtype=np.float64))               # (0 / 1 values, fewer than 2^24 of them: the exact integer)


def f1_of(n):
    preds, targets = _arrays(n)
    eps = np.float32(1e-6)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = targets == 1
        recall_pos = _sum(preds[pos]) / (_sum(targets[pos]) + eps)
        precision_pos = _sum(preds[pos]) / (_sum(preds) + eps)
        f1_pos = np.float32(2) * (precision_pos * recall_pos) / (precision_pos + recall_pos + eps)
        neg = targets == 0
        recall_neg = _sum(1 - preds[neg]) / _sum(1 - targets[neg]) + eps
        precision_neg = _sum(1 - preds[neg]) / _sum(1 - preds) + eps
        f1_neg = np.float32(2) * (precision_neg * recall_neg) / (precision_neg + recall_neg + eps)
    return {"val_match_f1_pos": float(f1_pos), "val_match_recall_pos": float(recall_pos),
            "val_match_precision_pos": float(precision_pos), "val_match_f1_neg": float(f1_neg),
            "val_match_recall_neg": float(recall_neg), "val_match_precision_neg": float(precision_neg)}


def acc_of(n):
    preds, targets = _arrays(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(_sum(preds == targets) / np.float32(len(preds)))


def entry_of(n, nan_to_minus1=True):
    e = f1_of(n)
    e["accuracy"] = acc_of(n)
    e["num_observations_pos"] = int(n[0] + n[1])
    e["num_observations_neg"] = int(n[2] + n[3])
    if nan_to_minus1:
        e = {k: (-1 if isinstance(v, float) and v != v else v) for k, v in e.items()}
    return e


def _select(grid, keep):
    """the six counters of the cells (lo, hi) of a square grid for which keep(lo, hi) holds"""
    n = np.zeros(CELLS, np.int64)
    for lo in range(grid.shape[0]):
        for hi in range(grid.shape[1]):
            if keep(lo, hi):
                n += grid[lo, hi]
    return n


def metrics_of(table, cls_to_idx=None, num_classes=None):
    t = np.asarray(table, np.int64)
    out = {"val_match_acc": acc_of(t[ALL:ALL + CELLS])}
    out.update(f1_of(t[ALL:ALL + CELLS]))
    if cls_to_idx:
        for name, idx in cls_to_idx.items():
            n = t[CLS0 + (idx + 1) * CELLS:CLS0 + (idx + 2) * CELLS] if -1 <= idx <= 62 else np.zeros(CELLS, np.int64)
            if n.sum() > 0:
                out["val_match_acc_%s" % name] = acc_of(n)
        if num_classes is not None:
            n = sum((t[CLSMAX + (c + 1) * CELLS:CLSMAX + (c + 2) * CELLS] for c in range(max(num_classes, -1), 63)),
                    np.zeros(CELLS, np.int64))
            if n.sum() > 0:
                out["val_match_acc_FP"] = acc_of(n)
    pts = t[PTS:VIS].reshape(PTS_BINS, PTS_BINS, CELLS)
    top = max([hi for lo in range(PTS_BINS) for hi in range(PTS_BINS) if pts[lo, hi].sum() > 0], default=0)
    for i in range(top):                                     # 2^i <= the largest cloud, whose bin is top
        n = _select(pts, lambda lo, hi: lo >= i + 1)
        if n.sum() > 0:
            out["val_match_acc_both_ge_%d_pts" % 2 ** i] = acc_of(n)
    obj = t[OBJ:OBJ + 4]
    with np.errstate(invalid="ignore", divide="ignore"):
        if obj[1] > 0:
            out["val_cls_acc"] = float(np.float32(obj[0]) / np.float32(obj[1]))
        if obj[3] > 0:
            out["val_fp_acc"] = float(np.float32(obj[2]) / np.float32(obj[3]))
    return out


def tables_of(table, fault=None):
    t = np.asarray(table, np.int64)
    pts = t[PTS:VIS].reshape(PTS_BINS, PTS_BINS, CELLS)
    vis = t[VIS:OBJ].reshape(KEY_BINS, KEY_BINS, CELLS)
    out = {}
    # points: a cloud of n points sits in bin 1 + floor(log2 n); edge i = 2^i
    top = max([hi for lo in range(PTS_BINS) for hi in range(PTS_BINS) if pts[lo, hi].sum() > 0], default=0)
    nb = max(top - 1, 0)
    out["results_per_points"] = dict(
        at_least_one={(i, i + 1): entry_of(_select(pts, lambda lo, hi: hi >= i + 1)) for i in range(nb)},
        at_least_both={(i, i + 1): entry_of(_select(pts, lambda lo, hi: lo >= i + 1)) for i in range(nb)},
        for_a_pair={((i, i + 1), (j, j + 1)): entry_of(_select(pts, lambda lo, hi: (lo, hi) == (i + 1, j + 1)))
                    for i, j in itertools.combinations_with_replacement(range(nb), 2)})
    # distance: index = value + 1
    vmax = max([hi for lo in range(KEY_BINS) for hi in range(KEY_BINS) if vis[lo, hi].sum() > 0]) - 1
    edges = [5 * i for i in range(int(vmax / 5) + 3)]
    nb = len(edges) - 1
    le = (lambda v, e: v < e) if fault == "edge_lt" else (lambda v, e: v <= e)
    inb = lambda v, i: edges[i] <= v < edges[i + 1]          # noqa: E731
    out["results_per_distance"] = dict(
        at_least_one={(i, i + 1): entry_of(_select(vis, lambda lo, hi: le(lo - 1, edges[i]))) for i in range(nb)},
        at_least_both={(i, i + 1): entry_of(_select(vis, lambda lo, hi: le(hi - 1, edges[i]))) for i in range(nb)},
        for_a_pair={((i, i + 1), (j, j + 1)): entry_of(_select(vis, lambda lo, hi: inb(lo - 1, i) and inb(hi - 1, j)))
                    for i, j in itertools.combinations_with_replacement(range(nb), 2)})
    # visibility: without the pairs of target -1
    real = vis.copy()
    real[:, :, 4:] = 0
    lv = (0, 1, 2, 3)
    out["results_per_visibility"] = dict(
        at_least_one={x: entry_of(_select(real, lambda lo, hi: hi - 1 >= x), nan_to_minus1=False) for x in lv},
        at_least_both={x: entry_of(_select(real, lambda lo, hi: lo - 1 >= x), nan_to_minus1=False) for x in lv},
        for_a_pair={(x, y): entry_of(_select(real, lambda lo, hi: (lo - 1, hi - 1) == (x, y)))
                    for x, y in itertools.combinations_with_replacement(lv, 2)})
    return out


def planted_rows(P, seed=0, num_classes=10):
    """P rows with every edge the rules name: classes 0..19 (some at or above num_classes) and -1, point counts at 0, 1,
    2^k - 1, 2^k, 2^k + 1, visibility / distance values at -1, 0, 5, 10, 59 and in between, gt in {1, 0, -1}, logits on
    both sides of 0 and at least 1e-3 away from it.  -> dict(logit, gt, cls, num_points, vis) of numpy arrays"""
    g = np.random.default_rng(seed)
    logit = g.standard_normal(P).astype(np.float32)
    logit = np.where(np.abs(logit) < 1e-3, np.float32(0.5), logit).astype(np.float32)
    gt = g.choice(np.asarray([1.0, 0.0, -1.0], np.float32), size=P, p=[0.45, 0.4, 0.15]).astype(np.float32)
    cls = g.integers(0, 20, size=(P, 2))
    cls[g.random(P) < 0.05, 0] = -1
    special = [0, 1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 1023, 1024, 1025, 65535, 65536, 65537]
    num_points = g.integers(1, 3000, size=(P, 2))
    pick = g.random((P, 2)) < 0.5
    num_points[pick] = g.choice(special, size=int(pick.sum()))
    vis = g.integers(-1, 60, size=(P, 2))
    pick = g.random((P, 2)) < 0.4
    vis[pick] = g.choice([-1, 0, 5, 10, 59, 4, 6, 3, 2, 1], size=int(pick.sum()))
    return dict(logit=logit, gt=gt, cls=cls.astype(np.int64), num_points=num_points.astype(np.int64),
                vis=vis.astype(np.int64))
