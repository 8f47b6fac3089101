"""numpy restatement of the block rule (include/pcr.h section A3, "The block rule"): what the tests compare
pcr_assoc_blocks_i32 / pcr_lsa_blocks_f32 against, bit for bit.

block_ids restates the id mapping (an object's label in [0, num_classes), the rest block num_classes otherwise; decision rows
and columns take their object's block), lsa_blocks the rule itself: gather the block's rows and columns in ascending
original index -> assoc_ref.lsa -> scatter as original indices.
"""
import numpy as np

import assoc_ref

F = np.float32


def block_ids(track_labels, det_labels, T, D, de, te, num_classes=8):
    """-> row_block (T + de*D,), col_block (D + te*T,) int32, G = num_classes + 1"""
    tl, dl = np.asarray(track_labels).astype(np.int64).reshape(T), np.asarray(det_labels).astype(np.int64).reshape(D)
    tb = np.where((tl >= 0) & (tl < num_classes), tl, num_classes).astype(np.int32)
    db = np.where((dl >= 0) & (dl < num_classes), dl, num_classes).astype(np.int32)
    return np.concatenate([tb] + [db] * de), np.concatenate([db] + [tb] * te), num_classes + 1


def lsa_blocks(cost, row_block, col_block, G, count_steps=False):
    """cost (R, C) -> col4row (R,), row4col (C,) int32, u (R,), v (C,) f32, info (G,) int32 [, search steps per block]"""
    cost = np.asarray(cost, F)
    R, C = cost.shape
    rb, cb = np.asarray(row_block).reshape(R), np.asarray(col_block).reshape(C)
    col4row, row4col = np.full(R, -1, np.int32), np.full(C, -1, np.int32)
    u, v, info, steps = np.zeros(R, F), np.zeros(C, F), np.zeros(G, np.int32), np.zeros(G, np.int64)
    for g in range(G):
        rows, cols = np.flatnonzero(rb == g), np.flatnonzero(cb == g)
        if not len(rows) or not len(cols):
            continue
        c4r, r4c, ug, vg, info[g], steps[g] = assoc_ref.lsa(cost[np.ix_(rows, cols)], count_steps=True)
        if info[g]:
            continue
        col4row[rows] = np.where(c4r >= 0, cols[np.maximum(c4r, 0)], -1)
        row4col[cols] = np.where(r4c >= 0, rows[np.maximum(r4c, 0)], -1)
        u[rows], v[cols] = ug, vg
    out = (col4row, row4col, u, v, info)
    return out + (steps,) if count_steps else out
