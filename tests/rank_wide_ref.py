"""CPU restatement of include/pcr.h section A12 (ranking a wide gallery): section A8's rules over rows of any width.  The
order comes from one np.lexsort per row, O(G log G) -- tests/rank_ref.py counts every rank, O(G^2), which a row of 40000
entries does not allow -- the average precision is in Python floats (binary64) in the written order with one cast at the end,
as there; `max_true` is the added rule (info 2); `fill` / `scatter` are the score matrix by column windows.
tests/test_rank_wide_cpu.py holds it against rank_ref.rank_gallery bit for bit."""
import numpy as np

NEG_INF = np.float32(-np.inf)
MAX_TRUE = 4096                                             # PCR_RANK_WIDE_MAX_TRUE


def fill(Q, G):
    """scores (Q, G), every element -inf"""
    return np.full((Q, G), NEG_INF, np.float32)


def scatter(scores, logits, pairs, count, col0, width):
    """logits[k] at scores[q, col0 + g] for k < min(max(count, 0), cap) with pairs[k] = (q, g) inside [0, Q) x [0, width);
    every other element as it is; in place -> scores"""
    logits = np.asarray(logits, np.float32)
    Q, G = scores.shape
    assert 0 <= col0 and 0 <= width and col0 + width <= G
    for k in range(min(max(int(count), 0), len(logits))):
        q, g = int(pairs[k][0]), int(pairs[k][1])
        if 0 <= q < Q and 0 <= g < width:
            scores[q, col0 + g] = logits[k]
    return scores


def rank_query(row, qid, gallery_ids, K, exclude=-1, max_true=MAX_TRUE):
    """one query by the rules -> (topk_idx (K,), topk_score (K,), n_cand, n_true, first_hit, ap (np.float32), info)"""
    row = np.asarray(row, np.float32)
    G = len(row)
    keep = row != NEG_INF                                   # (true for a NaN)
    if 0 <= exclude < G:
        keep[exclude] = False
    cand = np.flatnonzero(keep)
    topk_idx, topk_score = np.full(K, -1, np.int32), np.full(K, NEG_INF, np.float32)
    flagged = (topk_idx, topk_score, 0, 0, -1, np.float32(0.0))
    if np.isnan(row[cand]).any():
        return flagged + (1,)
    hit = np.asarray(gallery_ids)[cand] == qid if qid >= 0 else np.zeros(len(cand), bool)
    if int(hit.sum()) > max_true:
        return flagged + (2,)
    order = np.lexsort((cand, -(row[cand].astype(np.float64) + 0.0)))      # -0 + 0 = +0: the float compare's equality
    k = min(K, len(cand))
    topk_idx[:k], topk_score[:k] = cand[order[:k]], row[cand[order[:k]]]
    true = np.flatnonzero(hit[order])                       # the true candidates' ranks, ascending
    total = 0.0
    for i, r in enumerate(true.tolist()):
        total = total + float(i + 1) / float(r + 1)
    ap = np.float32(total / float(len(true))) if len(true) else np.float32(0.0)
    return topk_idx, topk_score, len(cand), len(true), (int(true[0]) if len(true) else -1), ap, 0


def rank_gallery(scores, query_ids, gallery_ids, K, exclude=None, max_true=MAX_TRUE):
    """scores (Q, G) -> dict of the seven outputs"""
    scores = np.asarray(scores, np.float32)
    Q, G = scores.shape
    out = dict(topk_idx=np.full((Q, K), -1, np.int32), topk_score=np.full((Q, K), NEG_INF, np.float32),
               n_cand=np.zeros(Q, np.int32), n_true=np.zeros(Q, np.int32), first_hit=np.full(Q, -1, np.int32),
               ap=np.zeros(Q, np.float32), info=np.zeros(Q, np.int32))
    gids = gallery_ids if gallery_ids is not None else np.full(G, -1, np.int32)
    for q in range(Q):
        qid = int(query_ids[q]) if query_ids is not None else -1
        r = rank_query(scores[q], qid, gids, K, int(exclude[q]) if exclude is not None else -1, max_true)
        for k, v in zip(("topk_idx", "topk_score", "n_cand", "n_true", "first_hit", "ap", "info"), r):
            out[k][q] = v
    return out
