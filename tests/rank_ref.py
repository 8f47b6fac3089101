"""CPU restatement of include/pcr.h section A8 (ranking a gallery), in numpy and plain Python: an explicit rank by
counting, the average precision in Python floats (binary64) in the written order with one cast at the end.  The kernels of
csrc/rank_kernels.hip equal it bit for bit (tests/test_gpu_rank.py); tests/test_rank_cpu.py holds it against an independent
check (np.lexsort, fractions.Fraction)."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def score_matrix(logits, pairs, count, Q, G):
    """logits (cap,), pairs (cap, 2), count -> scores (Q, G): logits[k] at pairs[k] for k < min(count, cap) inside the
    range, -inf elsewhere"""
    logits = np.asarray(logits, np.float32)
    scores = np.full((Q, G), NEG_INF, np.float32)
    n = min(max(int(count), 0), len(logits))
    for k in range(n):
        q, g = int(pairs[k][0]), int(pairs[k][1])
        if 0 <= q < Q and 0 <= g < G:
            scores[q, g] = logits[k]
    return scores


def rank_query(row, qid, gallery_ids, K, exclude=-1):
    """one query by the rules -> (topk_idx (K,), topk_score (K,), n_cand, n_true, first_hit, ap (np.float32), info)"""
    row = np.asarray(row, np.float32)
    G = len(row)
    ex = exclude if 0 <= exclude < G else -1
    cand = [g for g in range(G) if g != ex and not row[g] == NEG_INF]
    topk_idx, topk_score = np.full(K, -1, np.int32), np.full(K, NEG_INF, np.float32)
    if any(np.isnan(row[g]) for g in cand):
        return topk_idx, topk_score, 0, 0, -1, np.float32(0.0), 1
    ci = np.asarray(cand, np.int64)
    cs = row[ci]                                            # (the float compare: -0 == +0)
    rank = {g: int(np.count_nonzero((cs > row[g]) | ((cs == row[g]) & (ci < g)))) for g in cand}
    for g in cand:
        if rank[g] < K:
            topk_idx[rank[g]], topk_score[rank[g]] = g, row[g]
    true = sorted(rank[g] for g in cand if qid >= 0 and int(gallery_ids[g]) == qid)
    total = 0.0
    for i, r in enumerate(true):
        total = total + float(i + 1) / float(r + 1)
    ap = np.float32(total / float(len(true))) if true else np.float32(0.0)
    return topk_idx, topk_score, len(cand), len(true), (true[0] if true else -1), ap, 0


def rank_gallery(scores, query_ids, gallery_ids, K, exclude=None):
    """scores (Q, G) -> dict of the seven outputs"""
    scores = np.asarray(scores, np.float32)
    Q, G = scores.shape
    out = dict(topk_idx=np.full((Q, K), -1, np.int32), topk_score=np.full((Q, K), NEG_INF, np.float32),
               n_cand=np.zeros(Q, np.int32), n_true=np.zeros(Q, np.int32), first_hit=np.full(Q, -1, np.int32),
               ap=np.zeros(Q, np.float32), info=np.zeros(Q, np.int32))
    for q in range(Q):
        qid = int(query_ids[q]) if query_ids is not None else -1
        gids = gallery_ids if gallery_ids is not None else np.full(G, -1, np.int32)
        r = rank_query(scores[q], qid, gids, K, int(exclude[q]) if exclude is not None else -1)
        for k, v in zip(("topk_idx", "topk_score", "n_cand", "n_true", "first_hit", "ap", "info"), r):
            out[k][q] = v
    return out


def accumulate(counts, sums, result, ranks, valid=None):
    """the table after one more chunk: counts (3 + len(ranks)) ints and sums [sum ap, sum 1 / (first_hit + 1)] Python floats,
    the running sums continued in ascending q -> (counts, sums), new lists"""
    counts, sums = [int(c) for c in counts], [float(s) for s in sums]
    Q = len(result["info"])
    n = Q if valid is None else min(max(int(valid), 0), Q)
    for q in range(n):
        if int(result["info"][q]) != 0:
            counts[2] += 1
        elif int(result["n_true"][q]) > 0:
            counts[0] += 1
            fh = int(result["first_hit"][q])
            for i, r in enumerate(ranks):
                counts[3 + i] += int(fh < r)
            sums[0] = sums[0] + float(np.float32(result["ap"][q]))
            sums[1] = sums[1] + 1.0 / float(fh + 1)
        else:
            counts[1] += 1
    return counts, sums


def bits(a):
    """float arrays as their bit patterns, for exact comparison (a NaN equals itself, -0 differs from +0)"""
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
