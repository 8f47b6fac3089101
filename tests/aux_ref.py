"""Restatements of the auxiliary training losses (include/pcr.h section C2; ReIDNet.py:348-384, 467-482, 538-582) in the
closed forms the kernels implement: float64 torch for the values and the hand-written gradients, plain Python / numpy
for the draw rule.  tests/test_aux_ref_cpu.py holds them against torch's own KLDivLoss / TripletMarginLoss /
cross_entropy / BCE composites; tests/test_gpu_aux_losses.py holds the launches against them.

The `flip`, `eps` and `mean` arguments exist so that the CPU test can plant the three faults a port of these losses is
most likely to make and see each one detected."""
import numpy as np
import torch

EPS = 1e-6
INFO_KL_EMPTY, INFO_TRIPLET_NONE, INFO_TRIPLET_POOL = 1, 2, 4
STREAM_TRIPLET = 3
M32 = 0xFFFFFFFF


# ---- kl ----
def kl_pairs(h, match, flip=True):
    """h (2B, D) = [h1 ; h2], match (B) -> (loss, kl (B), lse (2B), cross (B), info); an empty group's mean counts as 0"""
    B, D = h.shape[0] // 2, h.shape[1]
    h1, h2 = h[:B], h[B:]
    lse = torch.logsumexp(h, dim=1)
    p2 = torch.exp(h2 - lse[B:, None])
    cross = (p2 * (h2 - h1)).sum(dim=1)
    kl = (cross - (lse[B:] - lse[:B])) / D
    m = torch.as_tensor(match).bool()
    n1 = int(m.sum())
    n0 = B - n1
    loss = h.new_zeros(())
    if n0:
        loss = loss + (-1.0 if flip else 1.0) * kl[~m].sum() / n0
    if n1:
        loss = loss + kl[m].sum() / n1
    return loss, kl, lse, cross, (0 if n0 and n1 else INFO_KL_EMPTY)


def kl_pairs_grad(h, match, g=1.0):
    """d(g * loss)/dh in closed form: w_i (p1 - p2) and w_i p2 [(h2 - h1) - cross_i], w_i = +-g / (group size * D)"""
    B, D = h.shape[0] // 2, h.shape[1]
    _, _, lse, cross, _ = kl_pairs(h, match)
    m = torch.as_tensor(match).bool()
    n1 = int(m.sum())
    n = torch.where(m, torch.tensor(float(max(n1, 1))), torch.tensor(float(max(B - n1, 1)))).to(h.dtype)
    w = torch.where(m, 1.0, -1.0).to(h.dtype) * g / (n * D)
    p = torch.exp(h - lse[:, None])
    p1, p2 = p[:B], p[B:]
    d1 = w[:, None] * (p1 - p2)
    d2 = w[:, None] * p2 * ((h[B:] - h[:B]) - cross[:, None])
    return torch.cat([d1, d2], dim=0)


# ---- cls / fp ----
def cross_entropy(logits, labels):
    """-> (mean over rows of lse - logit[label], its gradient)"""
    M = logits.shape[0]
    lse = torch.logsumexp(logits, dim=1)
    loss = (lse - logits[torch.arange(M), labels]).mean()
    grad = torch.exp(logits - lse[:, None])
    grad[torch.arange(M), labels] -= 1.0
    return loss, grad / M


def bce_logits(x, t):
    """-> (mean of max(x, 0) - x t + log1p(exp(-|x|)), its gradient)"""
    loss = (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()
    return loss, (torch.sigmoid(x) - t) / x.numel()


# ---- triplet ----
def pair_dist(a, h, eps=EPS):
    """a (B, D), h (R, D) -> || (a_i - h_r) + eps ||_2 (B, R)"""
    return ((a[:, None, :] - h[None, :, :]) + eps).pow(2).sum(dim=-1).sqrt()


def triplet(h, neg, match, margin, eps=EPS, mean="rows"):
    """h (2B, D) = [anchors ; positives], neg (B, T) integers, match (B) -> (loss with alpha = 1, dist (B, 2B), E (B, 2B),
    count, info).  A row takes part when it matches and neg[i][0] >= 0; mean: "rows" = T * the rows taking part (the
    reference's mean over all triplets), "all" = B * T (a planted fault)."""
    B = h.shape[0] // 2
    neg = np.asarray(neg)
    T = neg.shape[1]
    dist = pair_dist(h[:B], h, eps)
    E = torch.zeros_like(dist)
    total = h.new_zeros(())
    rows = [i for i in range(B) if int(match[i]) and neg[i, 0] >= 0]
    for i in rows:
        dap, k = dist[i, B + i], 0
        for t in range(T):
            r = int(neg[i, t])
            v = dap - dist[i, r] + margin
            if float(v.detach()) > 0:
                total = total + v
                k += 1
                if float(dist[i, r].detach()) > 0:
                    E[i, r] += 1.0 / dist[i, r].detach()
        if k and float(dap.detach()) > 0:
            E[i, B + i] -= k / dap.detach()
    count = len(rows) * T if mean == "rows" else B * T
    loss = total / count if count and rows else h.new_zeros(())
    return loss, dist, E, (count if rows else 0), (0 if rows else INFO_TRIPLET_NONE)


def triplet_grad(h, E, count, g=1.0, eps=EPS):
    """d(g * loss)/dh from the coefficient matrix: da_i = -g' sum_r E[i, r] diff, dh_r = +g' sum_i E[i, r] diff, g' = g / count,
    the anchors' part added into the first B rows"""
    B = h.shape[0] // 2
    if not count:
        return torch.zeros_like(h)
    diff = (h[:B, None, :] - h[None, :, :]) + eps
    w = E[:, :, None] * diff
    dh = (g / count) * w.sum(dim=0)
    dh[:B] -= (g / count) * w.sum(dim=1)
    return dh


def median_margin(h, neg, match, eps=EPS):
    """a margin under which active and inactive triplets both occur: the midpoint of the two central DISTINCT values
    of d_an - d_ap over the triplets (the median, for an even number of triplets without a repeated negative)"""
    B = h.shape[0] // 2
    dist = pair_dist(h[:B], h, eps)
    v = sorted({float(dist[i, int(r)] - dist[i, B + i]) for i in range(B) if int(match[i]) and neg[i][0] >= 0 for r in neg[i]})
    return 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def hinge_gaps(h, neg, match, margin, eps=EPS):
    """-> (the smallest |d_ap - d_an + margin| over the triplets, the largest distance): the hinge-gap condition"""
    B = h.shape[0] // 2
    dist = pair_dist(h[:B], h, eps)
    gaps = [abs(float(dist[i, B + i] - dist[i, int(r)] + margin))
            for i in range(B) if int(match[i]) and neg[i][0] >= 0 for r in neg[i]]
    return (min(gaps) if gaps else float("inf")), float(dist.max())


# ---- the draw (pcr.h: W(seed, stream, key, k), pick, the pool rule) ----
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def word(seed, stream, key, k):
    seed &= 0xFFFFFFFFFFFFFFFF
    h = mix32((seed & M32) ^ 0x9e3779b9)
    h = mix32(h ^ (seed >> 32))
    h = mix32(h ^ stream)
    h = mix32(h ^ (key & M32))
    return mix32(h ^ (k & M32))


def pick(u, n):
    return (u * n) >> 32


def pool_of(ids, i):
    return [r for r in range(len(ids)) if ids[r] != ids[i]]


def draw(ids, match, T, seed=0, rand=None):
    """ids (2B), match (B) -> (neg (B, T) int32, info): rows of non-matching pairs and of an empty pool are -1"""
    B = len(match)
    neg = np.full((B, T), -1, np.int32)
    info = 0
    for i in range(B):
        if not match[i]:
            continue
        pool = pool_of(ids, i)
        P = len(pool)
        if P == 0:
            info |= INFO_TRIPLET_POOL
            continue
        w = [(int(rand[i * T + t]) & M32) if rand is not None else word(seed, STREAM_TRIPLET, i, t) for t in range(T)]
        if P < T:
            neg[i] = [pool[pick(w[t], P)] for t in range(T)]
        else:
            for t in range(T):
                j = t + pick(w[t], P - t)
                pool[t], pool[j] = pool[j], pool[t]
                neg[i, t] = pool[t]
    return neg, info


def words_for(ids, match, neg):
    """the rand words (B T) int32 under which `draw` returns the given negatives (rows of matching pairs; entries of a
    row distinct when its pool holds at least T rows, as torch.multinomial without replacement gives them)"""
    B, T = neg.shape
    out = np.zeros(B * T, np.uint32)
    for i in range(B):
        if not match[i]:
            continue
        pool = pool_of(ids, i)
        P = len(pool)
        for t in range(T):
            j = pool.index(int(neg[i, t])) if P < T else pool.index(int(neg[i, t]), t)
            lo, n = (j, P) if P < T else (j - t, P - t)
            out[i * T + t] = -((-lo << 32) // n)                 # the smallest u with pick(u, n) == lo
            if P >= T:
                pool[t], pool[j] = pool[j], pool[t]
    return out.view(np.int32)
