"""Ranking a gallery on the device (include/pcr.h section A8, csrc/rank_kernels.hip).

`ReIDNet.match_gallery` scores any list of (i, j) combinations; its consumer so far is the tracker frame, which turns the
logits into a cost matrix and an assignment.  The other thing one does with a re-identification model is retrieval: for
every query object, which gallery objects is it, and how often does the right one come first.  Here that is three
fixed-shape launches without a host read and with the same bits on every run, so a ranked chunk of queries can be captured
in a HIP graph: `score_matrix` scatters the logits of a pair list onto -inf ("not a candidate"), `rank_gallery` ranks
every row (top-k, the first hit and the average precision against identities; ties to the lowest gallery index, the rule of
pcr_amd/nms.py), and `RankBook.add` adds a chunk's results to a table on the device.  `RankBook.metrics()` is the one host
read.  `ReIDNet.retrieve` chains compare_pairs, match_gallery and the two launches; `evaluate_retrieval` walks a split of a
`CropStore` through it.  INTEGRATION.md ("2h. Ranking a gallery") has the mapping and the rules.

A gallery above MAX_GALLERY entries takes the wide route (section A12), opt-in: `fill_scores` once, `scatter_scores` per
gallery block into the block's column window, `rank_gallery_wide` over the whole matrix (the row read from memory, not
staged in LDS); `ReIDNet.retrieve_wide` chains them and `evaluate_retrieval(gallery_block=)` walks a split through it.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import abi
from . import associate as A
from .frame import match_across

MAX_QUERIES, MAX_GALLERY, MAX_K, MAX_RANKS = 65535, 4096, 64, 8      # PCR_RANK_MAX_*
WIDE_MAX_GALLERY, WIDE_MAX_TRUE = 4194304, 4096                      # PCR_RANK_WIDE_MAX_* (section A12)
OUTPUTS = ("topk_idx", "topk_score", "n_cand", "n_true", "first_hit", "ap", "info")
_WHO = "pcr_amd.retrieval"


def rank_ok(Q, G, K=1, cap=0):
    """whether the section-A8 entry points take Q queries, G gallery entries, K ranks and a pair list of cap entries"""
    return bool(L.load().pcr_rank_ok(int(Q), int(G), int(K), int(cap)))


def score_matrix(logits, pairs, count, Q, G, out=None):
    """pcr_rank_scores_f32: logits (cap,), pairs (cap, 2) int32, count (1,) int32 on the device -> scores (Q, G) float32,
    every element written: logits[k] at pairs[k] = (q, g) for k < min(count, cap), -inf elsewhere; a pair outside
    [0, Q) x [0, G) is skipped.  The pairs must be distinct (compare_pairs' are).  out = a (Q, G) tensor to write into."""
    Q, G = int(Q), int(G)
    pairs = L.tensor(pairs, _WHO, "pairs", torch.int32, shape=(None, 2))
    cap = pairs.shape[0]
    logits = L.tensor(logits, _WHO, "logits", torch.float32, shape=(cap,))
    count = L.tensor(count, _WHO, "count", torch.int32, numel=1)
    L.require(Q >= 0 and G >= 0 and cap <= Q * G and rank_ok(Q, G, 1, cap), _WHO,
              "Q=%d G=%d cap=%d is out of range (pcr_rank_ok)", Q, G, cap)
    out = L.out_tensor(out, _WHO, "out", torch.float32, (Q, G), logits.device)
    L.require_cuda(logits, pairs, count, out)
    L.run.pcr_rank_scores_f32(logits, pairs, count, out, Q, G, cap, L.stream_ptr())
    return out


def rank_buffers(Q, K, device):
    """the seven outputs of rank_gallery for Q queries and K ranks, to be passed as out= (a captured graph keeps them)"""
    return {k: torch.empty((Q, K) if k.startswith("topk") else (Q,), dtype=abi.RankParams.ELEM[k], device=device)
            for k in OUTPUTS}


def rank_gallery(scores, query_ids, gallery_ids, topk=10, exclude=None, out=None):
    """pcr_rank_gallery_f32: scores (Q, G) float32 (-inf = not a candidate), query_ids (Q,), gallery_ids (G,) int32 (a value
    < 0, or None: no identity), exclude (Q,) int32 or None: the one gallery entry a query does not rank ->
    dict(topk_idx (Q, K) int32, topk_score (Q, K), n_cand, n_true, first_hit (Q,) int32, ap (Q,) float32, info (Q,) int32),
    every element written by the rules of include/pcr.h section A8: descending score, ties to the lowest gallery index;
    info 1 = a candidate's score is a NaN, the query is not ranked.  With None ids only topk_* and n_cand are meaningful.
    out = such a dict (`rank_buffers`) to write into."""
    scores = L.tensor(scores, _WHO, "scores", torch.float32, shape=(None, None))
    (Q, G), K = scores.shape, int(topk)
    L.require(rank_ok(Q, G, K), _WHO, "Q=%d G=%d topk=%d is out of range (pcr_rank_ok)", Q, G, K)
    dev = scores.device
    if query_ids is None:
        query_ids = torch.full((Q,), -1, dtype=torch.int32, device=dev)
    if gallery_ids is None:
        gallery_ids = torch.full((G,), -1, dtype=torch.int32, device=dev)
    if out is None:
        out = rank_buffers(Q, K, dev)
    L.require(isinstance(out, dict) and all(k in out for k in OUTPUTS), _WHO, "out must hold %s", ", ".join(OUTPUTS))
    sizes = dict(scores=Q * G, query_ids=Q, gallery_ids=G, exclude=Q, topk_idx=Q * K, topk_score=Q * K, n_cand=Q, n_true=Q,
                 first_hit=Q, ap=Q, info=Q)
    p = abi.RankParams()
    p.Q, p.G, p.K = Q, G, K
    abi.fill(p, dict({k: out[k] for k in OUTPUTS}, scores=scores, query_ids=query_ids, gallery_ids=gallery_ids,
                     exclude=exclude), sizes, who=_WHO)
    L.run.pcr_rank_gallery_f32(ctypes.byref(p), L.stream_ptr())
    return {k: out[k] for k in OUTPUTS}


def rank_wide_ok(Q, G, K=1):
    """whether the section-A12 entry points take Q queries, G gallery entries (up to WIDE_MAX_GALLERY) and K ranks"""
    return bool(L.load().pcr_rank_wide_ok(int(Q), int(G), int(K)))


def fill_scores(scores):
    """pcr_rank_fill_f32: every element of scores (Q, G) float32 becomes -inf ("not a candidate"); -> scores"""
    scores = L.tensor(scores, _WHO, "scores", torch.float32, shape=(None, None))
    Q, G = scores.shape
    L.require(rank_wide_ok(Q, G), _WHO, "Q=%d G=%d is out of range (pcr_rank_wide_ok)", Q, G)
    L.require_cuda(scores)
    L.run.pcr_rank_fill_f32(scores, Q, G, L.stream_ptr())
    return scores


def scatter_scores(logits, pairs, count, scores, col0, width):
    """pcr_rank_scatter_f32: the scatter of `score_matrix` into the column window [col0, col0 + width) of scores (Q, G):
    logits (cap,), pairs (cap, 2) int32 with the gallery index counted from col0, count (1,) int32 on the device;
    scores[q, col0 + g] = logits[k] for k < min(count, cap) and pairs[k] = (q, g) inside [0, Q) x [0, width); every other
    element is left as it is (`fill_scores` first).  The pairs must be distinct.  -> scores"""
    scores = L.tensor(scores, _WHO, "scores", torch.float32, shape=(None, None))
    (Q, G), col0, width = scores.shape, int(col0), int(width)
    pairs = L.tensor(pairs, _WHO, "pairs", torch.int32, shape=(None, 2))
    cap = pairs.shape[0]
    logits = L.tensor(logits, _WHO, "logits", torch.float32, shape=(cap,))
    count = L.tensor(count, _WHO, "count", torch.int32, numel=1)
    L.require(rank_wide_ok(Q, G) and col0 >= 0 and width >= 0 and col0 + width <= G and cap <= Q * width, _WHO,
              "Q=%d G=%d cap=%d col0=%d width=%d is out of range (pcr_rank_scatter_f32)", Q, G, cap, col0, width)
    L.require_cuda(logits, pairs, count, scores)
    L.run.pcr_rank_scatter_f32(logits, pairs, count, scores, Q, G, cap, col0, width, L.stream_ptr())
    return scores


def rank_gallery_wide(scores, query_ids, gallery_ids, topk=10, exclude=None, out=None):
    """pcr_rank_wide_f32: `rank_gallery` for a gallery of up to WIDE_MAX_GALLERY entries -- the same arguments, the same
    dict, the same rules and, for G <= MAX_GALLERY, the same bits; the row is read from memory (twice at the most) instead
    of staged in LDS.  One rule more: a query with more than WIDE_MAX_TRUE true candidates is not ranked and gets info 2
    (its outputs are a flagged query's; a NaN candidate, info 1, takes precedence)."""
    scores = L.tensor(scores, _WHO, "scores", torch.float32, shape=(None, None))
    (Q, G), K = scores.shape, int(topk)
    L.require(rank_wide_ok(Q, G, K), _WHO, "Q=%d G=%d topk=%d is out of range (pcr_rank_wide_ok)", Q, G, K)
    dev = scores.device
    if query_ids is None:
        query_ids = torch.full((Q,), -1, dtype=torch.int32, device=dev)
    if gallery_ids is None:
        gallery_ids = torch.full((G,), -1, dtype=torch.int32, device=dev)
    if out is None:
        out = rank_buffers(Q, K, dev)
    L.require(isinstance(out, dict) and all(k in out for k in OUTPUTS), _WHO, "out must hold %s", ", ".join(OUTPUTS))
    sizes = dict(scores=Q * G, query_ids=Q, gallery_ids=G, exclude=Q, topk_idx=Q * K, topk_score=Q * K, n_cand=Q, n_true=Q,
                 first_hit=Q, ap=Q, info=Q)
    p = abi.RankParams()
    p.Q, p.G, p.K = Q, G, K
    abi.fill(p, dict({k: out[k] for k in OUTPUTS}, scores=scores, query_ids=query_ids, gallery_ids=gallery_ids,
                     exclude=exclude), sizes, who=_WHO)
    L.run.pcr_rank_wide_f32(ctypes.byref(p), L.stream_ptr())
    return {k: out[k] for k in OUTPUTS}


def metrics_of(counts, sums, ranks):
    """the table on the host (counts: 3 + len(ranks) ints, sums: 2 floats) -> cmc@r per rank, mAP, mrr (NaN when no query
    was scored) and the raw counters scored (a true candidate exists), unscored (none does), flagged (a NaN)"""
    c = [int(v) for v in counts]
    scored = c[0]
    out = {"cmc@%d" % r: (c[3 + i] / scored if scored else float("nan")) for i, r in enumerate(ranks)}
    out["mAP"] = float(sums[0]) / scored if scored else float("nan")
    out["mrr"] = float(sums[1]) / scored if scored else float("nan")
    out["scored"], out["unscored"], out["flagged"] = c[0], c[1], c[2]
    return out


class RankBook:
    """The retrieval table of an evaluation, on the device: `counts` (3 + len(ranks),) int32 = scored, unscored, flagged
    queries and, per rank r, the scored queries whose first hit lies below r; `sums` (2,) float64 = the running sums of the
    average precision and of 1 / (first_hit + 1) over the scored queries, in the order they were added.  `add` is one launch
    on the current stream without a host read; `metrics` is the host read.  One book per class gives per-class figures, as
    for `TruthBook`."""

    def __init__(self, ranks=(1, 5, 10), device="cuda"):
        self.ranks = tuple(int(r) for r in ranks)
        L.require(len(self.ranks) <= MAX_RANKS and all(1 <= r <= MAX_GALLERY for r in self.ranks), _WHO,
                  "ranks must be at most %d values in [1, %d]", MAX_RANKS, MAX_GALLERY)
        self.device = torch.device(device)
        self.counts = torch.zeros(3 + len(self.ranks), dtype=torch.int32, device=self.device)
        self.sums = torch.zeros(2, dtype=torch.float64, device=self.device)

    def reset(self):
        self.counts.zero_()
        self.sums.zero_()

    def add(self, result, valid=None, gallery=None):
        """pcr_rank_accumulate: result = rank_gallery's (or retrieve's) dict; valid = a (1,) int32 device tensor (or an
        int): only the first clamp(valid, 0, Q) queries count (the rest is a chunk's padding); gallery = the number of
        gallery entries G the ranks are held against (every rank must lie in [1, G]); by default the width of
        result['scores'] when retrieve returned it, the largest rank otherwise.  The launch uses G only to bound the
        ranks, and a book's ranks are at most MAX_GALLERY already: for a wide gallery (rank_gallery_wide, retrieve_wide)
        pass gallery=min(G, MAX_GALLERY), as evaluate_retrieval does."""
        t = {k: result[k] for k in ("n_true", "first_hit", "info", "ap")}
        if isinstance(valid, int):
            valid = torch.tensor([valid], dtype=torch.int32, device=self.device)
        L.require(isinstance(t["n_true"], torch.Tensor) and t["n_true"].dim() == 1, _WHO, "n_true must be a (Q,) tensor")
        Q = t["n_true"].shape[0]
        if gallery is None:
            gallery = result["scores"].shape[1] if "scores" in result else max(self.ranks, default=0)
        G = int(gallery)
        L.require(rank_ok(Q, G) and all(r <= G for r in self.ranks), _WHO,
                  "Q=%d G=%d ranks=%s: out of range (pcr_rank_ok), or a rank above the gallery", Q, G, self.ranks)
        sizes = dict(n_true=Q, first_hit=Q, info=Q, ap=Q, valid=1, counts=3 + len(self.ranks), sums=2)
        p = abi.RankAccParams()
        p.Q, p.G, p.nranks = Q, G, len(self.ranks)
        for i, r in enumerate(self.ranks):
            p.ranks[i] = r
        abi.fill(p, dict(t, valid=valid, counts=self.counts, sums=self.sums), sizes, required=t, who=_WHO)
        L.run.pcr_rank_accumulate(ctypes.byref(p), L.stream_ptr())

    def metrics(self):
        """THE host read: see `metrics_of`"""
        return metrics_of(self.counts.cpu().tolist(), self.sums.cpu().tolist(), self.ranks)


def retrieval_split(table, row_of, seed=0):
    """One query and one gallery observation per true object of an `ObjectTable`, distractors from everything else, on the
    host -> (query_rows, gallery_rows, query_cls, gallery_cls, query_ids, gallery_ids), int32 arrays.

    For object index i of table.true_index, ascending, with obs = its `nums`: a, b = np.random.default_rng([seed, i]).
    choice(len(obs), 2, replace=False); the query is row_of[(token, obs[a])], its partner in the gallery
    row_of[(token, obs[b])], both with id i.  Every other object of a tracked class with at least one observation (the
    false positives, the tracks too short to be queries) gives a distractor: the observation
    obs[np.random.default_rng([seed, i]).integers(len(obs))] in the gallery with id -1.  The gallery is in object order."""
    true = set(table.true_index)
    q_rows, q_cls, q_ids, g_rows, g_cls, g_ids = [], [], [], [], [], []
    for i, o in enumerate(table.objects):
        obs = o["nums"]
        rng = np.random.default_rng([int(seed), i])
        if i in true:
            a, b = rng.choice(len(obs), 2, replace=False)
            q_rows.append(row_of[(o["token"], obs[a])])
            q_cls.append(o["cls"])
            q_ids.append(i)
            g_rows.append(row_of[(o["token"], obs[b])])
            g_cls.append(o["cls"])
            g_ids.append(i)
        elif o["cls"] != -1 and len(obs) > 0:
            g_rows.append(row_of[(o["token"], obs[int(rng.integers(len(obs)))])])
            g_cls.append(o["cls"])
            g_ids.append(-1)
    i32 = lambda a: np.asarray(a, dtype=np.int32)          # noqa: E731
    return i32(q_rows), i32(g_rows), i32(q_cls), i32(g_cls), i32(q_ids), i32(g_ids)


def retrieve(model, q_feats, q_xyz, q_labels, q_lengths, g_feats, g_xyz, g_labels, g_lengths, query_ids, gallery_ids, topk,
             exclude, min_points, num_classes, live_only):
    """ReIDNet.retrieve, which has the contract and the defaults"""
    L.require_cuda(q_feats, q_xyz, g_feats, g_xyz)
    Q, G = q_feats.shape[0], g_feats.shape[0]
    if not rank_ok(Q, G, topk):
        raise L.PcrError("retrieve: Q=%d G=%d topk=%d is out of range (pcr_rank_ok)%s" % (
            Q, G, topk, "; retrieve_wide ranks a gallery above %d entries" % MAX_GALLERY if G > MAX_GALLERY else ""))
    pairs, count = A.compare_pairs(q_labels, g_labels, q_lengths, g_lengths, min_points=min_points,
                                   num_classes=num_classes)
    if Q == 0 or G == 0:
        logits = torch.empty((pairs.shape[0],), dtype=torch.float32, device=q_feats.device)
    else:
        logits = match_across(model, torch.cat([q_feats, g_feats], dim=0), torch.cat([q_xyz, g_xyz], dim=0),
                              pairs, Q, count if live_only else None)                      # the gallery follows the queries
    scores = score_matrix(logits, pairs, count, Q, G)
    out = rank_gallery(scores, query_ids, gallery_ids, topk=topk, exclude=exclude)
    return dict(pairs=pairs, count=count, logits=logits, scores=scores, **out)


def retrieve_wide(model, q_feats, q_xyz, q_labels, q_lengths, g_feats, g_xyz, g_labels, g_lengths, query_ids, gallery_ids,
                  topk, exclude, min_points, num_classes, live_only, gallery_block, scores):
    """ReIDNet.retrieve_wide, which has the contract and the defaults"""
    L.require_cuda(q_feats, q_xyz, g_feats, g_xyz)
    Q, G, block = q_feats.shape[0], g_feats.shape[0], int(gallery_block)
    if not 1 <= block <= MAX_GALLERY:
        raise L.PcrError("retrieve_wide: gallery_block=%d: 1 to %d" % (block, MAX_GALLERY))
    if not rank_wide_ok(Q, G, topk):
        raise L.PcrError("retrieve_wide: Q=%d G=%d topk=%d is out of range (pcr_rank_wide_ok)" % (Q, G, topk))
    dev = q_feats.device
    scores = fill_scores(L.out_tensor(scores, "retrieve_wide", "scores", torch.float32, (Q, G), dev))
    counts = []
    g_labels = L.tensor(g_labels, "retrieve_wide", "g_labels", torch.int32, shape=(G,), cast_int64=True, copy=True)
    g_lengths = L.tensor(g_lengths, "retrieve_wide", "g_lengths", torch.int32, shape=(G,), optional=True, cast_int64=True,
                         copy=True)
    for lo in range(0, G, block):
        hi = min(G, lo + block)
        pairs, count = A.compare_pairs(q_labels, g_labels[lo:hi], q_lengths, None if g_lengths is None else g_lengths[lo:hi],
                                       min_points=min_points, num_classes=num_classes)
        counts.append(count)
        if Q == 0:
            continue
        logits = match_across(model, torch.cat([q_feats, g_feats[lo:hi]], dim=0), torch.cat([q_xyz, g_xyz[lo:hi]], dim=0),
                              pairs, Q, count if live_only else None)                      # the block follows the queries
        scatter_scores(logits, pairs, count, scores, lo, hi - lo)
    out = rank_gallery_wide(scores, query_ids, gallery_ids, topk=topk, exclude=exclude)
    counts = torch.cat(counts) if counts else torch.zeros((0,), dtype=torch.int32, device=dev)
    return dict(scores=scores, counts=counts, **out)


def _encode(model, clouds, batch):
    """forward_inference over clouds (B, n, 3) in batches -> xyz (B, N, 3), feats (B, C, N)"""
    xyz, feats = [], []
    cm = model.use_dgcnn or type(model.backbone).__name__ == "PointNet"
    for lo in range(0, clouds.shape[0], batch):
        c = clouds[lo:lo + batch]
        x, h = model.forward_inference(c.permute(0, 2, 1).contiguous() if cm else c)[:2]
        xyz.append(x)
        feats.append(h)
    return torch.cat(xyz, dim=0).contiguous(), torch.cat(feats, dim=0).contiguous()


def evaluate_retrieval(model, store, split, n=None, seed=0, topk=10, ranks=(1, 5, 10), query_chunk=64, min_points=2,
                       num_classes=None, live_only=True, encode_batch=256, gallery_block=None):
    """Retrieval over a `CropStore`: split = retrieval_split's six arrays.  The clouds come from store.gather(rows, n,
    keys=rows, seed=seed) (a row's sample depends on the row and the seed alone), the gallery is encoded once, the queries
    walk through `ReIDNet.retrieve` in chunks of query_chunk -- the last one padded with class -1, which joins nothing, the
    real count going to the book as `valid` -- and each chunk is added to a `RankBook`.  -> book.metrics() (the one host
    read) plus the per-query tensors of rank_gallery, (Q, ...) on the device, and the book itself under 'book'.
    num_classes defaults to the store's table's.

    gallery_block = an integer in [1, MAX_GALLERY] takes the wide route: a gallery of up to WIDE_MAX_GALLERY entries, every
    chunk through `ReIDNet.retrieve_wide` in gallery blocks of that many entries, one (query_chunk, G) score buffer reused
    by all chunks, the book's ranks held against min(G, MAX_GALLERY).  None is the narrow route, G <= MAX_GALLERY."""
    q_rows, g_rows, q_cls, g_cls, q_ids, g_ids = (np.asarray(a, dtype=np.int32) for a in split)
    Q, G, chunk = len(q_rows), len(g_rows), int(query_chunk)
    wide = gallery_block is not None
    if wide:
        L.require(1 <= int(gallery_block) <= MAX_GALLERY, _WHO, "gallery_block=%s: 1 to %d", gallery_block, MAX_GALLERY)
        L.require(1 <= G <= WIDE_MAX_GALLERY, _WHO, "a gallery of %d entries: 1 to PCR_RANK_WIDE_MAX_GALLERY = %d can be ranked",
                  G, WIDE_MAX_GALLERY)
        L.require(chunk >= 1 and rank_wide_ok(chunk, G, topk), _WHO,
                  "query_chunk=%d G=%d topk=%d is out of range (pcr_rank_wide_ok)", chunk, G, topk)
    else:
        L.require(1 <= G <= MAX_GALLERY, _WHO, "a gallery of %d entries: 1 to PCR_RANK_MAX_GALLERY = %d can be ranked; "
                  "gallery_block= takes the wide route (up to %d entries)", G, MAX_GALLERY, WIDE_MAX_GALLERY)
        L.require(chunk >= 1 and rank_ok(chunk, G, topk), _WHO, "query_chunk=%d G=%d topk=%d is out of range (pcr_rank_ok)", chunk, G, topk)
    L.require(len(q_cls) == Q and len(q_ids) == Q and len(g_cls) == G and len(g_ids) == G, _WHO, "the split's arrays do not agree")
    if num_classes is None:
        num_classes = int(store.table.num_classes) if getattr(store, "table", None) is not None else 8
    n = int(n or store.n)
    dev = store.device
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)      # noqa: E731
    book = RankBook(ranks, dev)
    per_query = {k: [] for k in OUTPUTS}
    with torch.no_grad():
        g_rows_t, g_cls_t, g_ids_t = put(g_rows), put(g_cls), put(g_ids)
        g_clouds, g_sizes = store.gather(g_rows_t, n, keys=g_rows_t, seed=seed)
        g_xyz, g_feats = _encode(model, g_clouds, encode_batch)
        wide_scores = torch.empty((chunk, G), dtype=torch.float32, device=dev) if wide else None
        for lo in range(0, Q, chunk):
            real = min(chunk, Q - lo)
            pad = lambda a, fill: np.concatenate([a[lo:lo + real], np.full(chunk - real, fill, np.int32)])   # noqa: E731
            rows_t, cls_t, ids_t = put(pad(q_rows, 0)), put(pad(q_cls, -1)), put(pad(q_ids, -1))
            clouds, sizes = store.gather(rows_t, n, keys=rows_t, seed=seed)
            xyz, feats = _encode(model, clouds, encode_batch)
            if wide:
                res = model.retrieve_wide(feats, xyz, cls_t, sizes, g_feats, g_xyz, g_cls_t, g_sizes, query_ids=ids_t,
                                          gallery_ids=g_ids_t, topk=topk, min_points=min_points, num_classes=num_classes,
                                          live_only=live_only, gallery_block=int(gallery_block), scores=wide_scores)
            else:
                res = model.retrieve(feats, xyz, cls_t, sizes, g_feats, g_xyz, g_cls_t, g_sizes, query_ids=ids_t,
                                     gallery_ids=g_ids_t, topk=topk, min_points=min_points, num_classes=num_classes,
                                     live_only=live_only)
            book.add(res, valid=torch.tensor([real], dtype=torch.int32, device=dev), gallery=min(G, MAX_GALLERY))
            for k in OUTPUTS:
                per_query[k].append(res[k][:real])
    out = book.metrics()
    empty = rank_buffers(0, int(topk), dev)
    out.update({k: torch.cat(v, dim=0) if v else empty[k] for k, v in per_query.items()})
    out["book"] = book
    return out
