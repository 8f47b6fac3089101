"""GPU: ranking a gallery (include/pcr.h section A8, pcr_amd/retrieval.py).  Every comparison is exact: == on integers and
on float bits, against the numpy restatement tests/rank_ref.py.
  * pcr_rank_gallery_f32 on random scores with planted structure: G at 1, around the 64-lane chunk (63, 64, 65), over
    several chunks (130) and at the limit (4096); Q of 1, 3 and 70; K of 1, 10 and 64, above and below the candidates;
  * the rules one by one: equal scores across a chunk boundary, -0 against +0, an empty row, a NaN among the candidates
    and one at an excluded slot, the best candidate excluded, 0 / 1 / 5 true candidates in different chunks, no identity,
    +inf scores, Q == 0 and G == 0;
  * score_matrix at every kind of count; RankBook over chunks, with `valid`; the same bits twice; one captured graph that
    follows the count and the logits; the refusals;
  * end to end on the toy Point-Transformer (128 points): retrieve against the restatement over its own logits,
    evaluate_retrieval whatever the query chunk, live_only against the full list."""
import numpy as np
import pytest
import torch

import rank_ref as R
from pcr_amd import _lib as L
from pcr_amd import retrieval as RT
from pcr_amd import testing as T

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(result):
    return {k: result[k].cpu().numpy() for k in RT.OUTPUTS}


def assert_same(got, want, what=""):
    for k in RT.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (what, k)


def run(scores, qids, gids, K, exclude=None, out=None):
    return RT.rank_gallery(dev(scores), None if qids is None else dev(qids), None if gids is None else dev(gids), topk=K,
                           exclude=None if exclude is None else dev(exclude), out=out)


def check(scores, qids, gids, K, exclude=None, what=""):
    got = host(run(scores, qids, gids, K, exclude))
    want = R.rank_gallery(scores, qids, gids, K, exclude)
    assert_same(got, want, what)
    return got


def planted(Q, G, seed):
    """random scores with many ties (a few values, both zeros, +inf), holes of -inf, ids from a small set so that a query
    has several true candidates spread over the row, some queries without an identity, exclusions in and out of range"""
    g = np.random.default_rng(seed)
    values = np.array([-np.inf, -np.inf, -2.5, -0.0, 0.0, 0.5, 0.5, 1.25, np.inf], np.float32)
    coarse = values[g.integers(0, len(values), (Q, G))]
    scores = np.where(g.random((Q, G)) < 0.4, coarse, g.standard_normal((Q, G)).astype(np.float32))
    gids = g.integers(-1, 5, G).astype(np.int32)
    qids = g.integers(-1, 5, Q).astype(np.int32)
    exclude = g.integers(-2, G + 2, Q).astype(np.int32)
    return scores, qids, gids, exclude


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (3, 1, 10), (3, 63, 10), (1, 63, 64), (70, 64, 1), (3, 64, 64), (3, 65, 10), (70, 65, 64), (70, 130, 10),
          (1, 130, 1), (3, 130, 64), (3, 4096, 10), (1, 4096, 64), (1, 4096, 1)]


@pytest.mark.parametrize("Q,G,K", SHAPES)
def test_kernel_equals_the_restatement(Q, G, K):
    scores, qids, gids, exclude = planted(Q, G, 1000 * G + 10 * Q + K)
    got = check(scores, qids, gids, K, exclude, (Q, G, K))
    assert not got["info"].any()
    if G >= 63:
        assert (got["n_cand"] > 0).all()
    if G >= 130 and Q >= 3:
        assert (got["n_true"] > 1).any()
    check(scores, qids, gids, K, None, (Q, G, K, "no exclusion"))


def test_the_rules_one_by_one():
    G, K = 200, 10
    g = np.random.default_rng(7)
    base = g.standard_normal(G).astype(np.float32)
    gids = np.full(G, -1, np.int32)
    gids[[5, 70, 71, 140, 199]] = 9                           # five entries of identity 9, in four chunks
    gids[100] = 4
    rows, qids, excl, names = [], [], [], []

    def add(name, row, qid, ex=-1):
        names.append(name), rows.append(row.astype(np.float32)), qids.append(qid), excl.append(ex)
    tie = base.copy()
    tie[[62, 63, 64, 65, 128]] = 30.0                         # the best score five times, across two chunk boundaries
    add("ties across a chunk boundary", tie, 9)
    zeros = np.full(G, NEG)
    zeros[[10, 63, 64, 150]] = [0.0, -0.0, 0.0, -0.0]
    zeros[20] = -1.0
    add("-0 against +0", zeros, -1)
    add("an empty row", np.full(G, NEG), 9)
    nan = base.copy()
    nan[77] = np.nan
    add("a NaN among the candidates", nan, 9)
    add("a NaN at the excluded slot", nan, 9, 77)
    best = base.copy()
    best[140] = 50.0
    add("the best candidate excluded", best, 9, 140)
    add("the best candidate kept", best, 9)
    add("no true candidate", base, 3)
    add("one true candidate", base, 4)
    add("five true candidates", base, 9)
    add("no identity", base, -1)
    inf = base.copy()
    inf[[3, 199]] = np.inf
    inf[70] = -np.inf
    add("+inf scores", inf, 9)
    few = np.full(G, NEG)
    few[[199, 5, 64]] = [1.0, 1.0, 2.0]
    add("fewer candidates than K", few, 9)
    scores, qids, excl = np.stack(rows), np.asarray(qids, np.int32), np.asarray(excl, np.int32)
    got = check(scores, qids, gids, K, excl)
    row = {n: i for i, n in enumerate(names)}
    # the restatement agrees; now what the rules say, spelled out
    assert got["topk_idx"][row["ties across a chunk boundary"], :5].tolist() == [62, 63, 64, 65, 128]
    z = row["-0 against +0"]
    assert got["topk_idx"][z, :6].tolist() == [10, 63, 64, 150, 20, -1] and got["n_cand"][z] == 5
    assert np.array_equal(R.bits(got["topk_score"][z, :4]), R.bits(np.array([0.0, -0.0, 0.0, -0.0], np.float32)))
    e = row["an empty row"]
    assert (got["topk_idx"][e] == -1).all() and (got["topk_score"][e] == NEG).all()
    assert (got["n_cand"][e], got["n_true"][e], got["first_hit"][e], got["ap"][e], got["info"][e]) == (0, 0, -1, 0, 0)
    n = row["a NaN among the candidates"]
    assert got["info"][n] == 1 and (got["topk_idx"][n] == -1).all() and got["n_cand"][n] == 0 and got["first_hit"][n] == -1
    n = row["a NaN at the excluded slot"]
    assert got["info"][n] == 0 and got["n_cand"][n] == G - 1 and got["n_true"][n] == 5          # it is ranked
    assert got["topk_idx"][row["the best candidate kept"], 0] == 140 and got["first_hit"][row["the best candidate kept"]] == 0
    b = row["the best candidate excluded"]
    assert 140 not in got["topk_idx"][b] and got["n_true"][b] == 4 and got["n_cand"][b] == G - 1
    assert [int(got["n_true"][row[k]]) for k in ("no true candidate", "one true candidate", "five true candidates",
                                                  "no identity")] == [0, 1, 5, 0]
    assert got["first_hit"][row["no identity"]] == -1 and got["ap"][row["no true candidate"]] == 0
    i = row["+inf scores"]
    assert got["topk_idx"][i, :2].tolist() == [3, 199] and got["n_true"][i] == 4 and got["first_hit"][i] == 1
    f = row["fewer candidates than K"]
    assert got["topk_idx"][f].tolist() == [64, 5, 199] + [-1] * 7 and got["n_true"][f] == 2 and got["first_hit"][f] == 1
    assert got["ap"][f] == np.float32((1.0 / 2.0 + 2.0 / 3.0) / 2.0)
    # first_hit is exact whatever K is
    one = check(scores, qids, gids, 1, excl)
    assert np.array_equal(one["first_hit"], got["first_hit"]) and np.array_equal(R.bits(one["ap"]), R.bits(got["ap"]))
    # None ids: nothing is true
    none = host(run(scores, None, None, K, excl))
    assert np.array_equal(none["topk_idx"], got["topk_idx"]) and not none["n_true"].any() and (none["first_hit"] == -1).all()


def test_empty_sides():
    got = host(run(np.zeros((0, 5), np.float32), np.zeros(0, np.int32), np.zeros(5, np.int32), 3))
    assert got["topk_idx"].shape == (0, 3) and got["ap"].shape == (0,)
    out = RT.rank_buffers(4, 3, "cuda")
    for t in out.values():
        t.fill_(77)
    got = host(run(np.zeros((4, 0), np.float32), np.arange(4, dtype=np.int32), np.zeros(0, np.int32), 3, out=out))
    assert_same(got, R.rank_gallery(np.zeros((4, 0), np.float32), np.arange(4), np.zeros(0, np.int32), 3))
    assert (got["topk_idx"] == -1).all() and (got["first_hit"] == -1).all() and not got["n_cand"].any()


def test_same_bits_on_two_runs_and_into_given_buffers():
    scores, qids, gids, exclude = planted(70, 130, 5)
    out = RT.rank_buffers(70, 10, "cuda")
    for t in out.values():
        t.fill_(-123)                                           # every element is written
    a = run(scores, qids, gids, 10, exclude, out=out)
    assert all(a[k] is out[k] for k in RT.OUTPUTS)
    a = host(a)
    assert_same(a, host(run(scores, qids, gids, 10, exclude)))
    assert_same(a, R.rank_gallery(scores, qids, gids, 10, exclude))


# ---- 2. the score matrix -----------------------------------------------------------------------------------------------------
def test_score_matrix_at_every_kind_of_count():
    Q, G = 5, 9
    g = np.random.default_rng(3)
    cap = 30
    cells = g.permutation(Q * G)[:cap]
    pairs = np.stack([cells // G, cells % G], axis=1).astype(np.int32)
    pairs[4], pairs[11], pairs[17], pairs[20] = (Q, 0), (0, G), (-1, 2), (1, -1)            # out of range: skipped
    logits = g.standard_normal(cap).astype(np.float32)
    for count in (0, 13, cap, cap + 7, -2):
        out = torch.full((Q, G), 123.0, device="cuda")
        got = RT.score_matrix(dev(logits), dev(pairs), dev(np.array([count], np.int32)), Q, G, out=out)
        assert got is out
        want = R.score_matrix(logits, pairs, count, Q, G)
        assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(want)), count
        assert np.isneginf(want).sum() == Q * G - (min(max(count, 0), cap) - sum(k < count for k in (4, 11, 17, 20)))
    assert RT.score_matrix(dev(logits[:0]), dev(pairs[:0]), dev(np.zeros(1, np.int32)), 0, G).shape == (0, G)
    empty = RT.score_matrix(dev(logits[:0]), dev(pairs[:0]), dev(np.zeros(1, np.int32)), Q, G)
    assert bool(torch.isneginf(empty).all())


# ---- 3. the book -------------------------------------------------------------------------------------------------------------
def test_rank_book_over_chunks():
    G, K, ranks = 130, 10, (1, 5, 10)
    scores, qids, gids, exclude = planted(70, G, 11)
    scores[3, 17] = np.nan                                      # flagged (17 is a candidate: not the excluded slot)
    exclude[3] = -1
    qids[5] = -1                                                # unscored
    res = run(scores, qids, gids, K, exclude)
    want = R.rank_gallery(scores, qids, gids, K, exclude)
    book = RT.RankBook(ranks, "cuda")
    first = {k: res[k][:31].contiguous() for k in RT.OUTPUTS}
    second = {k: res[k][31:].contiguous() for k in RT.OUTPUTS}
    book.add(first, gallery=G)
    book.add(second, gallery=G)
    counts, sums = R.accumulate([0] * 6, [0.0, 0.0], want, ranks)
    assert book.counts.cpu().tolist() == counts and counts[2] >= 1 and counts[1] >= 1 and counts[0] > 10
    assert np.array_equal(R.bits(book.sums.cpu().numpy()), R.bits(np.array(sums, np.float64)))
    m = book.metrics()
    assert (m["scored"], m["unscored"], m["flagged"]) == tuple(counts[:3])
    assert m["mAP"] == sums[0] / counts[0] and m["mrr"] == sums[1] / counts[0] and m["cmc@5"] == counts[4] / counts[0]
    assert 0 < m["cmc@1"] <= m["cmc@5"] <= m["cmc@10"] <= 1
    # valid below Q, as a device word and as an int; on top of the table as it stands
    book.add(res, valid=dev(np.array([20], np.int32)), gallery=G)
    counts, sums = R.accumulate(counts, sums, want, ranks, valid=20)
    book.add(res, valid=0, gallery=G)
    book.add(res, valid=1000, gallery=G)
    counts, sums = R.accumulate(counts, sums, want, ranks, valid=1000)
    assert book.counts.cpu().tolist() == counts
    assert np.array_equal(R.bits(book.sums.cpu().numpy()), R.bits(np.array(sums, np.float64)))
    book.reset()
    assert not book.counts.any() and not book.sums.any() and np.isnan(book.metrics()["mAP"])
    with pytest.raises(L.PcrError):
        book.add(res, gallery=9)                                # rank 10 against a gallery of 9


# ---- 4. a captured graph -----------------------------------------------------------------------------------------------------
def test_one_graph_follows_the_count_and_the_logits():
    Q, G, K, ranks = 6, 70, 10, (1, 5)
    g = np.random.default_rng(21)
    cap = Q * G
    cells = g.permutation(cap)
    pairs = np.stack([cells // G, cells % G], axis=1).astype(np.int32)
    qids, gids = g.integers(0, 4, Q).astype(np.int32), g.integers(0, 4, G).astype(np.int32)
    logits, count = torch.zeros(cap, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    pairs_d, qids_d, gids_d, valid = dev(pairs), dev(qids), dev(gids), dev(np.array([Q - 1], np.int32))
    scores, out, book = torch.empty((Q, G), device="cuda"), RT.rank_buffers(Q, K, "cuda"), RT.RankBook(ranks, "cuda")

    def step():
        RT.score_matrix(logits, pairs_d, count, Q, G, out=scores)
        res = RT.rank_gallery(scores, qids_d, gids_d, topk=K, out=out)
        book.add(res, valid=valid, gallery=G)
    step()                                                      # eager once: nothing is loaded inside the capture
    torch.cuda.synchronize()
    book.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    counts, sums = [0] * 5, [0.0, 0.0]
    for c, seed in ((cap, 1), (37, 2), (0, 3), (200, 4)):
        new = np.random.default_rng(seed).standard_normal(cap).astype(np.float32)
        logits.copy_(dev(new))
        count.fill_(c)
        graph.replay()
        torch.cuda.synchronize()
        want = R.rank_gallery(R.score_matrix(new, pairs, c, Q, G), qids, gids, K)
        assert_same(host(out), want, c)
        counts, sums = R.accumulate(counts, sums, want, ranks, valid=Q - 1)
        assert book.counts.cpu().tolist() == counts, c
        assert np.array_equal(R.bits(book.sums.cpu().numpy()), R.bits(np.array(sums, np.float64))), c
    assert counts[0] > 0 and counts[1] > 0


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")      # noqa: E731
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(1, 4097, device="cuda"), i32(1), i32(4097))
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8, device="cuda"), i32(2), i32(8), topk=65)
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8, device="cuda"), i32(2), i32(8), topk=0)
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8), i32(2), i32(8))                                       # a host tensor
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8, device="cuda"), i32(2).long(), i32(8))                 # int64 ids
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8, device="cuda"), i32(2), i32(8).long())
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8, device="cuda", dtype=torch.float64), i32(2), i32(8))
    with pytest.raises(L.PcrError):
        RT.rank_gallery(torch.zeros(2, 8, device="cuda"), i32(3), i32(8))                        # a wrong shape
    with pytest.raises(L.PcrError):
        RT.score_matrix(torch.zeros(20, device="cuda"), torch.zeros(20, 2, dtype=torch.int32, device="cuda"), i32(1), 2, 8)
    with pytest.raises(L.PcrError):
        RT.score_matrix(torch.zeros(4, device="cuda"), torch.zeros(4, 2, dtype=torch.int64, device="cuda"), i32(1), 2, 8)


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
N = 128
NOBJ, NOBS, NDIS = 12, 3, 3


@pytest.fixture(scope="module")
def toy():
    """the toy Point-Transformer of the other GPU tests (n = 128, seeded weights), calibrated once, over a CropStore of 12
    objects of two classes with 3 observations each plus 3 distractors (two false positives, one track too short)"""
    import bench
    from pcr_amd import store as ST
    from pcr_amd.pairs import ObjectTable
    model, _ = bench.build_pt_model([N, 64, 32])
    shapes = T.synthetic_clouds(NOBJ + NDIS, 160, seed=41, kind="box").numpy()
    g = np.random.default_rng(8)
    objs, arrays, keys = [], [], []
    for i in range(NOBJ + NDIS):
        dis = i >= NOBJ
        tok = ("dis_%02d" if dis else "obj_%02d") % i
        nobs = NOBS if not dis else (2 if i == NOBJ else 1)
        frames = {}
        for obs in range(nobs):
            npts = int(g.integers(90, 161))
            cloud = shapes[i][g.permutation(160)[:npts]] + 0.01 * g.standard_normal((npts, 3)).astype(np.float32)
            arrays.append(cloud.astype(np.float32))
            keys.append((tok, obs))
            frames[obs] = npts
        objs.append(dict(token=tok, cls=i % 2, frames=frames, fp=dis and i > NOBJ))
    table = ObjectTable(objs, num_classes=2)
    store = ST.CropStore.from_arrays(arrays, keys=keys, device="cuda", table=table, pair_rule=False)
    split = RT.retrieval_split(table, store.row_of, seed=2)
    assert len(split[0]) == NOBJ and len(split[1]) == NOBJ + NDIS
    with torch.no_grad():
        warm = T.synthetic_clouds(8, N, seed=31, kind="box").cuda()
        model.calibrate_precision(warm[:4], warm[4:])
    return model, store, split


def encoded(model, store, rows):
    rows = dev(np.asarray(rows, np.int32))
    clouds, sizes = store.gather(rows, N, keys=rows, seed=0)
    with torch.no_grad():
        xyz, feats = model.forward_inference(clouds)[:2]
    return xyz.contiguous(), feats.contiguous(), sizes


def test_retrieve_equals_the_restatement_over_its_own_logits(toy):
    model, store, (q_rows, g_rows, q_cls, g_cls, q_ids, g_ids) = toy
    q_xyz, q_feats, q_len = encoded(model, store, q_rows)
    g_xyz, g_feats, g_len = encoded(model, store, g_rows)
    Q, G, K = len(q_rows), len(g_rows), 5
    outs = []
    for live_only in (False, True):
        with torch.no_grad():
            res = model.retrieve(q_feats, q_xyz, dev(q_cls), q_len, g_feats, g_xyz, dev(g_cls), g_len, query_ids=dev(q_ids),
                                 gallery_ids=dev(g_ids), topk=K, num_classes=2, live_only=live_only)
        assert sorted(res) == sorted(RT.OUTPUTS + ("pairs", "count", "logits", "scores"))
        logits, pairs, count = res["logits"].cpu().numpy(), res["pairs"].cpu().numpy(), int(res["count"][0])
        assert pairs.shape == (Q * G, 2) and 0 < count < Q * G and not np.isnan(logits[:count]).any()
        scores = R.score_matrix(logits, pairs, count, Q, G)
        assert np.array_equal(R.bits(res["scores"].cpu().numpy()), R.bits(scores))
        want = R.rank_gallery(scores, q_ids, g_ids, K)
        assert_same(host(res), want, live_only)
        # a query's candidates are the gallery entries of its class, its partner among them
        assert want["n_cand"].tolist() == [int((g_cls == c).sum()) for c in q_cls] and (want["n_true"] == 1).all()
        outs.append(res)
    full, live = outs
    count = int(full["count"][0])
    for k in full:                                              # live_only changes logits[count:] and nothing else
        a, b = full[k].cpu().numpy(), live[k].cpu().numpy()
        if k == "logits":
            assert np.array_equal(R.bits(a[:count]), R.bits(b[:count])) and (b[count:] == 0).all()
        else:
            assert np.array_equal(R.bits(a), R.bits(b)), k
    # without identities only the order remains
    with torch.no_grad():
        bare = model.retrieve(q_feats, q_xyz, dev(q_cls), q_len, g_feats, g_xyz, dev(g_cls), g_len, topk=K, num_classes=2)
    assert torch.equal(bare["topk_idx"], full["topk_idx"]) and not bool(bare["n_true"].any())


def test_evaluate_retrieval_does_not_depend_on_the_query_chunk(toy):
    model, store, split = toy
    runs = [RT.evaluate_retrieval(model, store, split, n=N, seed=0, topk=5, ranks=(1, 5), query_chunk=c, live_only=lo)
            for c, lo in ((64, True), (5, True), (5, False))]
    ref = runs[0]
    assert ref["scored"] == NOBJ and ref["unscored"] == 0 and ref["flagged"] == 0
    assert 0 <= ref["cmc@1"] <= ref["cmc@5"] <= 1 and 0 < ref["mAP"] <= 1
    assert abs(ref["mAP"] - ref["mrr"]) < 1e-6                  # one true candidate each: ap is 1 / (rank + 1), in binary32
    assert ref["topk_idx"].shape == (NOBJ, 5) and ref["ap"].shape == (NOBJ,)
    for other in runs[1:]:
        for k in RT.OUTPUTS:
            assert np.array_equal(R.bits(ref[k].cpu().numpy()), R.bits(other[k].cpu().numpy())), k
        assert torch.equal(ref["book"].counts, other["book"].counts) and torch.equal(ref["book"].sums, other["book"].sums)
        assert all(ref[k] == other[k] for k in ("cmc@1", "cmc@5", "mAP", "mrr", "scored", "unscored", "flagged"))
    big = tuple(np.concatenate([a] * 400) for a in split[1::2])
    with pytest.raises(L.PcrError):                             # a gallery of 6000 entries
        RT.evaluate_retrieval(model, store, (split[0], big[0], split[2], big[1], split[4], big[2]), n=N)
