"""GPU: ranking a wide gallery (include/pcr.h section A12, pcr_amd/retrieval.py, ReIDNet.retrieve_wide).  Every comparison is
exact: == on integers and on float bits.
  * pcr_rank_wide_f32 equals pcr_rank_gallery_f32 on the shapes tests/test_gpu_rank.py lists, NaN rows included;
  * above 4096 entries it equals the restatement tests/rank_wide_ref.py: G of 4097, 8191, 12289 and 40000 (several steps of
    the sweep and a ragged tail whatever the step is), ties from a small value set across every boundary; planted orders at
    G = 12289 (ascending: every step displaces the whole carried top-k; descending; constant; empty; K candidates far apart;
    the last column as the true one, the excluded one, the NaN); the true-set cap (4096 ranked, 4097 flagged with info 2);
  * fill_scores + scatter_scores by column windows; one captured graph of fill, two scatters, the ranking and the book;
  * retrieve_wide on the toy Point-Transformer equals retrieve whatever the gallery block; evaluate_retrieval(gallery_block=)
    over the 6000-entry gallery the narrow route refuses; the refusals."""
import numpy as np
import pytest
import torch

import rank_ref as R
import rank_wide_ref as W
from pcr_amd import _lib as L
from pcr_amd import retrieval as RT
from test_gpu_rank import N, NOBJ, SHAPES, assert_same, dev, encoded, host, planted, toy      # noqa: F401 (toy: a fixture)

pytestmark = pytest.mark.gpu

NEG = np.float32(-np.inf)


def run_wide(scores, qids, gids, K, exclude=None, out=None):
    return RT.rank_gallery_wide(dev(scores), None if qids is None else dev(qids), None if gids is None else dev(gids), topk=K,
                                exclude=None if exclude is None else dev(exclude), out=out)


def run_narrow(scores, qids, gids, K, exclude=None):
    return RT.rank_gallery(dev(scores), None if qids is None else dev(qids), None if gids is None else dev(gids), topk=K,
                           exclude=None if exclude is None else dev(exclude))


def check(scores, qids, gids, K, exclude=None, what=""):
    got = host(run_wide(scores, qids, gids, K, exclude))
    assert_same(got, W.rank_gallery(scores, qids, gids, K, exclude), what)
    return got


# ---- 1. wide equals narrow ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,G,K", SHAPES)
def test_wide_equals_narrow(Q, G, K):
    scores, qids, gids, exclude = planted(Q, G, 1000 * G + 10 * Q + K)
    assert_same(host(run_wide(scores, qids, gids, K, exclude)), host(run_narrow(scores, qids, gids, K, exclude)), (Q, G, K))
    assert_same(host(run_wide(scores, qids, gids, K)), host(run_narrow(scores, qids, gids, K)), (Q, G, K, "no exclusion"))
    assert_same(host(run_wide(scores, None, None, K, exclude)), host(run_narrow(scores, None, None, K, exclude)), "no ids")
    if Q >= 3 and G >= 63:
        scores[0, G // 2], scores[1, G - 1] = np.nan, np.nan    # a NaN candidate; a NaN at the excluded slot
        exclude[0], exclude[1] = -1, G - 1
        wide = host(run_wide(scores, qids, gids, K, exclude))
        assert_same(wide, host(run_narrow(scores, qids, gids, K, exclude)), (Q, G, K, "NaN"))
        assert wide["info"][0] == 1 and wide["info"][1] == 0 and wide["n_cand"][1] > 0 and not wide["info"][2:].any()


def test_empty_sides_and_given_buffers():
    got = host(run_wide(np.zeros((0, 5), np.float32), np.zeros(0, np.int32), np.zeros(5, np.int32), 3))
    assert got["topk_idx"].shape == (0, 3) and got["ap"].shape == (0,)
    out = RT.rank_buffers(4, 3, "cuda")
    for t in out.values():
        t.fill_(77)                                             # every element is written
    res = run_wide(np.zeros((4, 0), np.float32), np.arange(4, dtype=np.int32), np.zeros(0, np.int32), 3, out=out)
    assert all(res[k] is out[k] for k in RT.OUTPUTS)
    got = host(res)
    assert_same(got, W.rank_gallery(np.zeros((4, 0), np.float32), np.arange(4), np.zeros(0, np.int32), 3))
    assert (got["topk_idx"] == -1).all() and (got["first_hit"] == -1).all() and not got["n_cand"].any()


# ---- 2. above the cap, against the restatement ---------------------------------------------------------------------------------
def wide_rows(Q, G, seed, ids=6):
    """half the scores from a small value set (ties across every boundary, both zeros, +inf, -inf holes), ids in [-1, ids)"""
    g = np.random.default_rng(seed)
    values = np.array([-np.inf, -2.5, -0.0, 0.0, 0.5, 0.5, 1.25, 7.0, np.inf], np.float32)
    scores = np.where(g.random((Q, G)) < 0.5, values[g.integers(0, len(values), (Q, G))],
                      g.standard_normal((Q, G)).astype(np.float32))
    gids = g.integers(-1, ids, G).astype(np.int32)
    qids = g.integers(-1, ids, Q).astype(np.int32)
    exclude = g.integers(-2, G + 2, Q).astype(np.int32)
    return scores, qids, gids, exclude


@pytest.mark.parametrize("G", [4097, 8191, 12289, 40000])
@pytest.mark.parametrize("Q,K", [(1, 1), (3, 10), (70, 64), (3, 64)])
def test_above_the_cap_equals_the_restatement(Q, K, G):
    scores, qids, gids, exclude = wide_rows(Q, G, 7 * G + 10 * Q + K)
    qids[0] = 2                                                 # (at least the first query has an identity)
    got = check(scores, qids, gids, K, exclude, (Q, G, K))
    # ids in [-1, 6): a seventh of the row is true -- ranked up to G = 12289, above the true-set cap at G = 40000
    assert got["info"][0] == (2 if G == 40000 else 0) and (got["info"][qids < 0] == 0).all()
    if G < 40000:
        assert got["n_true"][0] > G // 10 and (got["n_cand"] > G // 2).all()
    else:                                                       # the same rows with rarer identities: every query is ranked
        gids = np.random.default_rng(G + Q).integers(-1, 60, G).astype(np.int32)
        got = check(scores, qids, gids, K, exclude, (Q, G, K, "ids in [-1, 60)"))
        assert not got["info"].any() and 0 < got["n_true"][0] <= RT.WIDE_MAX_TRUE
    check(scores, qids, gids, K, None, (Q, G, K, "no exclusion"))


def test_same_bits_on_two_runs():
    scores, qids, gids, exclude = wide_rows(5, 12289, 77)
    a, b = host(run_wide(scores, qids, gids, 10, exclude)), host(run_wide(scores, qids, gids, 10, exclude))
    assert_same(a, b)


# ---- 3. planted orders ----------------------------------------------------------------------------------------------------------
def test_planted_orders():
    G, K = 12289, 10
    g = np.random.default_rng(12)
    base = g.standard_normal(G).astype(np.float32)
    gids = np.full(G, -1, np.int32)
    gids[[5, 5000, 9000]] = 9
    gids[G - 1] = 4
    gids[7000] = 3
    rows, qids, excl, names = [], [], [], []

    def add(name, row, qid, ex=-1):
        names.append(name), rows.append(np.asarray(row, np.float32)), qids.append(qid), excl.append(ex)
    ramp = np.arange(G, dtype=np.float32) / 8
    add("ascending", ramp, 9)                                   # every step displaces the whole carried top-k
    add("descending", -ramp, 9)
    add("constant", np.full(G, 0.5), 9)                         # order by index alone
    add("empty", np.full(G, NEG), 9)
    spread = np.full(G, NEG)
    spread[np.arange(K) * 1200 + 700] = g.standard_normal(K)
    add("exactly K candidates", spread, 9)
    few = np.full(G, NEG)
    few[[G - 1, 5, 6000]] = [1.0, 1.0, 2.0]
    add("K above n_cand", few, 9)
    add("the only true candidate in the last column", base, 4)
    add("exclude on the last column", base, 4, G - 1)           # ... which is the only true candidate: n_true 0
    add("exclude on the only true candidate", base, 3, 7000)
    top = base.copy()
    top[[3, G - 1]] = np.inf
    top[[10, 4095, 4096, 8192]] = [0.0, -0.0, 0.0, -0.0]
    top[(top > 0) & np.isfinite(top)] *= -1                     # +inf twice, then the four zeros, then negatives
    add("+inf and both zeros among the winners", top, 9)
    nan = base.copy()
    nan[G - 1] = np.nan
    add("a NaN in the last column", nan, 9)
    add("a NaN at the excluded last column", nan, 9, G - 1)
    scores, qids, excl = np.stack(rows), np.asarray(qids, np.int32), np.asarray(excl, np.int32)
    got = check(scores, qids, gids, K, excl)
    row = {n: i for i, n in enumerate(names)}
    # the restatement agrees; now what the rules say, spelled out
    a = row["ascending"]
    assert got["topk_idx"][a].tolist() == list(range(G - 1, G - 1 - K, -1)) and got["n_true"][a] == 3
    assert got["first_hit"][a] == G - 1 - 9000
    d = row["descending"]
    assert got["topk_idx"][d].tolist() == list(range(K)) and got["first_hit"][d] == 5
    assert got["ap"][d] == np.float32((1.0 / 6.0 + 2.0 / 5001.0 + 3.0 / 9001.0) / 3.0)
    c = row["constant"]
    assert got["topk_idx"][c].tolist() == list(range(K)) and got["first_hit"][c] == 5 and got["n_cand"][c] == G
    e = row["empty"]
    assert (got["topk_idx"][e] == -1).all() and (got["n_cand"][e], got["n_true"][e], got["first_hit"][e], got["info"][e]) == (0, 0, -1, 0)
    s = row["exactly K candidates"]
    assert got["n_cand"][s] == K and sorted(got["topk_idx"][s].tolist()) == (np.arange(K) * 1200 + 700).tolist()
    f = row["K above n_cand"]
    assert got["topk_idx"][f].tolist() == [6000, 5, G - 1] + [-1] * 7 and got["n_true"][f] == 1 and got["first_hit"][f] == 1
    t = row["the only true candidate in the last column"]
    assert got["n_true"][t] == 1 and got["first_hit"][t] == int((base > base[G - 1]).sum() + (base[:G - 1] == base[G - 1]).sum())
    assert got["ap"][t] == np.float32(1.0 / float(got["first_hit"][t] + 1))
    x = row["exclude on the last column"]
    assert (got["n_cand"][x], got["n_true"][x], got["first_hit"][x], got["ap"][x]) == (G - 1, 0, -1, 0)
    x = row["exclude on the only true candidate"]
    assert (got["n_cand"][x], got["n_true"][x], got["first_hit"][x], got["ap"][x]) == (G - 1, 0, -1, 0)
    i = row["+inf and both zeros among the winners"]
    assert got["topk_idx"][i, :6].tolist() == [3, G - 1, 10, 4095, 4096, 8192]
    assert np.array_equal(R.bits(got["topk_score"][i, 2:6]), R.bits(np.array([0.0, -0.0, 0.0, -0.0], np.float32)))
    n = row["a NaN in the last column"]
    assert got["info"][n] == 1 and (got["topk_idx"][n] == -1).all() and got["n_cand"][n] == 0 and got["first_hit"][n] == -1
    n = row["a NaN at the excluded last column"]
    assert got["info"][n] == 0 and got["n_cand"][n] == G - 1 and got["n_true"][n] == 3
    # K = 64 over the same rows: the ascending row now displaces 64 carried keys a step
    check(scores, qids, gids, 64, excl, "K = 64")


# ---- 4. the true cap ------------------------------------------------------------------------------------------------------------
def test_the_true_cap():
    G, K = 5000, 10
    g = np.random.default_rng(4)
    scores = np.stack([g.standard_normal(G).astype(np.float32) for _ in range(4)])
    scores[:, ::7] = np.float32(0.25)                           # ties among the true ones and the others
    gids = np.full(G, -1, np.int32)
    gids[g.permutation(G)[:4097]] = 1                           # 4097 entries of identity 1 ...
    last = int(np.flatnonzero(gids == 1)[-1])
    qids = np.array([1, 1, 1, -1], np.int32)
    excl = np.array([last, -1, -1, -1], np.int32)               # ... of which query 0 skips one: exactly 4096
    scores[2, 17] = np.nan                                      # a NaN takes precedence
    got = check(scores, qids, gids, K, excl)
    assert got["info"].tolist() == [0, 2, 1, 0] and got["n_true"].tolist() == [4096, 0, 0, 0]
    assert got["n_cand"].tolist() == [G - 1, 0, 0, G] and got["first_hit"][1] == -1 and got["ap"][1] == 0
    assert (got["topk_idx"][1] == -1).all() and (got["topk_score"][1] == NEG).all() and got["topk_idx"][3, 0] >= 0
    assert 0 < got["ap"][0] < 1
    book = RT.RankBook((1, 5), "cuda")
    book.add(run_wide(scores, qids, gids, K, excl), gallery=min(G, RT.MAX_GALLERY))
    counts, sums = R.accumulate([0] * 5, [0.0, 0.0], got, (1, 5))
    assert book.counts.cpu().tolist() == counts and counts[:3] == [1, 1, 2]           # scored, unscored, flagged
    assert np.array_equal(R.bits(book.sums.cpu().numpy()), R.bits(np.array(sums, np.float64)))
    assert book.metrics()["flagged"] == 2


# ---- 5. the score matrix by column windows --------------------------------------------------------------------------------------
def test_fill_and_scatter_over_three_blocks():
    Q, G = 5, 23
    g = np.random.default_rng(3)
    cap = 80
    cells = g.permutation(Q * G)[:cap]
    pairs = np.stack([cells // G, cells % G], axis=1).astype(np.int32)
    logits = g.standard_normal(cap).astype(np.float32)
    scores = torch.full((Q, G), 123.0, device="cuda")
    assert RT.fill_scores(scores) is scores and bool(torch.isneginf(scores).all())
    for col0, width in ((0, 9), (9, 9), (18, 5)):               # three blocks, the last one ragged
        inside = [k for k in range(cap) if col0 <= pairs[k, 1] < col0 + width]
        block = np.stack([pairs[inside, 0], pairs[inside, 1] - col0], axis=1).astype(np.int32)
        padded = np.concatenate([block, np.zeros((Q * width - len(inside), 2), np.int32)])          # compare_pairs' padding
        lg = np.concatenate([logits[inside], np.full(Q * width - len(inside), 99.0, np.float32)])
        assert RT.scatter_scores(dev(lg), dev(padded), dev(np.array([len(inside)], np.int32)), scores, col0, width) is scores
    assert np.array_equal(R.bits(scores.cpu().numpy()), R.bits(R.score_matrix(logits, pairs, cap, Q, G)))
    # pairs outside [0, Q) x [0, width) are skipped; the count is clamped; nothing outside the window is touched
    pairs = np.array([[0, 0], [1, 3], [Q, 0], [0, -1], [-1, 1], [2, 4], [4, 2], [3, 1]], np.int32)
    pairs[1], pairs[5] = (1, 4), (2, 5)                         # g = 4 is the window's last column, 5 the first outside
    logits = np.arange(1, 9, dtype=np.float32)
    for count in (0, 3, 8, 8 + 5, -2):
        sentinel = torch.full((Q, G), 55.0, device="cuda")
        RT.scatter_scores(dev(logits), dev(pairs), dev(np.array([count], np.int32)), sentinel, 10, 5)
        want = W.scatter(np.full((Q, G), 55.0, np.float32), logits, pairs, count, 10, 5)
        assert np.array_equal(R.bits(sentinel.cpu().numpy()), R.bits(want)), count
        inside = want[:, 10:15] != 55
        assert (want[:, :10] == 55).all() and (want[:, 15:] == 55).all() and inside.sum() == {0: 0, 3: 2, -2: 0}.get(count, 4)
    empty = torch.full((3, 7), 5.0, device="cuda")
    RT.scatter_scores(dev(logits[:0]), dev(pairs[:0]), dev(np.zeros(1, np.int32)), empty, 7, 0)       # an empty window
    assert bool((empty == 5).all()) and RT.fill_scores(torch.empty((0, 7), device="cuda")).shape == (0, 7)


# ---- 6. a captured graph ---------------------------------------------------------------------------------------------------------
def test_one_graph_of_fill_two_scatters_the_ranking_and_the_book():
    Q, G, K, ranks, split = 6, 5000, 10, (1, 5), 4096
    g = np.random.default_rng(21)
    windows = ((0, split), (split, G - split))
    lists = []
    for col0, width in windows:
        cells = g.permutation(Q * width)
        lists.append(np.stack([cells // width, cells % width], axis=1).astype(np.int32))
    qids, gids = g.integers(0, 4, Q).astype(np.int32), g.integers(0, 4, G).astype(np.int32)
    logits = [torch.zeros(len(p), device="cuda") for p in lists]
    counts = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in lists]
    pairs_d, qids_d, gids_d, valid = [dev(p) for p in lists], dev(qids), dev(gids), dev(np.array([Q - 1], np.int32))
    scores, out, book = torch.empty((Q, G), device="cuda"), RT.rank_buffers(Q, K, "cuda"), RT.RankBook(ranks, "cuda")

    def step():
        RT.fill_scores(scores)
        for (col0, width), lg, pr, ct in zip(windows, logits, pairs_d, counts):
            RT.scatter_scores(lg, pr, ct, scores, col0, width)
        res = RT.rank_gallery_wide(scores, qids_d, gids_d, topk=K, out=out)
        book.add(res, valid=valid, gallery=min(G, RT.MAX_GALLERY))
    step()                                                      # eager once: nothing is loaded inside the capture
    torch.cuda.synchronize()
    book.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    table, sums = [0] * 5, [0.0, 0.0]
    caps = [len(p) for p in lists]
    for seed, cs in ((1, caps), (2, (37, 0)), (3, (0, 0)), (4, (0, caps[1])), (5, (caps[0] + 9, 200))):
        new = [np.random.default_rng(10 * seed + b).standard_normal(caps[b]).astype(np.float32) for b in range(2)]
        want_scores = W.fill(Q, G)
        for b, (col0, width) in enumerate(windows):
            logits[b].copy_(dev(new[b]))
            counts[b].fill_(cs[b])
            W.scatter(want_scores, new[b], lists[b], cs[b], col0, width)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(R.bits(scores.cpu().numpy()), R.bits(want_scores)), cs
        want = W.rank_gallery(want_scores, qids, gids, K)
        assert_same(host(out), want, cs)
        table, sums = R.accumulate(table, sums, want, ranks, valid=Q - 1)
        assert book.counts.cpu().tolist() == table, cs
        assert np.array_equal(R.bits(book.sums.cpu().numpy()), R.bits(np.array(sums, np.float64))), cs
    assert table[0] > 0 and table[1] > 0


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
def test_retrieve_wide_equals_retrieve_whatever_the_block(toy):
    model, store, (q_rows, g_rows, q_cls, g_cls, q_ids, g_ids) = toy
    q_xyz, q_feats, q_len = encoded(model, store, q_rows)
    g_xyz, g_feats, g_len = encoded(model, store, g_rows)
    Q, G, K = len(q_rows), len(g_rows), 5
    excl = dev(np.arange(Q, dtype=np.int32) % G)
    for live_only in (False, True):
        args = (q_feats, q_xyz, dev(q_cls), q_len, g_feats, g_xyz, dev(g_cls), g_len)
        kw = dict(query_ids=dev(q_ids), gallery_ids=dev(g_ids), topk=K, num_classes=2, live_only=live_only)
        with torch.no_grad():
            narrow = model.retrieve(*args, **kw)
            narrow_ex = model.retrieve(*args, exclude=excl, **kw)
        assert int(narrow["n_true"].sum()) == Q
        for block in (4, 15, 4096):
            with torch.no_grad():
                wide = model.retrieve_wide(*args, gallery_block=block, **kw)
                wide_ex = model.retrieve_wide(*args, gallery_block=block, exclude=excl, **kw)
            assert sorted(wide) == sorted(RT.OUTPUTS + ("scores", "counts"))
            for a, b in ((wide, narrow), (wide_ex, narrow_ex)):
                assert np.array_equal(R.bits(a["scores"].cpu().numpy()), R.bits(b["scores"].cpu().numpy())), (block, live_only)
                assert_same(host(a), host(b), (block, live_only))
            blocks = -(-G // block)
            assert wide["counts"].shape == (blocks,) and wide["counts"].dtype == torch.int32
            assert int(wide["counts"].sum()) == int(narrow["count"][0])
    buf = torch.full((Q, G), 3.0, device="cuda")                # a given score buffer is written into
    with torch.no_grad():
        again = model.retrieve_wide(*args, gallery_block=4, scores=buf, **kw)
    assert again["scores"] is buf and torch.equal(buf, wide["scores"])


def test_evaluate_retrieval_above_the_cap(toy):
    model, store, split = toy
    big = tuple(np.concatenate([a] * 400) for a in split[1::2])
    wide_split = (split[0], big[0], split[2], big[1], split[4], big[2])
    G, K = len(big[0]), 5
    assert G == 6000
    runs = [RT.evaluate_retrieval(model, store, wide_split, n=N, seed=0, topk=K, ranks=(1, 5), query_chunk=c, gallery_block=4096)
            for c in (64, 5)]
    ref = runs[0]
    assert (ref["scored"], ref["unscored"], ref["flagged"]) == (NOBJ, 0, 0)
    assert (ref["n_true"] == 400).all() and ref["topk_idx"].shape == (NOBJ, K)
    for k in RT.OUTPUTS:                                        # whatever the query chunk
        assert np.array_equal(R.bits(ref[k].cpu().numpy()), R.bits(runs[1][k].cpu().numpy())), k
    assert torch.equal(ref["book"].counts, runs[1]["book"].counts) and torch.equal(ref["book"].sums, runs[1]["book"].sums)
    # retrieve_wide called directly, and the restatement over its scores
    put = lambda a: dev(np.asarray(a, np.int32))                # noqa: E731
    with torch.no_grad():
        q_clouds, q_len = store.gather(put(split[0]), N, keys=put(split[0]), seed=0)
        g_clouds, g_len = store.gather(put(big[0]), N, keys=put(big[0]), seed=0)
        q_xyz, q_feats = RT._encode(model, q_clouds, 256)
        g_xyz, g_feats = RT._encode(model, g_clouds, 256)
        res = model.retrieve_wide(q_feats, q_xyz, put(split[2]), q_len, g_feats, g_xyz, put(big[1]), g_len, query_ids=put(split[4]),
                                  gallery_ids=put(big[2]), topk=K, num_classes=2, live_only=True, gallery_block=4096)
    assert res["counts"].shape == (2,) and res["scores"].shape == (NOBJ, G)
    assert_same({k: ref[k].cpu().numpy() for k in RT.OUTPUTS}, host(res), "evaluate_retrieval against retrieve_wide")
    scores = res["scores"].cpu().numpy()
    assert_same(host(res), W.rank_gallery(scores, split[4], big[2], K), "retrieve_wide against the restatement")
    # identical clouds score identically in any batch position
    assert np.array_equal(R.bits(scores), R.bits(scores[:, np.arange(G) % 15]))
    with pytest.raises(L.PcrError, match="gallery_block"):      # the narrow route still refuses, and names the wide one
        RT.evaluate_retrieval(model, store, wide_split, n=N)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(toy):
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")      # noqa: E731
    wide = torch.zeros(2, 5000, device="cuda")
    for bad in (dict(topk=0), dict(topk=65)):
        with pytest.raises(L.PcrError):
            RT.rank_gallery_wide(wide, i32(2), i32(5000), **bad)
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(torch.zeros(2, 5000), i32(2), i32(5000))                             # a host tensor
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(wide, i32(2).long(), i32(5000))                                      # int64 ids
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(wide, i32(2), i32(5000).long())
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(wide.double(), i32(2), i32(5000))
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(wide, i32(3), i32(5000))                                             # a wrong shape
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(wide, i32(2), i32(5000), exclude=i32(2).long())
    too_wide = torch.empty(1, RT.WIDE_MAX_GALLERY + 1, device="cuda")                             # 16 MiB, never read
    with pytest.raises(L.PcrError):
        RT.rank_gallery_wide(too_wide, i32(1), i32(RT.WIDE_MAX_GALLERY + 1))
    with pytest.raises(L.PcrError):
        RT.fill_scores(too_wide)
    with pytest.raises(L.PcrError):
        RT.fill_scores(torch.zeros(2, 8))
    pairs = torch.zeros(6, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(L.PcrError):
        RT.scatter_scores(torch.zeros(6, device="cuda"), pairs, i32(1), wide, 4998, 3)            # col0 + width > G
    with pytest.raises(L.PcrError):
        RT.scatter_scores(torch.zeros(6, device="cuda"), pairs, i32(1), wide, 0, 2)               # cap > Q * width
    with pytest.raises(L.PcrError):
        RT.scatter_scores(torch.zeros(6, device="cuda"), pairs.long(), i32(1), wide, 0, 3)
    with pytest.raises(L.PcrError):
        RT.rank_gallery(wide, i32(2), i32(5000))                                                  # the narrow entry as before
    model, store, split = toy
    q_xyz, q_feats, q_len = encoded(model, store, split[0])
    g_xyz, g_feats, g_len = encoded(model, store, split[1])
    for block in (0, 4097):
        with pytest.raises(L.PcrError):
            model.retrieve_wide(q_feats, q_xyz, dev(split[2]), q_len, g_feats, g_xyz, dev(split[3]), g_len, gallery_block=block)
        with pytest.raises(L.PcrError):
            RT.evaluate_retrieval(model, store, split, n=N, gallery_block=block)
    with pytest.raises(L.PcrError):
        model.retrieve_wide(q_feats, q_xyz, dev(split[2]), q_len, g_feats, g_xyz, dev(split[3]), g_len, topk=65)
