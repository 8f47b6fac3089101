"""CPU: the ranking entry points (include/pcr.h section A8) exist and refuse what they must without a launch; the numpy
restatement the GPU tests compare against (tests/rank_ref.py) is held to an independent check -- np.lexsort for the order,
fractions.Fraction for the average precision, which the restatement must meet to within one binary32 rounding of the exact
value; retrieval_split on a hand-made object table."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import rank_ref as R
from conftest import ROOT

INVALID = 1
SYMBOLS = ("pcr_rank_ok", "pcr_rank_scores_f32", "pcr_rank_gallery_f32", "pcr_rank_accumulate")


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


# ---- 1. the restatement against an independent check ------------------------------------------------------------------------
def planted_rows(seed, Q, G):
    """random scores from a small set of values (many ties, both zeros, both infinities as scores and as holes)"""
    g = np.random.default_rng(seed)
    values = np.array([-np.inf, -2.5, -0.0, 0.0, 0.5, 0.5, 1.25, 7.0, np.inf], np.float32)
    scores = values[g.integers(0, len(values), (Q, G))]
    fine = g.standard_normal((Q, G)).astype(np.float32)
    scores = np.where(g.random((Q, G)) < 0.5, scores, fine)
    gids = g.integers(-1, 6, G).astype(np.int32)
    qids = g.integers(-1, 6, Q).astype(np.int32)
    exclude = g.integers(-2, G + 2, Q).astype(np.int32)
    return scores, qids, gids, exclude


@pytest.mark.parametrize("G", [1, 7, 64, 65, 150])
def test_restatement_equals_lexsort_and_exact_fractions(G):
    Q, K = 12, 10
    scores, qids, gids, exclude = planted_rows(100 + G, Q, G)
    got = R.rank_gallery(scores, qids, gids, K, exclude)
    assert not got["info"].any()
    for q in range(Q):
        ex = exclude[q] if 0 <= exclude[q] < G else -1
        cand = np.array([g for g in range(G) if g != ex and scores[q, g] != -np.inf], dtype=np.int64)
        s = scores[q, cand].astype(np.float64) + 0.0           # (-0 + 0 = +0: lexsort sees the float compare's equality)
        order = cand[np.lexsort((cand, -s))]
        assert got["n_cand"][q] == len(cand)
        k = min(K, len(cand))
        assert got["topk_idx"][q, :k].tolist() == order[:k].tolist() and (got["topk_idx"][q, k:] == -1).all()
        assert np.array_equal(R.bits(got["topk_score"][q, :k]), R.bits(scores[q, order[:k]]))
        assert (got["topk_score"][q, k:] == -np.inf).all()
        hits = [r for r, g in enumerate(order) if qids[q] >= 0 and gids[g] == qids[q]]
        assert got["n_true"][q] == len(hits) and got["first_hit"][q] == (hits[0] if hits else -1)
        if hits:
            exact = sum(Fraction(i + 1, r + 1) for i, r in enumerate(hits)) / len(hits)
            ap = Fraction(float(got["ap"][q]))
            assert abs(ap - exact) <= exact * Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60), (q, float(ap), float(exact))
        else:
            assert got["ap"][q] == 0
    if G >= 64:
        assert (got["n_true"] > 1).any() and (got["n_cand"] < G).any()


def test_restatement_nan_rule_and_empty_rows():
    gids = np.array([3, 3, 4, -1], np.int32)
    row = np.array([1.0, np.nan, 0.5, 2.0], np.float32)
    assert R.rank_query(row, 3, gids, 3)[-1] == 1 and R.rank_query(row, 3, gids, 3)[0].tolist() == [-1, -1, -1]
    idx, sc, n_cand, n_true, fh, ap, info = R.rank_query(row, 3, gids, 3, exclude=1)      # the NaN is no candidate's
    assert info == 0 and idx.tolist() == [3, 0, 2] and (n_cand, n_true, fh) == (3, 1, 1) and ap == np.float32(0.5)
    idx, sc, n_cand, n_true, fh, ap, info = R.rank_query(np.full(4, -np.inf, np.float32), 3, gids, 2)
    assert info == 0 and idx.tolist() == [-1, -1] and (n_cand, n_true, fh, float(ap)) == (0, 0, -1, 0.0)
    idx = R.rank_query(np.array([-0.0, 0.0, np.inf, 0.0], np.float32), -1, gids, 4)[0]
    assert idx.tolist() == [2, 0, 1, 3]                         # +inf is a score; the zeros tie, lowest index first


def test_restatement_score_matrix_and_accumulate():
    pairs = np.array([[0, 1], [1, 0], [2, 5], [-1, 0], [1, 2]], np.int32)
    logits = np.arange(1, 6, dtype=np.float32)
    s = R.score_matrix(logits, pairs, 4, 2, 3)
    assert s[0, 1] == 1 and s[1, 0] == 2 and np.isneginf(s).sum() == 4          # (2, 5), (-1, 0) skipped; k = 4 beyond count
    assert np.isneginf(R.score_matrix(logits, pairs, -3, 2, 3)).all()
    assert R.score_matrix(logits, pairs, 99, 2, 3)[1, 2] == 5
    res = dict(info=[0, 1, 0, 0], n_true=[2, 0, 0, 1], first_hit=[0, -1, -1, 4], ap=np.array([0.75, 0, 0, 0.2], np.float32))
    counts, sums = R.accumulate([0] * 5, [0.0, 0.0], res, (1, 5))
    assert counts == [2, 1, 1, 1, 2] and sums == [0.75 + float(np.float32(0.2)), 1.0 + 1.0 / 5.0]
    counts, sums = R.accumulate(counts, sums, res, (1, 5), valid=1)
    assert counts == [3, 1, 1, 2, 3]


# ---- 2. the ABI -------------------------------------------------------------------------------------------------------------
def test_constants_and_signatures(lib):
    from pcr_amd import abi, retrieval
    assert header_int("PCR_RANK_MAX_QUERIES") == retrieval.MAX_QUERIES == 65535
    assert header_int("PCR_RANK_MAX_GALLERY") == retrieval.MAX_GALLERY == header_int("PCR_ASSOC_MAX_OBJECTS") == 4096
    assert header_int("PCR_RANK_MAX_K") == retrieval.MAX_K == 64
    assert header_int("PCR_RANK_MAX_RANKS") == retrieval.MAX_RANKS == 8
    for s in SYMBOLS:
        assert s in abi.SIGNATURES and hasattr(lib, s), s
    assert abi.SIGNATURES["pcr_rank_gallery_f32"] == "s <RankParams>S"
    assert abi.SIGNATURES["pcr_rank_accumulate"] == "s <RankAccParams>S"
    assert lib.pcr_abi_version() == 17


def test_ok_ranges(lib):
    ok = lib.pcr_rank_ok
    assert ok(0, 0, 1, 0) == 1 and ok(65535, 4096, 64, 65535 * 4096) == 1 and ok(3, 5, 10, 15) == 1
    assert ok(65536, 1, 1, 0) == 0 and ok(-1, 1, 1, 0) == 0
    assert ok(1, 4097, 1, 0) == 0 and ok(1, -1, 1, 0) == 0
    assert ok(1, 1, 0, 0) == 0 and ok(1, 1, 65, 0) == 0 and ok(1, 1, 64, 1) == 1
    assert ok(3, 5, 1, 16) == 0 and ok(3, 5, 1, -1) == 0 and ok(0, 5, 1, 1) == 0
    assert ok(65535, 4096, 1, 2 ** 31 - 1) == 0                 # Q * G = 268431360 < 2^31 - 1: the product is not wrapped
    from pcr_amd import retrieval
    assert retrieval.rank_ok(70, 130, 10, 9100) and not retrieval.rank_ok(70, 130, 10, 9101)


def test_null_and_out_of_range_arguments_return_invalid(lib):
    from pcr_amd import abi
    fbuf, ibuf, dbuf = (ctypes.c_float * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 2)()
    f, i, d = (ctypes.cast(b, ctypes.c_void_p) for b in (fbuf, ibuf, dbuf))
    # (host pointers: each call below must be refused before anything is launched)
    sc = lib.pcr_rank_scores_f32
    assert sc(f, i, i, None, 2, 3, 6, None) == INVALID                      # scores
    assert sc(None, i, i, f, 2, 3, 6, None) == INVALID                      # logits
    assert sc(f, None, i, f, 2, 3, 6, None) == INVALID                      # pairs
    assert sc(f, i, None, f, 2, 3, 6, None) == INVALID                      # count
    assert sc(f, i, i, f, 2, 3, 7, None) == INVALID                         # cap > Q * G
    assert sc(f, i, i, f, 2, 4097, 6, None) == INVALID and sc(f, i, i, f, 65536, 3, 6, None) == INVALID
    assert sc(None, None, None, None, 0, 3, 0, None) == 0 and sc(None, None, None, None, 3, 0, 0, None) == 0     # nothing to do

    def block(**over):
        p = abi.RankParams()
        p.Q, p.G, p.K = 2, 3, 2
        p.scores, p.topk_score, p.ap = f.value, f.value, f.value
        for k in ("query_ids", "gallery_ids", "topk_idx", "n_cand", "n_true", "first_hit", "info"):
            setattr(p, k, i.value)
        for k, v in over.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    rank = lib.pcr_rank_gallery_f32
    assert rank(None, None) == INVALID
    for k in ("scores", "query_ids", "gallery_ids", "topk_idx", "topk_score", "n_cand", "n_true", "first_hit", "ap", "info"):
        assert rank(block(**{k: None}), None) == INVALID, k
    for over in (dict(K=0), dict(K=65), dict(G=4097), dict(G=-1), dict(Q=65536), dict(Q=-1)):
        assert rank(block(**over), None) == INVALID, over
    assert rank(block(Q=0, scores=None, query_ids=None, topk_idx=None), None) == 0      # nothing to do

    def acc_block(ranks=(1, 3), **over):
        p = abi.RankAccParams()
        p.Q, p.G, p.nranks = 2, 3, len(ranks)
        for k, r in enumerate(ranks[:8]):
            p.ranks[k] = r
        p.n_true, p.first_hit, p.info, p.ap, p.counts, p.sums = i.value, i.value, i.value, f.value, i.value, d.value
        for k, v in over.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    acc = lib.pcr_rank_accumulate
    assert acc(None, None) == INVALID
    for k in ("n_true", "first_hit", "info", "ap", "counts", "sums"):
        assert acc(acc_block(**{k: None}), None) == INVALID, k
    assert acc(acc_block(ranks=(0,)), None) == INVALID and acc(acc_block(ranks=(4,)), None) == INVALID      # outside [1, G]
    assert acc(acc_block(nranks=9), None) == INVALID and acc(acc_block(nranks=-1), None) == INVALID
    assert acc(acc_block(Q=65536), None) == INVALID and acc(acc_block(G=4097), None) == INVALID
    assert acc(acc_block(Q=0, n_true=None, first_hit=None, info=None, ap=None), None) == 0                 # nothing to do


def test_python_entries_refuse_host_tensors():
    import torch
    from pcr_amd import retrieval
    from pcr_amd._lib import PcrError
    with pytest.raises(PcrError):
        retrieval.rank_gallery(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(PcrError):
        retrieval.score_matrix(torch.zeros(6), torch.zeros(6, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 2, 3)
    with pytest.raises(PcrError):
        retrieval.RankBook(ranks=range(1, 10), device="cpu")
    with pytest.raises(PcrError):
        retrieval.RankBook(ranks=(0,), device="cpu")


# ---- 3. the split -----------------------------------------------------------------------------------------------------------
def hand_table():
    from pcr_amd.pairs import ObjectTable
    objs = [dict(token="A%d" % i, cls=i % 2, frames={n: 50 + n for n in range(3 + i % 3)}, fp=False) for i in range(7)]
    objs.insert(2, dict(token="S0", cls=0, frames={0: 40, 1: 41}, fp=False))           # too short to be a query
    objs.insert(5, dict(token="F0", cls=1, frames={4: 9}, fp=True))                    # a false positive
    objs.append(dict(token="U0", cls=-1, frames={0: 30, 1: 30, 2: 30}, fp=False))      # not a tracked class
    objs.append(dict(token="E0", cls=1, frames={0: 0}, fp=True))                       # no observation with a point
    table = ObjectTable(objs, num_classes=2)
    row_of = {}
    for o in objs:
        for n in sorted(o["frames"]):
            row_of[(o["token"], n)] = len(row_of)
    return table, row_of


def test_retrieval_split_on_a_hand_made_table():
    from pcr_amd import retrieval
    table, row_of = hand_table()
    key_of = {r: k for k, r in row_of.items()}
    split = retrieval.retrieval_split(table, row_of, seed=4)
    q_rows, g_rows, q_cls, g_cls, q_ids, g_ids = split
    assert all(a.dtype == np.int32 for a in split)
    assert q_ids.tolist() == table.true_index and len(table.true_index) == 7
    for row, cls, i in zip(q_rows, q_cls, q_ids):
        o = table.objects[i]
        partner = [g for g in range(len(g_rows)) if g_ids[g] == i]
        assert len(partner) == 1                                 # the partner is in the gallery under the same id ...
        tok, obs = key_of[int(g_rows[partner[0]])]
        assert tok == o["token"] == key_of[int(row)][0] and obs != key_of[int(row)][1]      # ... on another observation
        assert cls == o["cls"] == g_cls[partner[0]]
    distractors = [key_of[int(r)][0] for r, i in zip(g_rows, g_ids) if i == -1]
    assert sorted(distractors) == ["F0", "S0"] and len(g_rows) == 9           # U0 (class -1) and E0 (no observation) give none
    again = retrieval.retrieval_split(table, row_of, seed=4)
    assert all(np.array_equal(a, b) for a, b in zip(split, again))
    other = retrieval.retrieval_split(table, row_of, seed=5)
    assert not all(np.array_equal(a, b) for a, b in zip(split, other))
    # the draw is the one written down
    i = table.true_index[3]
    obs = table.objects[i]["nums"]
    a, b = np.random.default_rng([4, i]).choice(len(obs), 2, replace=False)
    assert q_rows[3] == row_of[(table.objects[i]["token"], obs[a])]
    assert g_rows[g_ids.tolist().index(i)] == row_of[(table.objects[i]["token"], obs[b])]
