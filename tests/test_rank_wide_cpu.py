"""CPU: ranking a wide gallery (include/pcr.h section A12).  The restatement the GPU tests compare against
(tests/rank_wide_ref.py, one lexsort per row) equals section A8's (tests/rank_ref.py, a count per rank) bit for bit where
both apply, and implements the true-set cap; the four entry points exist, are declared once in the binding, and refuse
what they must without a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_ref as R
import rank_wide_ref as W
from conftest import ROOT
from test_rank_cpu import planted_rows

INVALID = 1
SYMBOLS = ("pcr_rank_wide_ok", "pcr_rank_fill_f32", "pcr_rank_scatter_f32", "pcr_rank_wide_f32")


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def assert_same(got, want, what=""):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (what, k)


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 7, 64, 65, 150, 300])
def test_wide_restatement_equals_the_narrow_one(G):
    Q = 12
    scores, qids, gids, exclude = planted_rows(300 + G, Q, G)
    for K in (1, 10, 64):
        assert_same(W.rank_gallery(scores, qids, gids, K, exclude), R.rank_gallery(scores, qids, gids, K, exclude), (G, K))
    assert_same(W.rank_gallery(scores, qids, gids, 10), R.rank_gallery(scores, qids, gids, 10), (G, "no exclusion"))
    assert_same(W.rank_gallery(scores, None, None, 10, exclude), R.rank_gallery(scores, None, None, 10, exclude), (G, "no ids"))
    nan = scores.copy()
    nan[0, G // 2], nan[1, G - 1] = np.nan, np.nan          # a NaN candidate; a NaN at the excluded slot
    ex = exclude.copy()
    ex[0], ex[1] = -1, G - 1
    got = W.rank_gallery(nan, qids, gids, 10, ex)
    assert_same(got, R.rank_gallery(nan, qids, gids, 10, ex), (G, "NaN"))
    assert got["info"][0] == 1 and got["info"][1] == 0
    if G >= 64:
        assert (got["n_true"] > 1).any()


def test_the_true_cap():
    gids = np.array([3, 3, 4, 3, -1, 3, 3], np.int32)
    row = np.array([1.0, 0.5, 2.0, 0.5, 9.0, -np.inf, 0.25], np.float32)
    idx, sc, n_cand, n_true, fh, ap, info = W.rank_query(row, 3, gids, 3, max_true=4)       # four true ones: ranked
    assert info == 0 and idx.tolist() == [4, 2, 0] and (n_cand, n_true, fh) == (6, 4, 2)
    assert ap == np.float32((1.0 / 3.0 + 2.0 / 4.0 + 3.0 / 5.0 + 4.0 / 6.0) / 4.0)
    three = W.rank_query(row, 3, gids, 3, exclude=6, max_true=3)                           # a true set of 3 at a cap of 3
    assert three[-1] == 0 and three[3] == 3
    idx, sc, n_cand, n_true, fh, ap, info = W.rank_query(row, 3, gids, 3, max_true=3)       # a true set of 4
    assert info == 2 and idx.tolist() == [-1, -1, -1] and np.isneginf(sc).all()
    assert (n_cand, n_true, fh, float(ap)) == (0, 0, -1, 0.0)
    nan = row.copy()
    nan[4] = np.nan                                          # a NaN candidate beside 4 true ones
    assert W.rank_query(nan, 3, gids, 3, max_true=3)[-1] == 1
    assert W.rank_query(nan, 3, gids, 3, exclude=4, max_true=3)[-1] == 2                   # the NaN is no candidate's
    assert W.rank_query(row, 4, gids, 3, max_true=0)[-1] == 2 and W.rank_query(row, -1, gids, 3, max_true=0)[-1] == 0
    out = W.rank_gallery(np.stack([row, nan]), np.array([3, 3], np.int32), gids, 2, max_true=3)
    assert out["info"].tolist() == [2, 1] and (out["topk_idx"] == -1).all() and not out["n_true"].any()
    assert W.MAX_TRUE == header_int("PCR_RANK_WIDE_MAX_TRUE")


def test_fill_and_scatter_by_column_windows():
    Q, G = 4, 11
    g = np.random.default_rng(5)
    cells = g.permutation(Q * G)
    pairs = np.stack([cells // G, cells % G], axis=1).astype(np.int32)
    logits = g.standard_normal(Q * G).astype(np.float32)
    want = R.score_matrix(logits, pairs, 30, Q, G)
    got = W.fill(Q, G)
    assert np.isneginf(got).all() and got.dtype == np.float32
    for col0, width in ((0, 4), (4, 4), (8, 3)):            # three blocks, the last one ragged
        inside = [k for k in range(30) if col0 <= pairs[k, 1] < col0 + width]
        block = np.stack([pairs[inside, 0], pairs[inside, 1] - col0], axis=1)
        W.scatter(got, logits[inside], block, len(inside), col0, width)
    assert np.array_equal(R.bits(got), R.bits(want))
    sentinel = np.full((Q, G), 7.0, np.float32)
    W.scatter(sentinel, np.ones(4, np.float32), np.array([[0, 0], [1, 3], [Q, 0], [0, -1]], np.int32), 9, 4, 3)
    assert sentinel[0, 4] == 1 and (sentinel == 1).sum() == 1           # (1, 3), (Q, 0), (0, -1) are outside the window
    W.scatter(sentinel, np.ones(4, np.float32), np.array([[0, 1]] * 4, np.int32), -2, 4, 3)
    assert (sentinel == 1).sum() == 1


# ---- 2. the ABI ----------------------------------------------------------------------------------------------------------------
def test_constants_and_signatures(lib):
    from pcr_amd import abi, retrieval
    assert header_int("PCR_RANK_WIDE_MAX_GALLERY") == retrieval.WIDE_MAX_GALLERY == 4194304
    assert header_int("PCR_RANK_WIDE_MAX_TRUE") == retrieval.WIDE_MAX_TRUE == 4096
    assert header_int("PCR_RANK_MAX_GALLERY") == retrieval.MAX_GALLERY == 4096
    for s in SYMBOLS:
        assert s in abi.SIGNATURES and hasattr(lib, s), s
    assert abi.SIGNATURES["pcr_rank_wide_f32"] == abi.SIGNATURES["pcr_rank_gallery_f32"] == "s <RankParams>S"
    assert abi.SIGNATURES["pcr_rank_scatter_f32"] == "s FIIFiiiiiS" and abi.SIGNATURES["pcr_rank_fill_f32"] == "s FiiS"
    assert lib.pcr_abi_version() == 17


def test_ok_ranges(lib):
    ok = lib.pcr_rank_wide_ok
    assert ok(0, 0, 1) == 1 and ok(65535, 4194304, 64) == 1 and ok(3, 5000, 10) == 1
    assert ok(1, 4194305, 1) == 0 and ok(1, 1, 0) == 0 and ok(1, 1, 65) == 0 and ok(65536, 1, 1) == 0
    assert ok(-1, 1, 1) == 0 and ok(1, -1, 1) == 0 and ok(1, 1, -1) == 0
    assert lib.pcr_rank_ok(1, 4097, 1, 0) == 0                   # the narrow entries keep their limit
    from pcr_amd import retrieval
    assert retrieval.rank_wide_ok(70, 40000, 10) and retrieval.rank_wide_ok(1, 4097) and not retrieval.rank_wide_ok(1, 1, 65)


def test_null_and_out_of_range_arguments_return_invalid(lib):
    from pcr_amd import abi
    fbuf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    f, i = (ctypes.cast(b, ctypes.c_void_p) for b in (fbuf, ibuf))
    # (host pointers: each call below must be refused, or find nothing to do, before anything is launched)
    fill = lib.pcr_rank_fill_f32
    assert fill(None, 2, 3, None) == INVALID
    assert fill(f, 1, 4194305, None) == INVALID and fill(f, 65536, 1, None) == INVALID and fill(f, -1, 3, None) == INVALID
    assert fill(None, 0, 3, None) == 0 and fill(None, 3, 0, None) == 0                      # nothing to do

    sc = lib.pcr_rank_scatter_f32
    assert sc(f, i, i, None, 2, 8, 6, 2, 3, None) == INVALID                # scores
    assert sc(None, i, i, f, 2, 8, 6, 2, 3, None) == INVALID                # logits
    assert sc(f, None, i, f, 2, 8, 6, 2, 3, None) == INVALID                # pairs
    assert sc(f, i, None, f, 2, 8, 6, 2, 3, None) == INVALID                # count
    assert sc(f, i, i, f, 2, 8, 6, 6, 3, None) == INVALID                   # col0 + width > G
    assert sc(f, i, i, f, 2, 8, 6, 2 ** 31 - 1, 3, None) == INVALID         # ... not wrapped
    assert sc(f, i, i, f, 2, 8, 6, -1, 3, None) == INVALID and sc(f, i, i, f, 2, 8, 0, 2, -1, None) == INVALID
    assert sc(f, i, i, f, 2, 8, 7, 2, 3, None) == INVALID                   # cap > Q * width
    assert sc(f, i, i, f, 2, 8, -1, 2, 3, None) == INVALID
    assert sc(f, i, i, f, 1, 4194305, 1, 0, 1, None) == INVALID and sc(f, i, i, f, 65536, 8, 1, 0, 1, None) == INVALID
    # Q * width = 65535 * 32769 is above 2^31: wrapped to 32 bits it would be negative and refuse every cap, 0 included
    assert sc(None, None, None, None, 65535, 32769, 0, 0, 32769, None) == 0
    assert sc(None, None, None, None, 2, 8, 0, 2, 3, None) == 0 and sc(None, None, None, None, 0, 8, 0, 0, 8, None) == 0
    assert sc(f, i, i, f, 0, 8, 1, 0, 8, None) == INVALID                   # cap 1 > 0 * 8

    def block(**over):
        p = abi.RankParams()
        p.Q, p.G, p.K = 2, 3, 2
        p.scores, p.topk_score, p.ap = f.value, f.value, f.value
        for k in ("query_ids", "gallery_ids", "topk_idx", "n_cand", "n_true", "first_hit", "info"):
            setattr(p, k, i.value)
        for k, v in over.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    rank = lib.pcr_rank_wide_f32
    assert rank(None, None) == INVALID
    for k in ("scores", "query_ids", "gallery_ids", "topk_idx", "topk_score", "n_cand", "n_true", "first_hit", "ap", "info"):
        assert rank(block(**{k: None}), None) == INVALID, k
    for over in (dict(K=0), dict(K=65), dict(G=4194305), dict(G=-1), dict(Q=65536), dict(Q=-1)):
        assert rank(block(**over), None) == INVALID, over
    assert rank(block(Q=0, scores=None, query_ids=None, topk_idx=None), None) == 0      # nothing to do
    assert lib.pcr_rank_gallery_f32(block(G=4097), None) == INVALID                     # the narrow entry as before


def test_python_entries_refuse_host_tensors():
    import torch
    from pcr_amd import retrieval
    from pcr_amd._lib import PcrError
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)       # noqa: E731
    with pytest.raises(PcrError):
        retrieval.rank_gallery_wide(torch.zeros(2, 5000), i32(2), i32(5000))
    with pytest.raises(PcrError):
        retrieval.fill_scores(torch.zeros(2, 5000))
    with pytest.raises(PcrError):
        retrieval.scatter_scores(torch.zeros(6), torch.zeros(6, 2, dtype=torch.int32), i32(1), torch.zeros(2, 5000), 4000, 3)
    with pytest.raises(PcrError):                           # col0 + width > G: refused before the device is looked at
        retrieval.scatter_scores(torch.zeros(6), torch.zeros(6, 2, dtype=torch.int32), i32(1), torch.zeros(2, 8), 6, 3)
