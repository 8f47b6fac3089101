"""CPU: the block rule of include/pcr.h section A3.  The new entry points exist and are declared; the numpy restatement
(tests/assoc_blocks_ref.py) with one block equals assoc_ref.lsa; and solving a frame's matrix class by class decodes to the
same frame as the full solve, on random scenes with unlabelled and short objects, for every decision layout the tracker runs
-- the one known difference, the count of void fill entries where the full problem is forced to pair leftovers across classes,
is the only output left out, and only for the two layouts that force it."""
import numpy as np
import pytest

import assoc_blocks_ref as B
import assoc_ref as A
import decisions_ref as R

NEW_SYMBOLS = ("pcr_lsa_blocks_ok", "pcr_lsa_blocks_f32", "pcr_assoc_blocks_i32")
INVALID = 1
CLASSES = 4
SIZES = ((5, 3), (17, 9), (40, 30), (70, 33))
SEEDS = range(12)
# (dd, td, reduce); the full problem pairs leftovers across classes under the last two: info[1] is not compared there
EQUAL = [(dd, td, red) for dd, td in ((1, 1), (2, 0), (2, 1), (1, 0), (0, 1)) for red in (False, True)] + [(4, 4, True)]
EQUAL_BUT_VOIDS = [(0, 0, False), (4, 4, False)]


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def scene(T, D, dd, td, seed):
    """4 classes, 30 % of the objects without a class, 15 % below min_points; N(0, 16) logits, N(0, 1) decision values"""
    g = np.random.default_rng([seed, T, D])
    tl, dl = g.integers(0, CLASSES, T), g.integers(0, CLASSES, D)
    tl[g.random(T) < 0.3], dl[g.random(D) < 0.3] = -1, -1
    tn, dn = np.where(g.random(T) < 0.15, 1, 10), np.where(g.random(D) < 0.15, 1, 10)
    pairs, count = A.compare_pairs(tl, dl, tn, dn, min_points=2, num_classes=CLASSES)
    logits = (g.standard_normal(len(pairs)) * 4.0).astype(np.float32)
    return tl, dl, logits, pairs, count, g.standard_normal((dd, D)).astype(np.float32), \
        g.standard_normal((td, T)).astype(np.float32)


def both_routes(T, D, dd, td, reduce, kind, seed):
    tl, dl, logits, pairs, count, det_dec, trk_dec = scene(T, D, dd, td, seed)
    out = R.cost_multi(logits, pairs, count, T, D, det_dec, trk_dec, dd=dd, td=td, kind=kind, reduce=reduce)
    cost, choices = (out[0], (out[1], out[2])) if reduce else (out, None)
    c4r, r4c, _, _, info = A.lsa(cost)
    full = R.decode(cost, c4r, r4c, T, D, dd, td, choices=choices, born_dec=dd - 1, kill_dec=td - 1, solver_info=info)
    de, te = (R.shape(T, D, dd, td, reduce)[0] - T) // D, (R.shape(T, D, dd, td, reduce)[1] - D) // T
    rb, cb, G = B.block_ids(tl, dl, T, D, de, te, CLASSES)
    c4r, r4c, _, _, binfo = B.lsa_blocks(cost, rb, cb, G)
    blocks = R.decode(cost, c4r, r4c, T, D, dd, td, choices=choices, born_dec=dd - 1, kill_dec=td - 1,
                      solver_info=int(binfo.max()))
    return full, blocks


def assert_same_frame(full, blocks, voids, what):
    for k in full:
        a, b = full[k], blocks[k]
        if k == "info" and not voids:
            a, b = np.delete(a, 1), np.delete(b, 1)
        assert np.array_equal(a, b), "%s: %s differs between the full and the block solve" % (what, k)


def test_new_symbols_are_exported_declared_and_abi_is_17(lib):
    from pcr_amd import abi
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
        assert s in abi.SIGNATURES
    assert lib.pcr_abi_version() == 17


def test_blocks_ok_edges_and_refusals_without_a_launch(lib):
    ok = lib.pcr_lsa_blocks_ok
    assert ok(0, 0, 1) == 1 and ok(1024, 1024, 33) == 1 and ok(300, 0, 9) == 1
    assert ok(1025, 4, 1) == 0 and ok(4, 1025, 1) == 0 and ok(-1, 4, 1) == 0 and ok(4, -1, 1) == 0
    assert ok(4, 4, 0) == 0 and ok(4, 4, 34) == 0
    assert lib.pcr_lsa_blocks_f32(None, None, None, None, None, None, None, None, 4, 4, 0, None) == INVALID
    assert lib.pcr_lsa_blocks_f32(None, None, None, None, None, None, None, None, 4, 4, 2, None) == INVALID   # no pointers
    assert lib.pcr_assoc_blocks_i32(None, None, None, None, 4, 4, 5, 0, 8, None) == INVALID   # beyond the decisions
    assert lib.pcr_assoc_blocks_i32(None, None, None, None, 4, 4, 1, 1, 0, None) == INVALID   # no class
    assert lib.pcr_assoc_blocks_i32(None, None, None, None, 4, 4, 1, 1, 33, None) == INVALID
    assert lib.pcr_assoc_blocks_i32(None, None, None, None, 4, 4, 1, 1, 8, None) == INVALID   # no pointers
    assert lib.pcr_assoc_blocks_i32(None, None, None, None, 0, 0, 2, 1, 8, None) == 0         # nothing to do


@pytest.mark.parametrize("R_,C_", [(7, 7), (5, 12), (12, 5), (1, 1)])
def test_one_block_is_the_full_solve(R_, C_):
    for cost in (A.integer_case(R_, C_, 4, seed=R_ + C_), A.reference_case(R_, C_, seed=3)[0][:R_, :C_]):
        want = A.lsa(cost)
        got = B.lsa_blocks(cost, np.zeros(R_, np.int32), np.zeros(C_, np.int32), 1)
        for a, b in zip(want[:4], got[:4]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert got[4].tolist() == [want[4]]


def test_restated_rule_edges():
    cost = A.integer_case(6, 7, 5, seed=1)
    cost[0, 6] = np.nan                                   # row 0 is in block 0, column 6 in none: never read
    rb, cb = np.array([0, 1, 0, -1, 1, 2], np.int32), np.array([1, 0, 0, 1, 3, 0, 5], np.int32)
    c4r, r4c, u, v, info = B.lsa_blocks(cost, rb, cb, 3)
    assert info.tolist() == [0, 0, 0]
    assert c4r[3] == -1 and c4r[5] == -1 and r4c[4] == -1 and r4c[6] == -1 and u[3] == 0 and v[6] == 0
    sub = A.lsa(cost[np.ix_([0, 2], [1, 2, 5])])
    assert c4r[[0, 2]].tolist() == np.array([1, 2, 5])[sub[0]].tolist()
    cost[2, 2] = np.inf                                   # inside block 0: that block alone fails
    c4r2, r4c2, _, _, info2 = B.lsa_blocks(cost, rb, cb, 3)
    assert info2.tolist() == [1, 0, 0] and c4r2[[0, 2]].tolist() == [-1, -1] and r4c2[[1, 2, 5]].tolist() == [-1, -1, -1]
    assert c4r2[[1, 4]].tolist() == c4r[[1, 4]].tolist()


def test_block_ids():
    rb, cb, G = B.block_ids([0, 5, -1, 2], [2, 8, 0], 4, 3, 2, 1, num_classes=3)
    assert G == 4
    assert rb.tolist() == [0, 3, 3, 2] + [2, 3, 0] * 2 and cb.tolist() == [2, 3, 0] + [0, 3, 3, 2]


@pytest.mark.parametrize("T,D", SIZES)
@pytest.mark.parametrize("dd,td,reduce", EQUAL + EQUAL_BUT_VOIDS)
def test_margin_frames_decode_equal(T, D, dd, td, reduce):
    for seed in SEEDS:
        full, blocks = both_routes(T, D, dd, td, reduce, "margin", seed)
        assert_same_frame(full, blocks, (dd, td, reduce) in EQUAL, "T=%d D=%d (%d, %d) reduce=%s seed %d"
                          % (T, D, dd, td, reduce, seed))
        assert blocks["info"][1] <= full["info"][1]


@pytest.mark.parametrize("T,D", SIZES)
@pytest.mark.parametrize("dd,td", [(1, 1), (2, 0), (2, 1)])
def test_softmax_frames_decode_equal(T, D, dd, td):
    for seed in SEEDS:
        full, blocks = both_routes(T, D, dd, td, False, "softmax", seed)
        assert_same_frame(full, blocks, True, "softmax T=%d D=%d (%d, %d) seed %d" % (T, D, dd, td, seed))


def test_blocks_need_fewer_search_steps():
    """what the route is for: at T = 70, D = 33 the longest block's searches are a fraction of the full problem's"""
    tl, dl, logits, pairs, count, det_dec, trk_dec = scene(70, 33, 1, 1, 0)
    cost = R.cost_multi(logits, pairs, count, 70, 33, det_dec, trk_dec, dd=1, td=1)
    rb, cb, G = B.block_ids(tl, dl, 70, 33, 1, 1, CLASSES)
    assert B.lsa_blocks(cost, rb, cb, G, count_steps=True)[5].max() < A.lsa(cost, count_steps=True)[5]
