"""CPU: the association entry points exist and refuse what they must (no launch without a GPU), and the numpy restatement
the GPU tests compare against (tests/assoc_ref.py) obeys the rules include/pcr.h states: it is checked against the
answers scipy.optimize.linear_sum_assignment -- the reference's solver -- gave for the matrices of
tests/golden/assoc_lsa.npz (tools/make_assoc_golden.py; no test imports scipy)."""
import ctypes
import os
import re

import numpy as np
import pytest

import assoc_ref as R
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("pcr_assoc_pairs_ok", "pcr_assoc_pairs_i32", "pcr_assoc_cost_f32", "pcr_lsa_ok", "pcr_lsa_f32")
INVALID = 1
F = ctypes.c_float


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "assoc_lsa.npz"))
    out = [dict(cost=z["cost_%d" % i], rows=z["rows_%d" % i], cols=z["cols_%d" % i], kind=int(z["kind"][i]),
                total=float(z["total"][i]), solved=R.lsa(z["cost_%d" % i])) for i in range(len(z["kind"]))]
    assert sum(c["kind"] == 0 for c in out) >= 24 and sum(c["kind"] == 1 for c in out) >= 6
    return out


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_abi_is_17(lib):
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
    assert lib.pcr_abi_version() == 17


def test_ok_ranges(lib):
    lsa_max, objs, ncls = header_int("PCR_LSA_MAX"), header_int("PCR_ASSOC_MAX_OBJECTS"), header_int("PCR_ASSOC_MAX_CLASSES")
    assert lsa_max == 1024 and objs >= 4096 and ncls == 32
    ok = lib.pcr_lsa_ok
    assert ok(1, lsa_max, lsa_max) == 1 and ok(65535, 1, lsa_max) == 1 and ok(0, 0, 0) == 1 and ok(3, 0, 5) == 1
    assert ok(1, lsa_max + 1, 4) == 0 and ok(1, 4, lsa_max + 1) == 0 and ok(65536, 4, 4) == 0
    assert ok(-1, 4, 4) == 0 and ok(1, -1, 4) == 0 and ok(1, 4, -1) == 0
    ok = lib.pcr_assoc_pairs_ok
    assert ok(objs, objs, ncls, objs * objs) == 1 and ok(0, 0, 1, 0) == 1 and ok(200, 200, 8, 40000) == 1
    assert ok(5, 7, 8, 1000) == 1                                      # cap may exceed T * D: the rest is padding
    assert ok(objs + 1, 1, 8, 1) == 0 and ok(1, objs + 1, 8, 1) == 0 and ok(-1, 1, 8, 1) == 0 and ok(1, -1, 8, 1) == 0
    assert ok(4, 4, 0, 16) == 0 and ok(4, 4, ncls + 1, 16) == 0 and ok(4, 4, 8, -1) == 0
    assert ok(4, 4, 8, objs * objs + 1) == 0


def test_null_and_out_of_range_arguments_return_invalid(lib):
    fbuf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    p, i = ctypes.cast(fbuf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    # (host pointers: each call below must be refused before anything is launched)
    pairs = lib.pcr_assoc_pairs_i32
    assert pairs(None, None, None, None, None, None, 4, 4, 8, 2, 16, None) == INVALID
    assert pairs(None, i, None, None, i, i, 4, 4, 8, 2, 16, None) == INVALID            # track labels
    assert pairs(i, None, None, None, i, i, 4, 4, 8, 2, 16, None) == INVALID            # detection labels
    assert pairs(i, i, None, None, None, i, 4, 4, 8, 2, 16, None) == INVALID            # pairs
    assert pairs(i, i, None, None, i, None, 4, 4, 8, 2, 16, None) == INVALID            # count
    assert pairs(i, i, None, None, i, i, 4, 4, 33, 2, 16, None) == INVALID              # num_classes
    assert pairs(i, i, None, None, i, i, 4, 4, 8, 2, -1, None) == INVALID               # cap
    assert pairs(i, i, None, None, i, i, 4097, 4, 8, 2, 16, None) == INVALID            # T
    assert pairs(i, i, None, None, i, i, 4, -1, 8, 2, 16, None) == INVALID              # D
    cost = lib.pcr_assoc_cost_f32
    assert cost(None, None, None, None, None, None, F(22), F(3), F(1e4), None, 2, 3, 6, None) == INVALID
    assert cost(p, i, i, None, None, None, F(22), F(3), F(1e4), None, 2, 3, 6, None) == INVALID      # cost
    assert cost(None, i, i, None, None, None, F(22), F(3), F(1e4), p, 2, 3, 6, None) == INVALID      # logits
    assert cost(p, None, i, None, None, None, F(22), F(3), F(1e4), p, 2, 3, 6, None) == INVALID      # pairs
    assert cost(p, i, None, None, None, None, F(22), F(3), F(1e4), p, 2, 3, 6, None) == INVALID      # count
    assert cost(p, i, i, None, None, None, F(22), F(3), F(1e4), p, -1, 3, 6, None) == INVALID        # T
    assert cost(p, i, i, None, None, None, F(22), F(3), F(1e4), p, 2, 4097, 6, None) == INVALID      # D
    assert cost(p, i, i, None, None, None, F(22), F(3), F(1e4), p, 2, 3, -1, None) == INVALID        # cap
    lsa = lib.pcr_lsa_f32
    assert lsa(None, None, None, None, None, None, 1, 4, 4, None) == INVALID
    assert lsa(None, i, i, None, None, i, 1, 4, 4, None) == INVALID                     # cost
    assert lsa(p, None, i, None, None, i, 1, 4, 4, None) == INVALID                     # col4row
    assert lsa(p, i, None, None, None, i, 1, 4, 4, None) == INVALID                     # row4col
    assert lsa(p, i, i, None, None, None, 1, 4, 4, None) == INVALID                     # info
    assert lsa(p, i, i, None, None, i, 1, 1025, 4, None) == INVALID
    assert lsa(p, i, i, None, None, i, 1, 4, 1025, None) == INVALID
    assert lsa(p, i, i, None, None, i, 65536, 4, 4, None) == INVALID
    assert lsa(p, i, i, None, None, i, 1, -1, 4, None) == INVALID
    # nothing to do is not an error and launches nothing
    assert pairs(None, None, None, None, None, None, 0, 4, 8, 2, 0, None) == 0
    assert pairs(None, None, None, None, None, None, 4, 0, 8, 2, 16, None) == 0
    assert cost(None, None, None, None, None, None, F(22), F(3), F(1e4), None, 0, 0, 0, None) == 0
    assert lsa(None, None, None, None, None, None, 0, 4, 4, None) == 0
    assert lsa(None, None, None, None, None, None, 2, 0, 4, None) == 0
    assert lsa(None, None, None, None, None, None, 2, 4, 0, None) == 0


def test_host_tensors_raise_from_every_entry_point():
    import torch
    from pcr_amd import associate as A
    from pcr_amd._lib import PcrError
    labels = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(PcrError):
        A.compare_pairs(labels, labels)
    with pytest.raises(PcrError):
        A.association_cost(torch.zeros(9), torch.zeros((9, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 3, 3)
    with pytest.raises(PcrError):
        A.linear_assignment(torch.zeros(4, 4))
    import bench
    model, _ = bench.build_pt_model([128, 64, 32], device="cpu")
    feats, xyz = torch.zeros(3, 32, 32), torch.zeros(3, 32, 3)
    with pytest.raises(PcrError):
        model.associate(feats, xyz, labels, None, feats, xyz, labels, None)


# ---- 2. the restatement against scipy's recorded answers ---------------------------------------------------------------
def _chosen(cost, col4row):
    rows = np.nonzero(col4row >= 0)[0]
    return rows, col4row[rows]


def test_every_fixture_case_is_a_valid_assignment_no_worse_than_scipy(cases):
    for n, c in enumerate(cases):
        cost = c["cost"]
        R_, C_ = cost.shape
        col4row, row4col, u, v, info = c["solved"]
        assert info == 0
        rows, cols = _chosen(cost, col4row)
        assert len(rows) == min(R_, C_) and len(set(cols.tolist())) == len(cols), "case %d: not a permutation" % n
        assert np.array_equal(row4col[cols], rows) and (row4col >= 0).sum() == len(rows)
        total = cost.astype(np.float64)[rows, cols].sum()
        assert total <= c["total"] + 1e-9 * max(1.0, abs(c["total"])), "case %d: total %r above scipy's %r" % (n, total, c["total"])
        if c["kind"] == 0:
            assert (cost.astype(np.float64) - u[:, None] - v[None, :]).min() >= -1e-3, "case %d: duals infeasible" % n


def test_float_cases_equal_scipy_exactly(cases):
    for n, c in enumerate(cases):
        if c["kind"] != 0:
            continue
        want = np.full(c["cost"].shape[0], -1, np.int32)
        want[c["rows"]] = c["cols"]
        assert np.array_equal(c["solved"][0], want), "float case %d differs from scipy's assignment" % n
        rows, cols = _chosen(c["cost"], c["solved"][0])
        assert not (c["cost"][rows, cols] == 10000.0).any(), "float case %d chose a fill entry" % n


def test_integer_cases_have_scipys_total_exactly(cases):
    for n, c in enumerate(cases):
        if c["kind"] != 1:
            continue
        rows, cols = _chosen(c["cost"], c["solved"][0])
        assert c["cost"].astype(np.float64)[rows, cols].sum() == c["total"], "integer case %d" % n


def test_restatement_reports_non_finite_problems():
    c = np.zeros((3, 4), np.float32)
    for badv in (np.nan, np.inf, -np.inf):
        c2 = c.copy()
        c2[1, 2] = badv
        col4row, row4col, u, v, info = R.lsa(c2)
        assert info == 1 and (col4row == -1).all() and (row4col == -1).all()
    assert R.lsa(c)[4] == 0 and R.lsa(c)[0].tolist() == [0, 1, 2]        # ties go to the lowest column


# ---- 3. the pair list and the matrix layout ---------------------------------------------------------------------------
def _pairs_by_rule(tl, dl, tn, dn, min_points, num_classes):
    """the rule of pcr.h, evaluated literally: a triple loop in the stated order"""
    out = []
    for x in range(num_classes):
        for t in range(len(tl)):
            for d in range(len(dl)):
                if tl[t] == x and dl[d] == x and (tn is None or tn[t] >= min_points) and (dn is None or dn[d] >= min_points):
                    out.append((t, d))
    return out


def test_pair_list_membership_and_order():
    tl = [2, 0, 9, 2, 5, 0, 8, -1, 2]          # 9 and 8 are >= num_classes, -1 is below; class 5 has no detection
    dl = [0, 2, 2, 7, 0, 3, 2]                 # classes 7 and 3 have no track
    tn = [2, 1, 5, 0, 9, 2, 4, 4, 3]
    dn = [2, 2, 0, 9, 1, 5, 100]
    for lengths in (False, True):
        for ncls in (8, 3):
            a, b = (tn, dn) if lengths else (None, None)
            want = _pairs_by_rule(tl, dl, a, b, 2, ncls)
            pairs, count = R.compare_pairs(tl, dl, a, b, min_points=2, num_classes=ncls)
            assert count == len(want) and pairs.shape == (len(tl) * len(dl), 2) and pairs.dtype == np.int32
            assert [tuple(p) for p in pairs[:count].tolist()] == want
            assert not pairs[count:].any()
            small, count2 = R.compare_pairs(tl, dl, a, b, num_classes=ncls, cap=3)
            assert count2 == count and [tuple(p) for p in small.tolist()] == want[:3]
    want = _pairs_by_rule(tl, dl, tn, dn, 2, 8)
    assert want == [(5, 0), (0, 1), (0, 6), (8, 1), (8, 6)]           # written out once by hand
    pairs, count = R.compare_pairs([], dl)                              # T = 0
    assert count == 0 and pairs.shape == (0, 2)
    pairs, count = R.compare_pairs([], dl, cap=4)
    assert count == 0 and pairs.shape == (4, 2) and not pairs.any()


def test_cost_matrix_blocks_on_a_hand_made_example():
    T, D, f = 2, 3, 10000.0
    pairs = np.array([[0, 1], [1, 0], [1, 2], [0, 0], [0, 0], [0, 0]], np.int32)          # three listed, three padding
    logits = np.array([1.5, -2.0, 0.25, 99.0, 99.0, 99.0], np.float32)
    miss, new = np.array([0.5, -0.5], np.float32), np.array([1.0, 2.0, 3.0], np.float32)
    dist = np.array([[0.0, 30.0, 30.0], [22.0, 0.0, 22.5]], np.float32)
    cost = R.association_cost(logits, pairs, 3, T, D, miss, new, dist=dist)
    want = np.array([[f, 1.5, f, 0.5, f],                 # (0,1): -1.5 + 3 (30 m > 22 m)
                     [2.0, f, 2.75, f, -0.5],             # (1,0): 22 m is not > 22 m; (1,2): -0.25 + 3
                     [1.0, f, f, f, 2.0],
                     [f, 2.0, f, 1.5, f],
                     [f, f, 3.0, f, 2.75]], np.float32)
    assert cost.dtype == np.float32 and np.array_equal(cost, want)
    assert np.array_equal(cost[T:, D:], cost[:T, :D].T)
    plain = R.association_cost(logits, pairs, 3, T, D)
    assert plain[0, 1] == -1.5 and plain[1, 2] == -0.25 and (np.diag(plain[:T, D:]) == 0).all() and (np.diag(plain[T:, :D]) == 0).all()
    # a count above the capacity lists the capacity
    assert np.array_equal(R.association_cost(logits[:2], pairs[:2], 3, T, D)[:T, :D], [[f, -1.5, f], [2.0, f, f]])


def test_planted_permutation_is_recovered():
    T, D = 5, 8
    g = np.random.default_rng(0)
    det_of_track = g.permutation(D)[:T]
    labels_t, labels_d = np.zeros(T, np.int64), np.zeros(D, np.int64)
    pairs, count = R.compare_pairs(labels_t, labels_d)
    assert count == T * D
    logits = np.where(det_of_track[pairs[:, 0]] == pairs[:, 1], 8.0, -8.0).astype(np.float32)
    cost = R.association_cost(logits, pairs, count, T, D)
    col4row, row4col, u, v, info = R.lsa(cost)
    t2d, d2t = R.decode(col4row, row4col, T, D)
    assert info == 0 and np.array_equal(t2d, det_of_track)
    extras = np.setdiff1d(np.arange(D), det_of_track)
    assert (d2t[extras] == -1).all() and np.array_equal(d2t[det_of_track], np.arange(T))
