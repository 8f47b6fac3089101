"""CPU: association with any set of decisions (include/pcr.h section A3, "Any set of decisions").  The numpy restatement
the GPU tests compare against (tests/decisions_ref.py) is held against what the reference's own associators computed for
the cases of tests/golden/assoc_decisions.npz (tools/make_decisions_golden.py; no test imports scipy or the reference);
the new entry points exist, are declared in pcr_amd/abi.py and refuse what they must without a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import assoc_ref as A
import decisions_ref as R
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("pcr_assoc_multi_ok", "pcr_assoc_multi_ws_bytes", "pcr_assoc_cost_multi_f32", "pcr_assoc_decode_i32")
INVALID = 1
FILL = 10000.0


def softmax_f32_bound(c):
    """The golden softmax matrices are torch's float32 softmax, the restatement's float64 rounded once.  What float32 can
    lose on p = exp(x - m) / sum <= 1, in units of 2^-24 relative to p (an absolute bound since p <= 1): the rounding of
    x - m, |x - m| <= spread of the scores, which exp turns into a relative error of spread * 2^-24; exp itself and the
    division, 3 units together; a sum of n positive terms in any order, at most n units; the final rounding, 1."""
    scores = np.concatenate([c["sup"].ravel(), c["det"].ravel(), c["trk"].ravel()])
    spread = float(scores.max() - scores.min())
    n = max(c["T"] + c["dd"], c["D"] + c["td"])
    return (spread + n + 4) * 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "assoc_decisions.npz"))
    out = []
    for i in range(len(z["T"])):
        c = {k: int(z[k][i]) for k in ("T", "D", "dd", "td", "kind", "reduce")}
        for k in ("sup", "det", "trk", "cost", "det_decision", "track_decision", "track_to_det", "det_choice", "trk_choice"):
            if "%s_%d" % (k, i) in z.files:
                c[k] = z["%s_%d" % (k, i)]
        out.append(c)
    configs = {(c["dd"], c["td"], c["kind"]) for c in out if not c["reduce"]}
    assert configs == {(dd, td, k) for dd, td in ((2, 0), (2, 1), (1, 2), (2, 2), (1, 1), (0, 1), (3, 1)) for k in (0, 1)}
    assert sum(c["reduce"] for c in out) >= 50 and sum((c["T"], c["D"]) == (70, 40) for c in out) >= 10
    return out


def listed(c):
    """the golden's supervise['cost_mat'] as the entry point's inputs: margin -> the entries that are not 10000 are the
    listed pairs (row-major, as the class gate lists them) and logits = -cost; softmax -> every pair, logits = the scores"""
    sup = c["sup"]
    t, d = np.nonzero(sup != np.float32(FILL)) if c["kind"] == 0 else np.nonzero(np.ones_like(sup, bool))
    pairs = np.stack([t, d], axis=1).astype(np.int32)
    logits = -sup[t, d] if c["kind"] == 0 else sup[t, d]
    return logits.astype(np.float32), pairs, len(pairs)


def restated(c):
    logits, pairs, count = listed(c)
    return R.cost_multi(logits, pairs, count, c["T"], c["D"], c["det"], c["trk"], dd=c["dd"], td=c["td"],
                        kind=("margin", "softmax")[c["kind"]], reduce=bool(c["reduce"]), fill=FILL)


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_abi_is_17(lib):
    from pcr_amd import abi
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
        assert s in abi.SIGNATURES
    assert lib.pcr_abi_version() == 17
    assert header_int("PCR_ASSOC_MAX_DECISIONS") == 4
    assert set(abi.BLOCKS) >= {"pcr_assoc_multi", "pcr_assoc_decode"}


def test_multi_ok_edges(lib):
    ok, lsa_max, md = lib.pcr_assoc_multi_ok, header_int("PCR_LSA_MAX"), header_int("PCR_ASSOC_MAX_DECISIONS")
    assert ok(0, 0, 0, 0, 0) == 1 and ok(0, 5, 2, 0, 0) == 1 and ok(5, 0, 0, 2, 0) == 1
    assert ok(-1, 5, 1, 1, 0) == 0 and ok(5, -1, 1, 1, 0) == 0
    assert ok(4, 4, md, md, 16) == 1 and ok(4, 4, md + 1, 1, 16) == 0 and ok(4, 4, 1, md + 1, 16) == 0
    assert ok(4, 4, -1, 1, 16) == 0 and ok(4, 4, 1, -1, 16) == 0
    assert ok(4, 4, 1, 1, 16) == 1 and ok(4, 4, 1, 1, 17) == 0 and ok(4, 4, 1, 1, -1) == 0        # 0 <= cap <= T * D
    assert ok(lsa_max, 0, 4, 0, 0) == 1 and ok(lsa_max + 1, 0, 0, 0, 0) == 0
    assert ok(512, 256, 2, 1, 0) == 1 and ok(512, 256, 2, 2, 0) == 0 and ok(512, 257, 2, 1, 0) == 0   # T + dd*D, D + td*T
    assert ok(200, 100, 2, 1, 20000) == 1 and ok(40, 30, 2, 0, 1200) == 1
    ws = lib.pcr_assoc_multi_ws_bytes
    assert ws(0, 0, 0, 0) == 0 and ws(5, 7, 2, 1) >= 4 * 5 * 7 and ws(4, 4, md + 1, 0) == 0


def test_entries_refuse_without_a_launch(lib):
    from pcr_amd import abi
    assert lib.pcr_assoc_cost_multi_f32(None, None) == INVALID and lib.pcr_assoc_decode_i32(None, None) == INVALID
    p = abi.AssocMultiParams()
    p.T, p.D, p.dd, p.td, p.cap = 4, 4, 5, 0, 0
    assert lib.pcr_assoc_cost_multi_f32(ctypes.byref(p), None) == INVALID            # beyond PCR_ASSOC_MAX_DECISIONS
    p.dd, p.kind = 1, 2
    assert lib.pcr_assoc_cost_multi_f32(ctypes.byref(p), None) == INVALID            # no such kind
    p.kind, p.reduce = 1, 1
    assert lib.pcr_assoc_cost_multi_f32(ctypes.byref(p), None) == INVALID            # softmax with reduce
    p.reduce, p.dist = 0, 64
    assert lib.pcr_assoc_cost_multi_f32(ctypes.byref(p), None) == INVALID            # softmax with a distance prior
    p.dist = None
    assert lib.pcr_assoc_cost_multi_f32(ctypes.byref(p), None) == INVALID            # no cost pointer
    p.T, p.D, p.dd = 0, 0, 0
    assert lib.pcr_assoc_cost_multi_f32(ctypes.byref(p), None) == 0                  # nothing to do
    q = abi.AssocDecodeParams()
    q.born_dec = q.kill_dec = -1
    assert lib.pcr_assoc_decode_i32(ctypes.byref(q), None) == 0                      # T + D == 0: nothing to do
    q.T, q.D, q.dd, q.td = 3, 3, 1, 1
    assert lib.pcr_assoc_decode_i32(ctypes.byref(q), None) == INVALID                # no pointers
    q.born_dec = 1
    assert lib.pcr_assoc_decode_i32(ctypes.byref(q), None) == INVALID                # born_dec must be below dd


def test_python_argument_errors_come_before_any_launch():
    import torch
    from pcr_amd import associate
    from pcr_amd._lib import PcrError
    z, p, c = torch.zeros(4), torch.zeros((4, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(PcrError, match="softmax kind takes no distance prior"):
        associate.association_cost_multi(z, p, c, 2, 2, kind="softmax", dist=torch.zeros(2, 2))
    with pytest.raises(PcrError, match="reduce goes with the margin kind"):
        associate.association_cost_multi(z, p, c, 2, 2, kind="softmax", reduce=True)
    with pytest.raises(PcrError, match="kind must be"):
        associate.association_cost_multi(z, p, c, 2, 2, kind="sigmoid")
    with pytest.raises(PcrError):                                                    # no CPU fallback
        associate.association_cost_multi(z, p, c, 2, 2)
    assert associate.multi_shape(5, 3, 2, 1) == (11, 8) and associate.multi_shape(5, 3, 2, 0, reduce=True) == (8, 3)


# ---- 2. the matrices against the reference's own ----------------------------------------------------------------------
def test_margin_and_reduce_matrices_equal_the_reference_bit_for_bit(cases):
    n = 0
    for c in cases:
        if c["kind"] != 0:
            continue
        got = restated(c)
        if c["reduce"]:
            got, det_choice, trk_choice = got
            if c["dd"]:
                assert np.array_equal(det_choice, c["det_choice"])
            if c["td"]:
                assert np.array_equal(trk_choice, c["trk_choice"])
        assert got.dtype == np.float32 and got.shape == c["cost"].shape
        assert np.array_equal(got.view(np.uint32), c["cost"].view(np.uint32)), (c["T"], c["D"], c["dd"], c["td"], c["reduce"])
        n += 1
    assert n >= 150


def test_margin_with_one_decision_per_side_is_association_cost(cases):
    for seed, (T, D) in enumerate(((1, 1), (5, 3), (9, 17))):
        logits, pairs, count, det, trk = R.random_case(T, D, 1, 1, seed)
        dist = np.random.default_rng(seed).random((T, D)).astype(np.float32) * 40
        a = A.association_cost(logits, pairs, count, T, D, trk[0], det[0], dist=dist)
        b = R.cost_multi(logits, pairs, count, T, D, det, trk, dist=dist)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_softmax_matrix_is_within_tolerance_of_the_reference(cases):
    n, worst = 0, 0.0
    for c in cases:
        if c["kind"] != 1:
            continue
        got = restated(c)
        assert got.shape == c["cost"].shape
        assert np.array_equal(got == np.float32(FILL), c["cost"] == np.float32(FILL))
        dev = float(np.abs(got.astype(np.float64) - c["cost"].astype(np.float64)).max())
        bound = softmax_f32_bound(c)
        worst = max(worst, dev / bound)
        assert dev <= bound, (c["T"], c["D"], c["dd"], c["td"], dev, bound)
        n += 1
    print("softmax: the float64 restatement deviates from the golden by at most %.3f of the float32 bound" % worst)
    assert n >= 80


def test_softmax_leaves_gated_pairs_out():
    """pcr.h's deliberate difference: an unlisted pair takes part in neither softmax and stays at fill"""
    logits = np.array([1.0, 2.0, 0.5], np.float32)
    pairs = np.array([[0, 0], [0, 1], [1, 1]], np.int32)                             # (1, 0) is gated out
    det, trk = np.array([[0.25, -1.0]], np.float32), np.array([[0.0, 3.0]], np.float32)
    cost = R.cost_multi(logits, pairs, 3, 2, 2, det, trk, kind="softmax")
    assert cost.shape == (4, 4) and cost[1, 0] == np.float32(FILL) and cost[2, 3] == np.float32(FILL)     # and its transpose
    e = np.exp
    p_row0 = e(1.0) / (e(1.0) + e(2.0) + e(0.0))
    p_col0 = e(1.0) / (e(1.0) + e(0.25))                                             # (1, 0) is not in column 0's sum
    assert abs(cost[0, 0] + max(p_row0, p_col0)) < 1e-7 and cost[2, 2] == cost[0, 0]
    assert abs(cost[2, 0] + e(0.25) / (e(1.0) + e(0.25))) < 1e-7
    assert abs(cost[1, 3] + e(3.0) / (e(0.5) + e(3.0))) < 1e-7


# ---- 3. the decode against the reference's decision lists --------------------------------------------------------------
def test_decoded_decisions_equal_the_reference_on_every_case(cases):
    n = repaired = 0
    for c in cases:
        if c["reduce"]:
            continue
        cost = c["cost"]                                 # the reference's own matrix: no tolerance enters the decisions
        col4row, row4col, _, _, info = A.lsa(cost)
        out = R.decode(cost, col4row, row4col, c["T"], c["D"], c["dd"], c["td"], fill=FILL, solver_info=info)
        key = (c["T"], c["D"], c["dd"], c["td"], c["kind"])
        assert out["info"][0] == 0 and out["info"][1] == 0, key
        assert np.array_equal(out["det_decision"], c["det_decision"]), key
        assert np.array_equal(out["track_decision"], c["track_decision"]), key
        assert np.array_equal(out["track_to_det"], c["track_to_det"]), key
        d2t = np.full(c["D"], -1, np.int32)
        m = c["track_to_det"] >= 0
        d2t[c["track_to_det"][m]] = np.flatnonzero(m)
        assert np.array_equal(out["det_to_track"], d2t), key
        repaired += int(out["info"][2] + out["info"][3] > 0)
        n += 1
    assert n >= 200 and repaired >= 5, (n, repaired)


def test_masks_and_unmatched_code():
    logits, pairs, count, det, trk = R.random_case(6, 9, 2, 0, 3)
    cost = R.cost_multi(logits, pairs, count, 6, 9, det, trk)
    col4row, row4col, _, _, info = A.lsa(cost)
    out = R.decode(cost, col4row, row4col, 6, 9, 2, 0, born_dec=1, kill_dec=-1, solver_info=info)
    assert np.array_equal(out["born"], (out["det_decision"] == 2).astype(np.int32)) and out["born"].sum() > 0
    assert not out["kill"].any() and set(out["track_decision"]) <= {0, 1}            # td = 0: matched or unmatched (1 + 0)
    lists = R.decision_lists(out, ["det_false_positive", "det_newborn"], [])
    assert sorted(np.concatenate([lists[k] for k in lists if k.startswith("det")]).tolist()) == list(range(9))
    none = R.decode(cost, col4row, row4col, 6, 9, 2, 0, born_dec=1, solver_info=1)   # the solver refused: nothing is assigned
    assert (none["track_to_det"] == -1).all() and (none["det_decision"] == 3).all() and not none["born"].any()
    assert none["info"].tolist() == [1, 0, 0, 0]


def test_sequential_repair_on_a_collision():
    """two forgotten tracks whose cheapest free column is the same detection: the reference's simultaneous pick hands it to
    both (:171-181); here track 0 takes it and track 1 goes on to its next free column"""
    T, D, dd, td, f = 2, 1, 2, 1, np.float32(FILL)
    cost = np.full((T + dd * D, D + td * T), f, np.float32)
    cost[0, 0], cost[1, 0] = -5.0, -4.0                  # both tracks like detection 0 best
    cost[0, 1], cost[1, 2] = 1.0, 2.0                    # their own tracking decision
    cost[2, 0], cost[3, 0] = 0.5, 0.7                    # the detection's two decisions
    cost[2, 1], cost[2, 2], cost[3, 1], cost[3, 2] = -5.0, -4.0, -5.0, -4.0
    col4row = np.array([-1, -1, 1, 2], np.int32)         # an assignment that lives in the bottom right only
    row4col = np.array([-1, 2, 3], np.int32)
    out = R.decode(cost, col4row, row4col, T, D, dd, td)
    assert out["track_to_det"].tolist() == [0, -1] and out["det_to_track"].tolist() == [0]
    assert out["track_decision"].tolist() == [0, 1] and out["det_decision"].tolist() == [0]
    assert out["info"].tolist() == [0, 0, 2, 0]


def test_a_detection_without_a_row_stays_unmatched():
    """dd = 0 and more detections than tracks: the reference gives the leftover detection track 0 again and exits; here
    its least free value is fill (there is no free row), so it is 'unmatched'"""
    T, D = 1, 2
    cost = np.array([[-1.0, -2.0, 0.5]], np.float32)
    out = R.decode(cost, np.array([1], np.int32), np.array([-1, 0, -1], np.int32), T, D, 0, 1)
    assert out["track_to_det"].tolist() == [1] and out["det_decision"].tolist() == [1, 0] and out["info"].tolist() == [0, 0, 0, 0]


def test_void_assignment_is_dropped_and_counted():
    """the only column left for track 1 holds fill: the reference prints and exits, here the pair is void (info[1]) and,
    with a tracking decision present, the track is repaired from what is free"""
    f = np.float32(FILL)
    cost = np.array([[-3.0, f], [-2.0, f]], np.float32)                              # dd = td = 0: (T, D) = (2, 2)
    col4row, row4col, _, _, info = A.lsa(cost)
    assert col4row.tolist() == [0, 1]
    out = R.decode(cost, col4row, row4col, 2, 2, 0, 0, solver_info=info)
    assert out["track_to_det"].tolist() == [0, -1] and out["det_to_track"].tolist() == [0, -1]
    assert out["track_decision"].tolist() == [0, 1] and out["det_decision"].tolist() == [0, 1]
    assert out["info"].tolist() == [0, 1, 0, 0]
    cost = np.array([[-3.0, f, 0.25, f], [f, f, f, f]], np.float32)                  # td = 1; track 1 has nothing but fill
    col4row, row4col, _, _, info = A.lsa(cost)
    out = R.decode(cost, col4row, row4col, 2, 2, 0, 1, solver_info=info)
    assert out["info"].tolist() == [0, 1, 0, 0]                                      # void, and the repair skips a fill minimum
    assert out["track_to_det"].tolist() == [0, -1] and out["track_decision"].tolist() == [0, 2]
    assert out["det_decision"].tolist() == [0, 1]
