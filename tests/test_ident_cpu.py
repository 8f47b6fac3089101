"""CPU: the numpy restatement of the identity metrics (tests/ident_ref.py, include/pcr.h section A9) against scipy's totals
(tests/golden/ident_lsa.npz, written by tools/make_ident_golden.py), a brute force and hand-worked scenes; the new entry
points' ABI and the binding's refusals."""
import itertools
import math

import numpy as np
import pytest
import torch

import ident_ref as R
import truth_ref as TRU


# ---- 1. the assignment's total -----------------------------------------------------------------------------------------------
def test_restatement_idtp_equals_scipy_on_every_golden_case(golden):
    gold = golden("ident_lsa")
    cases = R.golden_cases()
    assert [n for n, _ in cases] == gold["names"].tolist() and len(cases) == len(R.GOLDEN_SHAPES) * len(R.GOLDEN_KINDS)
    shapes, empty_rows, tied = set(), 0, 0
    for i, (name, cooc) in enumerate(cases):
        assert cooc.dtype == np.int32 and (cooc == gold["cooc_%d" % i]).all() and cooc.min() >= 0, name
        # exactness: every solver value is an integer below 2^24 (include/pcr.h), so ties cannot cost anything
        assert (min(cooc.shape) + 1) * int(cooc.max()) < 1 << 24
        assert R.idtp_of(cooc) == int(gold["total_%d" % i]), name
        shapes.add(cooc.shape)
        empty_rows += int((cooc.sum(axis=1) == 0).any() and (cooc.sum(axis=0) == 0).any())
        tied += int(name.startswith("ties"))
    assert (256, 512) in shapes and (65, 33) in shapes and empty_rows >= 8 and tied == len(R.GOLDEN_SHAPES)


def brute_force(m):
    R_, C_ = m.shape
    if R_ > C_:
        m, R_, C_ = m.T, C_, R_
    return max(sum(int(m[r, c]) for r, c in enumerate(cols)) for cols in itertools.permutations(range(C_), R_))


def test_restatement_idtp_equals_a_brute_force_up_to_4_by_4():
    """every shape up to 4 x 4: ALL matrices over {0, 1, 2} where there are at most 3^6 of them, and 40 random ones with
    heavy ties (counts 0 .. 3) and 10 with large counts for every shape"""
    g = np.random.default_rng(5)
    seen = 0
    for r, c in itertools.product(range(1, 5), repeat=2):
        mats = []
        if r * c <= 6:
            mats += [np.array(v, np.int32).reshape(r, c) for v in itertools.product(range(3), repeat=r * c)]
        mats += [g.integers(0, 4, (r, c)).astype(np.int32) for _ in range(40)]
        mats += [g.integers(0, 100000, (r, c)).astype(np.int32) for _ in range(10)]
        for m in mats:
            assert R.idtp_of(m) == brute_force(m), m
            seen += 1
    assert seen == 1776 + 16 * 50


# ---- 2. hand-worked scenes ---------------------------------------------------------------------------------------------------
def run_scene(frames, gt_rows, id_cap, gt_cap, C=4):
    """frames of (det_labels, det_gt, det_id, gt_labels, gt_ids) through the identity restatement and the MOT record of
    tests/truth_ref.py -> (scene, MOT stats)"""
    scene, book = R.new_scene(gt_rows, id_cap), TRU.new_book(C, gt_cap)
    for det_labels, det_gt, det_id, gt_labels, gt_ids in frames:
        a = lambda v: np.asarray(v, np.int32)
        D, G = len(det_labels), len(gt_labels)
        cost = np.full((D, G), 0.5, np.float32)
        book = TRU.record(book, np.full(C, -1, np.int32), np.full(C, -1, np.int32), a(det_gt), np.full(D, -1, np.int32), a(det_id),
                          a(gt_labels), a(gt_ids), np.zeros(G, np.int32), gt_cap, a(det_labels))
        scene = R.record(scene, a(det_labels), a(det_gt), a(det_id), a(gt_labels), a(gt_ids), cost, gt_cap)
    return scene, book["stats"]


def product_metrics(pool, fp=0):
    """the figures by the PRODUCT's host arithmetic (pcr_amd.identity.metrics_of is pure host code) over a pooled table"""
    from pcr_amd import identity as ID
    return ID.metrics_of(pool["table"].tolist(), float(pool["dist_total"][0]), int(fp))


def test_two_tracks_that_swap_identities_half_way():
    """two ground-truth tracks of 10 frames; the tracker's ids 10 and 11 swap at frame 5: each track shares 5 frames with
    either id, so the best global assignment keeps 5 + 5 = 10 of 20"""
    frames = [([0, 0], [0, 1], [10, 11] if f < 5 else [11, 10], [0, 0], [0, 1]) for f in range(10)]
    scene, stats = run_scene(frames, gt_rows=2, id_cap=16, gt_cap=2)
    assert scene["cooc"][:, 10:12].tolist() == [[5, 5], [5, 5]] and scene["cooc"].sum() == 20
    pool, id_map, idtp, comp = R.close_scene(scene, R.new_pool(), 4, 4)
    m = product_metrics(pool, fp=stats[TRU.FP])
    assert (m["idtp"], m["gt_total"], m["pred_total"], m["idfn"], m["idfp"]) == (10, 20, 20, 10, 10)
    assert m["idf1"] == 0.5 and m["idp"] == 0.5 and m["idr"] == 0.5
    assert (m["frag"], m["mt"], m["pt"], m["ml"], m["tracks"]) == (0, 2, 0, 0, 2)
    assert (m["tid"], m["lgd"], m["faf"], m["frames"]) == (0.0, 0.0, 0.0, 10) and m["motp"] == 0.5
    assert (m["overflow"], m["inexact"], m["dropped_gt"], m["dropped_id"]) == (0, 0, 0, 0)
    assert sorted(id_map.tolist()) == [10, 11]
    assert stats[TRU.SWITCHES] == 2 and stats[TRU.TP] == 20          # MOTA sees two events, whatever follows them


def test_one_track_seen_on_and_off():
    """T T - - T - T: two fragments, a longest gap of two frames, tracked from its first frame.  A gap is a frame without a
    true positive (frames 2 and 5) or with an untracked one (frame 3); frame 4 also carries the id on a second box"""
    on, off, untracked = ([0], [0], [7], [0], [3]), ([-1], [-1], [-1], [0], [3]), ([0], [0], [-1], [0], [3])
    twice = ([0], [1], [7], [0, 0], [3, 3])
    scene, _ = run_scene([on, on, off, untracked, twice, off, on], gt_rows=5, id_cap=8, gt_cap=5)
    row = scene["gt_track"][3]
    assert (row[R.FRAGS], row[R.LONGEST_GAP], row[R.FIRST_GAP], row[R.PRESENT], row[R.TRACKED]) == (2, 2, 0, 7, 4)
    assert scene["cooc"][3, 7] == 4 and scene["cooc"].sum() == 4 and (scene["gt_track"][[0, 1, 2, 4]] == 0).all()
    assert scene["totals"][:4].tolist() == [7, 8, 4, 5]       # frames, boxes, tracked detections, true positives
    pool, id_map, idtp, _ = R.close_scene(scene, R.new_pool(), 2, 2)
    m = product_metrics(pool)
    assert (m["idtp"], m["pt"], m["mt"], m["ml"], m["frag"], m["lgd"], m["tid"]) == (4, 1, 0, 0, 2, 2.0, 0.0)
    assert id_map.tolist() == [-1, -1, -1, 7, -1]
    # a track that is found late and one that never is: TID counts the frames before the first tracked one / all of them
    late = [off, off, on, on, on, on, on, on, on, on, on, on]
    scene, _ = run_scene(late, gt_rows=5, id_cap=8, gt_cap=5)
    assert scene["gt_track"][3].tolist() == [12, 10, 0, 2, 2, 0, 1, 1]
    scene = R.record(scene, *(np.asarray(v, np.int32) for v in ([-1], [-1], [-1], [0], [4])), np.zeros((1, 1), np.float32), 5)
    pool, _, _, _ = R.close_scene(scene, R.new_pool(), 2, 2)
    m = product_metrics(pool)
    assert (m["mt"], m["ml"], m["tracks"], m["tid"], m["lgd"]) == (1, 1, 2, 1.5, 1.5) and m["motp"] == 0.5       # every match costs 0.5


def test_flags_and_pooling_of_the_restatement():
    cooc = np.zeros((9, 40), np.int32)
    cooc[[1, 3, 8], [2, 30, 39]] = (4, 5, 6)
    scene = R.new_scene(9, 40)
    scene["cooc"] = cooc
    pool, id_map, idtp, comp = R.close_scene(scene, R.new_pool(), 3, 3)
    assert idtp == 15 and comp["row_list"].tolist() == [1, 3, 8] and comp["col_list"].tolist() == [2, 30, 39]
    pool, id_map, idtp, comp = R.close_scene(scene, pool, 2, 3)       # one row too many
    assert idtp == 0 and (id_map == -1).all() and (comp["cost"] == 0).all() and comp["counts"][:2].tolist() == [3, 3]
    assert pool["table"][R.IX["overflow"]] == 1 and pool["table"][R.IX["idtp"]] == 15
    scene["cooc"] = cooc * (1 << 22)
    pool, _, idtp, _ = R.close_scene(scene, pool, 3, 3)
    assert pool["table"][R.IX["inexact"]] == 1 and idtp == 15 << 22
    m = product_metrics(pool)
    assert (m["idtp"], m["overflow"], m["inexact"]) == (15 + (15 << 22), 1, 1) and m["tracks"] == 0
    m = product_metrics(R.new_pool())                        # nothing was seen: every ratio lacks its denominator
    assert all(math.isnan(m[k]) for k in ("idf1", "idp", "idr", "tid", "lgd", "motp", "faf"))
    assert all(m[k] == 0 for k in m if not isinstance(m[k], float))


def test_metrics_of_on_a_hand_written_table():
    """the product's host arithmetic on figures that are all different: 6 of 10 ground-truth boxes and of 8 predictions keep
    their identity; 4 tracks waited 6 frames in all for their first tracked frame and had longest gaps of 10 in all; 8 true
    positives lie 2.0 m off in all; 3 false detections in 12 frames"""
    from pcr_amd import identity as ID
    t = dict(idtp=6, frames=12, gt_total=10, pred_total=8, tp=8, tracks=4, mt=1, pt=2, ml=1, frag=5, tid_sum=6, lgd_sum=10,
             overflow=0, inexact=1, dropped_gt=2, dropped_id=3)
    assert ID.TABLE == R.TABLE and sorted(t) == sorted(ID.TABLE)
    m = ID.metrics_of([t[k] for k in ID.TABLE], 2.0, fp=3)
    assert (m["idtp"], m["idfn"], m["idfp"]) == (6, 4, 2)
    assert (m["idp"], m["idr"], m["idf1"]) == (0.75, 0.6, 12 / 18)
    assert (m["mt"], m["pt"], m["ml"], m["tracks"], m["frag"]) == (1, 2, 1, 4, 5)
    assert (m["tid"], m["lgd"], m["motp"], m["faf"]) == (1.5, 2.5, 0.25, 0.25)
    assert (m["frames"], m["gt_total"], m["pred_total"], m["tp"]) == (12, 10, 8, 8)
    assert (m["overflow"], m["inexact"], m["dropped_gt"], m["dropped_id"]) == (0, 1, 2, 3)
    want = R.metrics([t[k] for k in R.TABLE], 2.0, fp=3)     # the restatement's copy of the formulas says the same
    assert m == want
    # predictions without ground truth: precision 0, recall undefined, F1 0
    t.update(idtp=0, gt_total=0, tp=0, tracks=0, tid_sum=0, lgd_sum=0, mt=0, pt=0, ml=0)
    m = ID.metrics_of([t[k] for k in ID.TABLE], 0.0, fp=8)
    assert m["idp"] == 0.0 and math.isnan(m["idr"]) and m["idf1"] == 0.0 and m["idfp"] == 8 and math.isnan(m["motp"])
    assert math.isnan(m["tid"]) and math.isnan(m["lgd"]) and m["faf"] == 8 / 12


# ---- 3. the ABI and the binding's refusals -------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_the_abi_version_stays():
    from pcr_amd import _lib as L
    from pcr_amd import abi
    lib = L.load()
    assert lib.pcr_abi_version() == 17 == L.ABI_VERSION
    for name in ("pcr_ident_ok", "pcr_ident_record_i32", "pcr_ident_compact_f32", "pcr_ident_score_i32"):
        assert name in abi.SIGNATURES and getattr(lib, name) is not None


def test_ident_ok_ranges():
    from pcr_amd import identity as ID
    ok = dict(D=100, G=120, gt_cap=500, gt_rows=300, id_cap=4096, max_rows=256, max_cols=512)
    assert ID.ident_ok(**ok)
    assert ID.ident_ok(0, 0, 1, 1, 1, 1, 1) and ID.ident_ok(1024, 1024, 65536, 65536, 1024, 1024, 1024)
    assert ID.ident_ok(0, 0, 1, 1024, 65536) and ID.ident_ok(0, 0, 1, 8192, 8192)
    for k, bad in (("D", (-1, 1025)), ("G", (-1, 1025)), ("gt_cap", (0, 65537)), ("gt_rows", (0, 65537)), ("id_cap", (0, 65537)),
                   ("max_rows", (0, 1025)), ("max_cols", (0, 1025))):
        for v in bad:
            assert not ID.ident_ok(**dict(ok, **{k: v})), (k, v)
    assert not ID.ident_ok(0, 0, 1, 1025, 65536) and not ID.ident_ok(0, 0, 1, 8193, 8192)       # gt_rows * id_cap > 2^26


def test_cpu_tensors_and_wrong_dtypes_raise():
    from pcr_amd import _lib as L
    from pcr_amd import identity as ID
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    t = dict(det_labels=i32(4), det_gt=i32(4), det_id=i32(4), gt_labels=i32(3), gt_ids=i32(3), cost=torch.zeros(4, 3),
             cooc=i32(5, 6), gt_track=i32(5, 8), totals=i32(8), dist_sum=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(L.PcrError, match="no CPU"):
        ID.record(t, 5, 5, 6)
    for k, bad in (("det_id", torch.zeros(4, dtype=torch.int64)), ("cost", torch.zeros(4, 3, dtype=torch.float64)),
                   ("dist_sum", torch.zeros(1)), ("cooc", torch.zeros(5, 6, dtype=torch.int64))):
        with pytest.raises(L.PcrError, match="%s must be a" % k):
            ID.record(dict(t, **{k: bad}), 5, 5, 6)
    with pytest.raises(L.PcrError, match="hold 30 elements"):
        ID.record(dict(t, cooc=i32(5, 5)), 5, 5, 6)
    with pytest.raises(L.PcrError, match="out of range"):
        ID.record(t, 5, 0, 6)
    c = dict(cooc=i32(5, 6), flags=i32(11), counts=i32(4), row_list=i32(2), col_list=i32(3), cost=torch.zeros(2, 3))
    with pytest.raises(L.PcrError, match="no CPU"):
        ID.compact(c, 5, 6, 2, 3)
    with pytest.raises(L.PcrError, match="flags is missing"):
        ID.compact({k: v for k, v in c.items() if k != "flags"}, 5, 6, 2, 3)
    s = dict(cooc=i32(5, 6), gt_track=i32(5, 8), totals=i32(8), dist_sum=torch.zeros(1, dtype=torch.float64), counts=i32(4),
             row_list=i32(2), col_list=i32(3), col4row=i32(2), info=i32(1), id_map=i32(5),
             table=torch.zeros(16, dtype=torch.int64), dist_total=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(L.PcrError, match="no CPU"):
        ID.score(s, 5, 6, 2, 3)
    with pytest.raises(L.PcrError, match="table must be a"):
        ID.score(dict(s, table=i32(16)), 5, 6, 2, 3)
    with pytest.raises(L.PcrError, match="TruthBook"):
        ID.IdentityBook(object(), 16)
