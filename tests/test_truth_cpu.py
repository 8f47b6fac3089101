"""CPU: the section-A7 entry points (ground truth) exist and refuse what they must, and the numpy restatement the GPU
tests compare against (tests/truth_ref.py, the array form) is right: over scripted scenes it keeps the same books as a
list form written the way the reference's tracker keeps them, and the thresholded outcome of its cost with
assoc_ref.lsa is the one scipy gives (tests/golden/truth_lsa.npz, written by tools/make_truth_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_ref as TR
import truth_ref as R
from conftest import ROOT

NEW_SYMBOLS = ("pcr_truth_ok", "pcr_truth_cost_f32", "pcr_truth_decide_i32", "pcr_truth_record_i32")
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


# ---- 1. symbols and arguments ---------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_abi_is_17(lib):
    from pcr_amd import abi, build, truth
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
        assert re.search(r"\b%s\s*\(" % s, header), "include/pcr.h does not declare %s" % s
        assert s in abi.SIGNATURES
    assert lib.pcr_abi_version() == 17
    assert "pcr_truth" in abi.BLOCKS
    assert build.FLAGS["truth_kernels.hip"] == ["-ffp-contract=off"]
    # the table's layout, once in the header and once on each side of the binding
    for name, i in (("TOTAL_GT", 15), ("TOTAL_CORRECT", 16), ("FRAMES", 17), ("GT_TOTAL", 18), ("TP", 19), ("FP", 20), ("FN", 21),
                    ("SWITCHES", 22), ("UNTRACKED", 23), ("STATS", 24)):
        assert header_int("PCR_TRUTH_" + name) == i == getattr(R, name)
    assert truth.STATS == R.STATS and truth.MOT == R.MOT and truth.KINDS == R.KINDS
    assert (truth.TOTAL_GT, truth.TOTAL_CORRECT) == (R.TOTAL_GT, R.TOTAL_CORRECT)
    for k, name in enumerate(("DET_MATCH", "DET_NEWBORN", "DET_FP", "TRACK_FN", "TRACK_FP")):
        assert header_int("PCR_TRUTH_" + name) == k


def test_truth_ok_ranges(lib):
    top, lsa, ids = header_int("PCR_ASSOC_MAX_OBJECTS"), header_int("PCR_LSA_MAX"), header_int("PCR_TRUTH_MAX_IDS")
    ok = lib.pcr_truth_ok
    assert ids == 65536
    assert ok(1, 0, 0, 9, 1) == 1 and ok(top, lsa, lsa, 7, ids) == 1 and ok(200, 100, 100, 9, 500) == 1
    assert ok(0, 4, 4, 9, 8) == 0 and ok(-1, 4, 4, 9, 8) == 0 and ok(top + 1, 4, 4, 9, 8) == 0          # C
    assert ok(4, -1, 4, 9, 8) == 0 and ok(4, lsa + 1, 4, 9, 8) == 0                                      # D
    assert ok(4, 4, -1, 9, 8) == 0 and ok(4, 4, lsa + 1, 9, 8) == 0                                      # G
    for W in (-1, 0, 5, 6, 8, 10):
        assert ok(4, 4, 4, W, 8) == 0
    assert ok(4, 4, 4, 9, 0) == 0 and ok(4, 4, 4, 9, -3) == 0 and ok(4, 4, 4, 9, ids + 1) == 0           # gt_cap


def host_block(C=4, D=3, G=2, gt_cap=8):
    """a pcr_truth over HOST arrays: every call that gets one must be refused before anything is launched"""
    from pcr_amd import abi
    keep = []

    def buf(ct, n):
        a = (ct * max(n, 1))()
        keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p).value
    p = abi.TruthParams()
    p.C, p.D, p.G, p.gt_cap, p.skip_empty = C, D, G, gt_cap, 1
    sizes = dict(ids=C, slot_gt=C, slot_tte=C, gt_last=gt_cap, stats=R.STATS, col4row=D, row4col=G, info=1, gt_labels=G,
                 gt_ids=G, gt_tte=G, det_labels=D, track_to_det=C, det_to_track=D, born=D, kill=C, det_gt=D, true_t2d=C,
                 true_d2t=D, det_truth=D, track_truth=C, det_slot=D, det_id=D)
    for k, n in sizes.items():
        setattr(p, k, buf(ctypes.c_int, n))
    p.cost, p.thresh = buf(ctypes.c_float, D * G), buf(ctypes.c_float, 1)
    return p, keep


DECIDE_NEEDS = ("ids", "slot_gt", "slot_tte", "stats", "col4row", "row4col", "info", "cost", "thresh", "gt_labels", "gt_ids",
                "gt_tte", "det_labels", "track_to_det", "det_to_track", "det_gt", "true_t2d", "true_d2t", "det_truth",
                "track_truth")
RECORD_NEEDS = ("ids", "slot_gt", "slot_tte", "gt_last", "stats", "gt_labels", "gt_ids", "gt_tte", "det_labels", "det_gt",
                "track_truth", "det_slot", "det_id")


def test_decide_and_record_refuse_null_and_out_of_range_arguments(lib):
    top, lsa, ids = header_int("PCR_ASSOC_MAX_OBJECTS"), header_int("PCR_LSA_MAX"), header_int("PCR_TRUTH_MAX_IDS")
    for fn, needs in ((lib.pcr_truth_decide_i32, DECIDE_NEEDS), (lib.pcr_truth_record_i32, RECORD_NEEDS)):
        assert fn(None, None) == INVALID
        for k in needs:
            p, keep = host_block()
            setattr(p, k, None)
            assert fn(ctypes.byref(p), None) == INVALID, "NULL %s" % k
        for field, bad in (("C", 0), ("C", -1), ("C", top + 1), ("D", -1), ("D", lsa + 1), ("G", -1), ("G", lsa + 1),
                           ("gt_cap", 0), ("gt_cap", ids + 1)):
            p, keep = host_block()
            setattr(p, field, bad)
            assert fn(ctypes.byref(p), None) == INVALID, (field, bad)


def test_cost_refuses_null_and_out_of_range_arguments_and_empty_work_is_ok(lib):
    fbuf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    p, i = ctypes.cast(fbuf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    lsa, ids = header_int("PCR_LSA_MAX"), header_int("PCR_TRUTH_MAX_IDS")
    cost = lib.pcr_truth_cost_f32
    good = [p, i, p, i, i, p, p]
    for k in (1, 3, 4, 6):                                                     # labels, ids and the output, whatever the kind
        args = list(good)
        args[k] = None
        assert cost(*args, 3, 2, 9, 8, None) == INVALID, "NULL argument %d" % k
    for k in (0, 2):                                                           # without an IoU the boxes are read
        args = list(good)
        args[k], args[5] = None, None
        assert cost(*args, 3, 2, 9, 8, None) == INVALID, "NULL argument %d" % k
    for shape in ((-1, 2, 9, 8), (lsa + 1, 2, 9, 8), (3, -1, 9, 8), (3, lsa + 1, 9, 8), (3, 2, 8, 8), (3, 2, 0, 8), (3, 2, 9, 0),
                  (3, 2, 9, ids + 1)):
        assert cost(*good, *shape, None) == INVALID, shape
    assert cost(*([None] * 7), 0, 2, 9, 8, None) == 0 and cost(*([None] * 7), 3, 0, 7, 8, None) == 0     # nothing to do


def test_host_tensors_raise_from_every_function():
    import torch
    from pcr_amd import truth as T
    from pcr_amd._lib import PcrError
    C, D, G = 4, 3, 2
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    t = dict(ids=i32(C), slot_gt=i32(C), slot_tte=i32(C), gt_last=i32(8), stats=i32(R.STATS), col4row=i32(D), row4col=i32(G),
             info=i32(1), cost=torch.zeros(D, G), thresh=torch.zeros(1), gt_labels=i32(G), gt_ids=i32(G), gt_tte=i32(G),
             det_labels=i32(D), track_to_det=i32(C), det_to_track=i32(D), det_gt=i32(D), true_t2d=i32(C), true_d2t=i32(D),
             det_truth=i32(D), track_truth=i32(C), det_slot=i32(D), det_id=i32(D))
    calls = (lambda: T.cost(torch.zeros(D, 9), i32(D), torch.zeros(G, 9), i32(G), i32(G), 8),
             lambda: T.decide(t, 8), lambda: T.record(t, 8), lambda: T.TruthBook(None, 4, 8))
    for call in calls:
        with pytest.raises(PcrError):
            call()


# ---- 2. the array form against the list form ------------------------------------------------------------------------------
FRAMES, LIMIT = 14, 3


@pytest.mark.parametrize("seed", [3, 4])
def test_array_form_keeps_the_books_of_the_list_form(seed):
    C, D, G, W = 26, 12, 12, 9
    sc = R.Scene(n_obj=14, frames=FRAMES, D=D, G=G, W=W, seed=seed)
    g = np.random.default_rng(100 + seed)
    st, book, lt = TR.new_state(C, W), R.new_book(C, sc.gt_cap), R.ListTruth()
    used = np.zeros(C, bool)
    seen = dict(births=0, gt_ends=0, missed_objects=0, false_detections=0, duplicate_ids=0, reused_slots=0, deaths=0,
                switches=0, skipped_kinds=0)
    alive_before = set()
    for f in range(FRAMES):
        fr = sc.frame(f)
        dl, gl, gi, gtte = fr["det_labels"], fr["gt_labels"], fr["gt_ids"], fr["gt_tte"]
        cost = R.cost(fr["det_boxes"], dl, fr["gt_boxes"], gl, gi, sc.gt_cap)
        col, row, info = R.lsa_maps(cost)
        tr = R.truth(book, st["ids"], col, row, info, cost, sc.thresh, gl, gi, sc.gt_cap, dl)
        assert [(d, int(j)) for d, j in enumerate(tr["det_gt"]) if j >= 0] == fr["pairs"]      # the true positives by construction
        t2d, d2t, born, kill = R.corrupt(g, tr, st["ids"], dl)
        every = R.decide(book, st["ids"], col, row, info, cost, sc.thresh, gl, gi, sc.gt_cap, dl, t2d, d2t, born, kill,
                         skip_empty=False)[0]["stats"]
        book, out = R.decide(book, st["ids"], col, row, info, cost, sc.thresh, gl, gi, sc.gt_cap, dl, t2d, d2t, born, kill,
                             skip_empty=True)
        new, src, det_slot, det_id = TR.plan(st, t2d, d2t, dl, np.full(D, 5, np.int32), fr["det_boxes"], fr["det_scores"],
                                             born=born, kill=kill, frame_limit=LIMIT)
        assert new["info"][0] == 0
        held = book["slot_gt"][(new["ids"] >= 0) & (book["slot_gt"] >= 0)]
        # ---- the list form, over the frame's real detections and ground truth and the active tracks in bank order ----
        slots = np.nonzero(st["ids"] >= 0)[0]
        vd, vg = np.nonzero(dl >= 0)[0], np.nonzero(R.gt_valid(gl, gi, sc.gt_cap))[0]
        cd, cg, cs = {int(d): i for i, d in enumerate(vd)}, {int(j): i for i, j in enumerate(vg)}, {int(s): i for i, s in enumerate(slots)}
        tp_det = np.array([cd[d] for d, _ in fr["pairs"]], np.int64)
        tp_gt = np.array([cg[j] for _, j in fr["pairs"]], np.int64)
        tp = lt.decisions(st["ids"][slots].astype(np.int64), tp_det, tp_gt, gi[vg].astype(np.int64), len(vd))
        assert sorted(zip(slots[tp["pos_track_match"]].tolist(), vd[tp["pos_det_match"]].tolist())) == \
            [(int(s), int(d)) for s, d in enumerate(out["true_t2d"]) if d >= 0] == \
            sorted((int(s), int(d)) for d, s in enumerate(out["true_d2t"]) if s >= 0)
        for key, arr, idx, code in (("pos_det_newborn", out["det_truth"], vd, 1), ("pos_det_false_positive", out["det_truth"], vd, 2),
                                    ("pos_track_false_negative", out["track_truth"], slots, 1),
                                    ("pos_track_false_positive", out["track_truth"], slots, 2)):
            assert idx[tp[key]].tolist() == np.nonzero(arr == code)[0].tolist(), (f, key)
        assert (out["det_truth"][dl < 0] == -1).all() and (out["track_truth"][st["ids"] < 0] == -1).all()
        killed = [s for s in slots if kill[s]]
        matched = [(s, t2d[s]) for s in slots if t2d[s] >= 0 and not kill[s]]
        taken = {d for _, d in matched}
        lt.get_stats(dict(track_match=[cs[s] for s, _ in matched], det_match=[cd[d] for _, d in matched],
                          det_newborn=[cd[d] for d in vd if d not in taken and born[d]],
                          det_false_positive=[cd[d] for d in vd if d not in taken and not born[d]],
                          track_false_positive=[cs[s] for s in killed],
                          track_false_negative=[cs[s] for s in slots if not kill[s] and t2d[s] < 0]), tp)
        for k, name in enumerate(R.KINDS):
            for i, what in enumerate(("_gt", "_correct", "_num_pred")):
                assert book["stats"][3 * k + i] == lt.logging.get(name + what, 0), (f, name, what)
        seen["skipped_kinds"] += int((every[:15] != book["stats"][:15]).any())      # a prediction without a true instance
        assert book["stats"][R.TOTAL_GT] == lt.logging.get("total_gt", 0)
        assert book["stats"][R.TOTAL_CORRECT] == lt.logging.get("total_correct", 0)
        # ---- the frame's end: now and then the track NMS retires the higher of two slots that hold one id ----
        ids_now = new["ids"].copy()
        dup = [s for s in np.nonzero(ids_now >= 0)[0] if det_slot.tolist().count(s) == 0 and book["slot_gt"][s] >= 0 and
               (book["slot_gt"][:s][ids_now[:s] >= 0] == book["slot_gt"][s]).any()]
        if dup and f % 2:
            new = TR.retire(np.isin(np.arange(C), dup[-1:]).astype(np.int32), new)
        switches = book["stats"][R.SWITCHES]
        book = R.record(book, new["ids"], out["track_truth"], out["det_gt"], det_slot, det_id, gl, gi, gtte, sc.gt_cap, dl)
        kept = [int(d) for d in vd if det_id[d] >= 0]
        ck = {d: i for i, d in enumerate(kept)}
        pairs_kept = [(d, j) for d, j in fr["pairs"] if d in ck]
        lt.update_mapping(int(new["next_id"][0]), gtte[vg].astype(np.int64), gi[vg].astype(np.int64),
                          np.array([ck[d] for d, _ in pairs_kept], np.int64), np.array([cg[j] for _, j in pairs_kept], np.int64),
                          det_id[kept].astype(np.int64))
        for s in np.nonzero(new["ids"] >= 0)[0]:
            assert book["slot_gt"][s] == lt.trkid_to_gt[new["ids"][s]], (f, s)
            assert book["slot_tte"][s] == lt.trkid_to_tte[new["ids"][s]], (f, s)
        free = new["ids"] < 0
        assert (book["slot_gt"][free] == -1).all() and (book["slot_tte"][free] == -1).all()
        # ---- what the frame exercised ----
        born_slots = [int(s) for s in det_slot[det_slot >= 0] if st["ids"][s] < 0]
        seen["births"] += len(born_slots)
        seen["reused_slots"] += int(used[born_slots].sum())
        used |= new["ids"] >= 0
        seen["deaths"] += int(((st["ids"] >= 0) & (new["ids"] < 0)).sum())
        alive = set(gi[vg].tolist())
        seen["gt_ends"] += len(alive_before - alive)
        alive_before = alive
        seen["missed_objects"] += len(vg) - len(fr["pairs"])
        seen["false_detections"] += len(vd) - len(fr["pairs"])
        seen["duplicate_ids"] += len(held) - len(set(held.tolist()))
        seen["switches"] += int(book["stats"][R.SWITCHES] - switches)
        st = new
    m = R.metrics(book["stats"])
    assert m["frames"] == FRAMES and m["tp"] + m["fn"] == m["gt_total"] and m["mota"] < 1.0
    for k, v in seen.items():
        assert v >= 1, "the script never exercised %r" % k


def test_record_and_decide_ignore_what_they_must():
    """a frame in mid-sequence with junk: the outputs stay in range and the padding joins nothing"""
    g = np.random.default_rng(9)
    c = R.random_case(g, 70, 67, 66, 9)
    cost = R.cost(c["det_boxes"], c["det_labels"], c["gt_boxes"], c["gt_labels"], c["gt_ids"], c["gt_cap"])
    col, row, info = R.lsa_maps(cost)
    fr, st = c["fr"], c["st"]
    book, out = R.decide(c["book"], st["ids"], col, row, info, cost, 2.0, c["gt_labels"], c["gt_ids"], c["gt_cap"], c["det_labels"],
                         fr["track_to_det"], fr["det_to_track"], fr["born"], fr["kill"])
    ok = R.gt_valid(c["gt_labels"], c["gt_ids"], c["gt_cap"])
    tp = out["det_gt"] >= 0
    assert tp.sum() >= 10 and (~ok).sum() >= 3 and ok[out["det_gt"][tp]].all() and (c["det_labels"][tp] >= 0).all()
    assert (out["true_d2t"] >= 0).sum() == (out["true_t2d"] >= 0).sum() >= 3
    for d in np.nonzero(out["true_d2t"] >= 0)[0]:
        s = out["true_d2t"][d]
        assert out["true_t2d"][s] == d and st["ids"][s] >= 0 and c["book"]["slot_gt"][s] == c["gt_ids"][out["det_gt"][d]]
        assert not ((c["book"]["slot_gt"][:s] == c["book"]["slot_gt"][s]) & (st["ids"][:s] >= 0)).any()      # the lowest holder
    nan = cost.copy()
    nan[3, 4] = np.nan
    col, row, info = R.lsa_maps(nan)
    assert info[0] == 1
    none = R.truth(c["book"], st["ids"], col, row, info, nan, 2.0, c["gt_labels"], c["gt_ids"], c["gt_cap"], c["det_labels"])
    assert (none["det_gt"] == -1).all() and (none["true_t2d"] == -1).all() and set(none["det_truth"].tolist()) <= {-1, 2}


def test_padding_rows_pull_real_pairs_only_while_they_must_take_real_columns():
    """The limit written in the header, and the way round it.  One detection 0.3 m from object A, a missed object B behind
    A as seen from the origin, one padding detection.  With as many columns as rows the padding row must take a real
    column, and leaving it A (10000 + 9.7) with the detection on B (10) is cheaper than the true pair (0.3) with the
    padding row on B (10000 + 20): the true positive is lost.  With max_gt = max_dets + (the valid ground truth) the
    padding row has a padding column at a flat 10000 and the true pair stands."""
    W, gt_cap = 9, 8
    det_boxes, det_labels = np.zeros((2, W), np.float32), np.array([0, -1], np.int32)
    det_boxes[0, 0] = 10.0
    for G, want in ((2, -1), (4, 0)):
        gt_boxes, gt_labels, gt_ids = np.zeros((G, W), np.float32), np.full(G, -1, np.int32), np.full(G, -1, np.int32)
        gt_boxes[0, 0], gt_boxes[1, 0] = 9.7, 20.0
        gt_labels[:2], gt_ids[:2] = 0, (3, 4)
        cost = R.cost(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, gt_cap)
        col, row, info = R.lsa_maps(cost)
        tr = R.truth(R.new_book(1, gt_cap), np.full(1, -1, np.int32), col, row, info, cost, 2.0, gt_labels, gt_ids, gt_cap, det_labels)
        assert tr["det_gt"].tolist() == [want, -1], (G, col.tolist())
        if G == 4:
            assert col[1] >= 2 and cost[1, col[1]] == 10000.0                  # the padding row sits on a padding column


# ---- 3. the thresholded assignment against scipy's ----------------------------------------------------------------------------
def test_thresholded_assignment_equals_scipys():
    z = np.load(os.path.join(ROOT, "tests", "golden", "truth_lsa.npz"))
    cases = R.lsa_cases()
    assert z["names"].tolist() == [name for name, _ in cases] and len(cases) == len(R.LSA_SHAPES) * R.LSA_SEEDS
    n_tp = 0
    for i, (name, c) in enumerate(cases):
        cost = c["cost"]
        assert cost.tobytes() == z["cost_%d" % i].tobytes(), name      # scipy saw this very matrix
        D, G = cost.shape
        want_col = np.full(D, -1, np.int64)
        want_col[z["rows_%d" % i]] = z["cols_%d" % i]
        want = R.thresholded(want_col, cost, c["thresh"])
        col, row, info = R.lsa_maps(cost)
        assert info[0] == 0 and R.thresholded(col, cost, c["thresh"]) == want, name
        # ... and decide's true positives are those pairs, less the ones the validity rules take out (none: a pair below
        # the threshold carries no mask)
        tr = R.truth(R.new_book(1, c["gt_cap"]), np.full(1, -1, np.int32), col, row, info, cost, c["thresh"], c["gt_labels"],
                     c["gt_ids"], c["gt_cap"], c["det_labels"])
        assert [(d, int(j)) for d, j in enumerate(tr["det_gt"]) if j >= 0] == want, name
        # the generator's promise: ground truth of a class >= 6 m apart, a detection within 0.5 m of one or beyond 6 m of all
        gb, db = c["gt_boxes"][:, :2].astype(np.float64), c["det_boxes"][:, :2].astype(np.float64)
        dg = np.hypot(*(gb[:, None] - gb[None]).transpose(2, 0, 1)) + 1e9 * np.eye(G)
        assert dg.min() >= 6.0, name
        dd = np.hypot(*(db[:, None] - gb[None]).transpose(2, 0, 1))
        assert (((dd <= 0.5).sum(1) == 1) | (dd.min(1) > 6.0)).all(), name
        n_tp += len(want)
    assert n_tp >= 300
