"""CPU: the section-A5 entry points (track state) exist and refuse what they must, and the numpy restatement the GPU
tests compare against (tests/track_ref.py, the array form) is right: over scripted frames it keeps the same books as a
list form written the way the reference's tracker keeps them, and its float32 propagation and distance stay within a
derived bound of the same formulas in float64."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_ref as R
from conftest import ROOT

NEW_SYMBOLS = ("pcr_bank_ok", "pcr_bank_plan_i32", "pcr_bank_move_f32", "pcr_bank_dist_f32", "pcr_bank_retire_i32")
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
    from pcr_amd import abi, build
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
        assert re.search(r"\b%s\s*\(" % s, header), "include/pcr.h does not declare %s" % s
        assert s in abi.SIGNATURES
    assert lib.pcr_abi_version() == 17
    assert "pcr_bank" in abi.BLOCKS
    assert build.FLAGS["track_kernels.hip"] == ["-ffp-contract=off"]


def test_bank_ok_ranges(lib):
    top, row = header_int("PCR_ASSOC_MAX_OBJECTS"), header_int("PCR_BANK_MAX_ROW")
    ok = lib.pcr_bank_ok
    assert ok(1, 0, 9, 0, 0) == 1 and ok(top, top, 7, row, row) == 1 and ok(40, 12, 9, 64 * 128, 128 * 3) == 1
    assert ok(0, 4, 9, 8, 3) == 0 and ok(top + 1, 4, 9, 8, 3) == 0 and ok(-1, 4, 9, 8, 3) == 0          # C
    assert ok(4, -1, 9, 8, 3) == 0 and ok(4, top + 1, 9, 8, 3) == 0                                      # D
    for W in (-1, 0, 5, 6, 8, 10):
        assert ok(4, 4, W, 8, 3) == 0
    assert ok(4, 4, 7, -1, 3) == 0 and ok(4, 4, 7, row + 1, 3) == 0                                      # feat_floats
    assert ok(4, 4, 7, 8, -1) == 0 and ok(4, 4, 7, 8, row + 1) == 0                                      # xyz_floats


def host_bank(C=4, D=3, W=9):
    """a pcr_bank over HOST arrays: every call that gets one must be refused before anything is launched"""
    from pcr_amd import abi
    keep = []

    def buf(ct, n):
        a = (ct * max(n, 1))()
        keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p).value
    p = abi.BankParams()
    p.C, p.D, p.W, p.frame_limit, p.replace_all, p.reset_on_match, p.propagate = C, D, W, 10, 0, 0, 1
    for k in ("lengths", "labels", "ids", "steps", "misses", "track_to_det", "kill", "src"):
        setattr(p, k, buf(ctypes.c_int, C))
    for k in ("next_id", "info"):
        setattr(p, k, buf(ctypes.c_int, 1))
    p.boxes, p.scores = buf(ctypes.c_float, C * W), buf(ctypes.c_float, C)
    for k in ("det_to_track", "det_labels", "det_lengths", "born", "det_slot", "det_id"):
        setattr(p, k, buf(ctypes.c_int, D))
    p.det_boxes, p.det_scores, p.carry = buf(ctypes.c_float, D * W), buf(ctypes.c_float, D), buf(ctypes.c_float, 12)
    return p, keep


def test_plan_refuses_null_and_out_of_range_arguments(lib):
    plan = lib.pcr_bank_plan_i32
    assert plan(None, None) == INVALID
    required = ("lengths", "boxes", "scores", "labels", "ids", "steps", "misses", "next_id", "info", "track_to_det",
                "det_to_track", "det_labels", "det_lengths", "det_boxes", "det_scores", "src", "det_slot", "det_id")
    for k in required:
        p, keep = host_bank()
        setattr(p, k, None)
        assert plan(ctypes.byref(p), None) == INVALID, "NULL %s" % k
    top = header_int("PCR_ASSOC_MAX_OBJECTS")
    for field, bad in (("C", 0), ("C", -1), ("C", top + 1), ("D", -1), ("D", top + 1), ("W", 8), ("W", 0),
                       ("frame_limit", 0), ("frame_limit", -2)):
        p, keep = host_bank()
        setattr(p, field, bad)
        assert plan(ctypes.byref(p), None) == INVALID, (field, bad)


def test_move_dist_retire_refuse_null_and_out_of_range_arguments_and_empty_work_is_ok(lib):
    fbuf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
    p, i = ctypes.cast(fbuf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    top, row = header_int("PCR_ASSOC_MAX_OBJECTS"), header_int("PCR_BANK_MAX_ROW")
    move, dist, retire = lib.pcr_bank_move_f32, lib.pcr_bank_dist_f32, lib.pcr_bank_retire_i32
    good = [i, p, p, p, p]
    for k in range(len(good)):
        args = list(good)
        args[k] = None
        assert move(*args, 4, 3, 4, 3, None) == INVALID, "NULL argument %d" % k
    for shape in ((0, 3, 4, 3), (top + 1, 3, 4, 3), (4, -1, 4, 3), (4, top + 1, 4, 3), (4, 3, -1, 3), (4, 3, row + 1, 3),
                  (4, 3, 4, -1), (4, 3, 4, row + 1)):
        assert move(*good, *shape, None) == INVALID, shape
    assert move(*([None] * 5), 4, 0, 4, 3, None) == 0 and move(*([None] * 5), 4, 3, 0, 0, None) == 0      # nothing to do
    good = [p, i, p, p, p]
    for k in (0, 1, 2, 4):                                                     # (carry_inv may be NULL: identity)
        args = list(good)
        args[k] = None
        assert dist(*args, 4, 3, 9, None) == INVALID, "NULL argument %d" % k
    for shape in ((0, 3, 9), (top + 1, 3, 9), (4, -1, 9), (4, top + 1, 9), (4, 3, 8), (4, 3, 0)):
        assert dist(*good, *shape, None) == INVALID, shape
    assert dist(*([None] * 5), 4, 0, 9, None) == 0                             # nothing to do
    good = [i, i, i, i]
    for k in range(len(good)):
        args = list(good)
        args[k] = None
        assert retire(*args, 4, None) == INVALID, "NULL argument %d" % k
    assert retire(*good, 0, None) == INVALID and retire(*good, top + 1, None) == INVALID and retire(*good, -1, None) == INVALID


def test_host_tensors_raise_from_every_function():
    import torch
    from pcr_amd import tracks as T
    from pcr_amd._lib import PcrError
    C, D, W = 4, 3, 9
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    st = dict(lengths=i32(C), boxes=torch.zeros(C, W), scores=torch.zeros(C), labels=i32(C), ids=i32(C), steps=i32(C),
              misses=i32(C), next_id=i32(1), info=i32(1))
    calls = (lambda: T.plan(st, i32(C), i32(D), i32(D), i32(D), torch.zeros(D, W), torch.zeros(D), i32(C), i32(D), i32(D)),
             lambda: T.move(i32(C), torch.zeros(D, 3, 5), torch.zeros(D, 5, 3), torch.zeros(C, 3, 5), torch.zeros(C, 5, 3)),
             lambda: T.distances(torch.zeros(C, W), i32(C), torch.zeros(D, W)),
             lambda: T.retire(i32(C), i32(C), i32(C), i32(C)),
             lambda: T.TrackBank(C, D, device="cpu"))
    for call in calls:
        with pytest.raises(PcrError):
            call()


# ---- 2. the array form against the list form ------------------------------------------------------------------------------
FRAMES, LIMIT = 12, 3


@pytest.mark.parametrize("reset_on_match", [False, True])
def test_array_form_keeps_the_books_of_the_list_form(reset_on_match):
    g = np.random.default_rng(5)
    C, D, W = 96, 8, 9
    st = R.new_state(C, W)
    feats, xyz = np.zeros((C, 3, 5), np.float32), np.zeros((C, 5, 3), np.float32)
    lt = R.ListTracker()
    absorbed = {}                                            # (a)'s side of "the detections a track absorbed"
    seen = dict(equal=0, longer=0, died_at_limit=0, match_after_miss=0, killed=0, propagated=0)
    for f in range(FRAMES):
        fr = R.make_frame(g, st, D, W, masks=f % 2 == 0)
        det = dict(labels=fr["labels"], lengths=fr["lengths"], boxes=fr["boxes"], scores=fr["scores"],
                   feats=g.standard_normal((D, 3, 5)).astype(np.float32), xyz=g.standard_normal((D, 5, 3)).astype(np.float32))
        carry = R.rigid(g)[0] if f % 3 else None
        args = dict(carry=carry, frame_limit=LIMIT, reset_on_match=reset_on_match, propagate=f % 4 != 3)
        # what the frame exercises, read off the state before it
        kill = fr["kill"] if fr["kill"] is not None else np.zeros(C, np.int32)
        for s, d in fr["intended"]:
            if not kill[s]:
                seen["equal"] += st["lengths"][s] == fr["lengths"][d]
                seen["longer"] += st["lengths"][s] > fr["lengths"][d]
                seen["match_after_miss"] += st["misses"][s] > 0
        held = {s for s, _ in fr["intended"]}
        for s in np.nonzero(st["ids"] >= 0)[0]:
            seen["killed"] += bool(kill[s])
            if s not in held and not kill[s]:
                seen["died_at_limit"] += st["misses"][s] + 1 == LIMIT
        ids_before = st["ids"].copy()
        new, src, det_slot, det_id = R.plan_frame(st, fr, **args)
        feats, xyz = R.move(src, det["feats"], det["xyz"], feats, xyz)
        seen["propagated"] += int(((new["steps"] == st["steps"] + 1) & (new["misses"] == st["misses"] + 1)).sum())
        st = new
        assert st["info"][0] == 0                            # the bank is large enough: nothing is dropped
        want_id = lt.step(f, [(int(ids_before[s]), d) for s, d in fr["intended"]],
                          [int(ids_before[s]) for s in np.nonzero((ids_before >= 0) & (kill != 0))[0]], det, born=fr["born"],
                          **args)
        assert np.array_equal(det_id, want_id)
        for d in np.nonzero(det_id >= 0)[0]:
            absorbed.setdefault(int(det_id[d]), []).append((f, int(d)))
            assert st["ids"][det_slot[d]] == det_id[d]
        live_a = {int(st["ids"][s]): int(s) for s in np.nonzero(st["ids"] >= 0)[0]}
        live_b = lt.live()
        assert sorted(live_a) == sorted(live_b) and len(live_a) == (st["ids"] >= 0).sum()      # one to one
        for tid, s in live_a.items():
            t, i = lt.tracks[live_b[tid]], live_b[tid]
            assert absorbed[tid] == t["absorbed"]
            assert feats[s].tobytes() == lt.feats[i].tobytes() and xyz[s].tobytes() == lt.xyz[i].tobytes()
            assert st["lengths"][s] == lt.lengths[i]
            assert st["boxes"][s].tobytes() == t["boxes"][-1].tobytes()
            assert np.float32(st["scores"][s]).tobytes() == np.float32(t["scores"][-1]).tobytes()
            assert st["labels"][s] == t["cls"][-1]
            assert st["steps"][s] == len(t["boxes"]) and st["misses"][s] == t["misses"]
        free = st["ids"] < 0
        assert (st["labels"][free] == -1).all() and (st["lengths"][free] == 0).all()
    assert st["next_id"][0] == lt.count and lt.count >= FRAMES
    for k, v in seen.items():
        assert v >= 2, "the script never exercised %r" % k


def test_plan_ignores_what_it_must_and_reports_dropped_births():
    g = np.random.default_rng(11)
    st = R.random_state(g, 70, 9)
    fr = R.make_frame(g, st, 67, 9)
    new, src, det_slot, det_id = R.plan_frame(st, fr, frame_limit=3)
    matched = {d: s for s, d in fr["intended"] if not fr["kill"][s]}
    for d in range(67):
        if d in matched:
            assert det_slot[d] == matched[d] and det_id[d] == st["ids"][matched[d]]
        elif det_slot[d] >= 0:                              # born: into a slot that was free, with a fresh id
            assert st["ids"][det_slot[d]] < 0 and det_id[d] >= st["next_id"][0] and fr["born"][d] and fr["labels"][d] >= 0
    n_free = int((st["ids"] < 0).sum())
    wanted = sum(1 for d in range(67) if fr["labels"][d] >= 0 and d not in matched and fr["born"][d])
    assert wanted > n_free > 0                               # the case has fewer free slots than births
    assert new["info"][0] == wanted - n_free and new["next_id"][0] == st["next_id"][0] + n_free
    born_slots = sorted(det_slot[d] for d in range(67) if d not in matched and det_slot[d] >= 0)
    assert born_slots == sorted(np.nonzero(st["ids"] < 0)[0].tolist())
    # slots freed in this launch are not reused by it
    freed = (st["ids"] >= 0) & (new["ids"] < 0)
    assert freed.any() and not np.isin(np.nonzero(freed)[0], det_slot).any()


# ---- 3. float32 against float64 ---------------------------------------------------------------------------------------------
def test_float32_propagation_and_distance_against_float64():
    """Inputs within 100 m in every coordinate and translation, rigid rotations.  A propagated coordinate is at most six
    roundings of partial sums <= 400 (half an ulp of 400 is 1.5e-5 -- the bound allows ten times that, 1.5e-4, for each);
    a distance takes two such coordinates and adds the square root's half ulp at <= 600 m (3e-5): within 1e-3 m."""
    g = np.random.default_rng(3)
    worst_p = worst_d = 0.0
    for trial in range(20):
        carry, carry_inv = R.rigid(g)
        boxes = R.det_boxes(g, 70, 9)
        dets = R.det_boxes(g, 67, 9)
        M = carry.astype(np.float64).reshape(3, 4)
        for b in boxes:
            got = R.propagate_box(b, carry)
            c = np.array([b[0] + np.float64(b[7]) / 2, b[1] + np.float64(b[8]) / 2, b[2], 1.0], np.float64)
            worst_p = max(worst_p, np.abs(got[:3].astype(np.float64) - M @ c).max())
            assert got[3:].tobytes() == b[3:].tobytes()      # size, yaw and velocity stay
        ids = np.zeros(70, np.int32)
        got = R.dist(boxes, ids, dets, carry_inv).astype(np.float64)
        Mi = carry_inv.astype(np.float64).reshape(3, 4)
        prev = np.concatenate([dets[:, :3].astype(np.float64), np.ones((67, 1))], 1) @ Mi.T
        want = np.hypot(boxes[:, None, 0].astype(np.float64) - prev[None, :, 0], boxes[:, None, 1].astype(np.float64) - prev[None, :, 1])
        worst_d = max(worst_d, np.abs(got - want).max())
    print("float32 vs float64: propagation %.3g m, distance %.3g m" % (worst_p, worst_d))
    assert worst_p <= 1e-3 and worst_d <= 1e-3
    assert (R.dist(boxes, np.full(70, -1, np.int32), dets, carry_inv) == 0).all()          # a free slot's row is 0
