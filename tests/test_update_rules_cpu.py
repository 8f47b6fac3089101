"""CPU: the numpy restatement of the updater as configured and of the scene log (tests/update_ref.py, include/pcr.h section
A11) is right.  Driven by the decision lists that the reference's own TrackingUpdater was driven with (tests/golden/
updater_rules.npz, written by tools/make_updater_golden.py) it keeps the reference's active tracks, outputs, unmatched
counts and id numbering frame by frame; three planted faults are each caught by that file; in the two forms
pcr_bank_plan_i32 can express it equals tests/track_ref.py::plan bit for bit; and the log compacts in row order."""
import os

import numpy as np
import pytest

import track_ref as R
import update_ref as U
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "updater_rules.npz")
W = 9


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def scene_frames(z, i):
    """the frames of scene i: per frame a dict of the recorded lists"""
    names = ("det_decision", "trk_ids", "trk_codes", "match_ids", "match_dets", "active_ids", "active_misses",
             "active_steps", "decom_ids", "output_ids", "track_count")
    cut = {k: np.concatenate([[0], np.cumsum(z["%s_n_%d" % (k, i)])]) for k in names}
    return [{k: z["%s_%d" % (k, i)][cut[k][f]:cut[k][f + 1]] for k in names} for f in range(int(z["frames"]))]


def scene_rules(z, i):
    config = {k: dict(zip(("output", "active", "decom"), row)) for k, row in zip(U.RULE_KEYS, z["config_%d" % i])}
    det_names = [U.RULE_KEYS[k] for k in z["det_names_%d" % i]]
    trk_names = [U.RULE_KEYS[k] for k in z["trk_names_%d" % i]]
    assert det_names == sorted(det_names) and trk_names == sorted(trk_names)
    return U.rules_from_config(config, det_names, trk_names), config


def run_scene(z, i, fault=None):
    """the restatement over scene i -> [] if every frame agrees with the reference, else the disagreements"""
    g = np.random.default_rng(i)
    rules, _ = scene_rules(z, i)
    dd, td, C, limit = (int(z["%s_%d" % (k, i)]) for k in ("dd", "td", "capacity", "frame_limit"))
    st = R.new_state(C, W)
    bad = []
    for f, fr in enumerate(scene_frames(z, i)):
        D = len(fr["det_decision"])
        slot_of = {int(t): s for s, t in enumerate(st["ids"]) if t >= 0}
        if sorted(slot_of) != sorted(fr["trk_ids"].tolist()):
            bad.append((f, "active before"))
            break
        t2d, d2t = np.full(C, -1, np.int32), np.full(D, -1, np.int32)
        tdec = np.full(C, 1 + td, np.int32)
        for t, code in zip(fr["trk_ids"], fr["trk_codes"]):
            tdec[slot_of[int(t)]] = code
        for t, d in zip(fr["match_ids"], fr["match_dets"]):
            t2d[slot_of[int(t)]], d2t[d] = d, slot_of[int(t)]
        st, src, det_slot, det_id, info, table = U.plan_rules(
            st, t2d, d2t, g.integers(0, 3, D).astype(np.int32), g.integers(1, 6, D).astype(np.int32), R.det_boxes(g, D, W),
            g.uniform(0.05, 1.0, D).astype(np.float32), fr["det_decision"], tdec, rules, frame_limit=limit, fault=fault)
        live = st["ids"] >= 0
        by_id = {int(t): s for s, t in enumerate(st["ids"]) if t >= 0}
        if info[0] != 0:
            bad.append((f, "dropped"))
        if sorted(by_id) != sorted(fr["active_ids"].tolist()) or live.sum() != len(fr["active_ids"]):
            bad.append((f, "active"))
            break
        if sorted(table["out_ids"][table["out_valid"] != 0].tolist()) != sorted(fr["output_ids"].tolist()):
            bad.append((f, "output"))
        if any(st["misses"][by_id[int(t)]] != m for t, m in zip(fr["active_ids"], fr["active_misses"])):
            bad.append((f, "misses"))
        if any(st["steps"][by_id[int(t)]] != n for t, n in zip(fr["active_ids"], fr["active_steps"])):
            bad.append((f, "steps"))
        if st["next_id"][0] != fr["track_count"][0]:
            bad.append((f, "next_id"))
        # a row that carries the rule's DECOM flag belongs to a track the reference decommissioned in this frame (but for a
        # propagated one: the reference adds a track_false_negative track to decomTracks only when it expires, :136-138)
        decom = table["out_ids"][(table["out_valid"] != 0) & (table["out_flags"] == 1)]
        if not set(decom.tolist()) <= set(fr["decom_ids"].tolist()):
            bad.append((f, "decom"))
    return bad


def test_golden_covers_what_the_issue_asks(golden):
    z = golden
    n = int(z["scenes"])
    assert n >= 24 and int(z["frames"]) == 12
    shapes = {(int(z["dd_%d" % i]), int(z["td_%d" % i])) for i in range(n)}
    assert shapes == {(2, 0), (2, 1), (1, 2), (2, 2), (1, 1), (0, 1)}
    configs = {tuple(z["config_%d" % i].reshape(-1).tolist()) for i in range(n)}
    assert len(configs) >= 4
    keys = list(U.RULE_KEYS)
    assert any(z["config_%d" % i][keys.index("det_false_positive")][1] for i in range(n))        # det_false_positive active
    assert any(not z["config_%d" % i][keys.index("match")][1] for i in range(n))                 # match not active
    for i in range(n):
        assert not (z["config_%d" % i][:, 1] & z["config_%d" % i][:, 2]).any()


def test_restatement_follows_the_reference_updater_frame_by_frame(golden):
    for i in range(int(golden["scenes"])):
        assert run_scene(golden, i) == [], i


@pytest.mark.parametrize("fault,what", [("index_order_ids", "active"), ("propagate_unmatched", "output"),
                                        ("output_expired", "output")])
def test_planted_faults_are_caught_by_the_golden(golden, fault, what):
    caught = [i for i in range(int(golden["scenes"])) if run_scene(golden, i, fault=fault)]
    assert len(caught) >= 3, (fault, caught)
    assert any(what in [k for _, k in run_scene(golden, i, fault=fault)] for i in caught), fault


# ---- against track_ref.plan in the forms the one-flag plan can express --------------------------------------------------------
def _same_state(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in R.STATE)


@pytest.mark.parametrize("td", [1, 0])
@pytest.mark.parametrize("W_,with_carry", [(9, True), (7, False)])
def test_equals_the_one_flag_plan_bit_for_bit(td, W_, with_carry):
    """dd = 1 (det_newborn: output + active), td = 1 (track_false_negative: active) with no track left unmatched is
    plan(propagate=True, born=<decision mask>); with td = 0 every missed track waits: plan(propagate=False)"""
    g = np.random.default_rng([td, W_])
    C, D = 70, 40
    st = R.random_state(g, C, W_, 0.6)
    rules = dict(match_rule=U.OUTPUT | U.ACTIVE, det_rule=[U.OUTPUT | U.ACTIVE], trk_rule=[U.ACTIVE] * td, trk_kind=[U.MISS] * td)
    carry = R.rigid(g)[0] if with_carry else None
    for f in range(12):
        fr = R.make_frame(g, st, D, W_, masks=False, junk=False, p_match=0.5)
        born = (g.random(D) < 0.7).astype(np.int32)
        ddec = np.where(born != 0, 1, 2).astype(np.int32)
        tdec = np.full(C, 1, np.int32)             # td = 1: every unpaired track is a miss; td = 0: it is unmatched
        for s, d in fr["intended"]:
            tdec[s], ddec[d] = 0, 0
        for args in (dict(), dict(replace_all=True, reset_on_match=True)):
            want, w_src, w_slot, w_id = R.plan(st, fr["track_to_det"], fr["det_to_track"], fr["labels"], fr["lengths"],
                                               fr["boxes"], fr["scores"], born=born, carry=carry, frame_limit=3,
                                               propagate=td == 1, **args)
            got, src, det_slot, det_id, info, table = U.plan_rules(
                st, fr["track_to_det"], fr["det_to_track"], fr["labels"], fr["lengths"], fr["boxes"], fr["scores"], ddec,
                tdec, rules, carry=carry, frame_limit=3, **args)
            assert _same_state(got, want), f
            assert (src == w_src).all() and (det_slot == w_slot).all(), f
            slotted = w_slot >= 0
            assert (det_id[slotted] == w_id[slotted]).all() and info[0] == want["info"][0]
            # matched and newborn tracks are output from their slots, nothing else is
            out = np.zeros(C + D, bool)
            out[w_slot[slotted]] = True
            assert (table["out_valid"] != 0).tolist() == out.tolist() and info[1] == out.sum()
        st = want
    assert (st["ids"] >= 0).sum() > 10


def test_rules_on_a_hand_made_frame():
    """one frame worked by hand: every branch of the rules once"""
    C, D = 6, 5
    st = R.new_state(C, 7)
    st["ids"][:5] = [10, 11, 12, 13, 14]
    st["labels"][:5], st["lengths"][:5], st["steps"][:5] = 1, 3, 2
    st["misses"][:5] = [0, 0, 1, 1, 0]
    st["scores"][:5] = 0.5
    st["boxes"][:5, 0] = np.arange(5)
    st["next_id"][0] = 20
    rules = dict(match_rule=U.OUTPUT | U.ACTIVE, det_rule=[U.OUTPUT | U.DECOM, U.OUTPUT | U.ACTIVE],
                 trk_rule=[U.OUTPUT | U.ACTIVE, U.OUTPUT | U.DECOM], trk_kind=[U.MISS, U.KEEP])
    labels = np.array([1, 1, -1, 1, 1], np.int32)
    boxes = R.det_boxes(np.random.default_rng(0), D, 7)
    ddec = np.array([0, 2, 2, 1, 2], np.int32)               # matched, newborn, (no label), false positive, newborn
    tdec = np.array([0, 1, 1, 2, 3, 1], np.int32)            # matched, miss, miss (expires), false positive, unmatched
    t2d, d2t = np.array([0, -1, -1, -1, -1, -1], np.int32), np.array([0, -1, -1, -1, -1], np.int32)
    new, src, det_slot, det_id, info, table = U.plan_rules(st, t2d, d2t, labels, np.full(D, 4, np.int32), boxes,
                                                           np.full(D, 0.9, np.float32), ddec, tdec, rules, frame_limit=2)
    assert new["ids"].tolist() == [10, 11, -1, -1, 14, 21]                       # the false positive (20) takes no slot
    assert det_id.tolist() == [10, 21, -1, 20, 22] and det_slot.tolist() == [0, 5, -1, -1, -1]
    assert new["next_id"][0] == 23 and info.tolist() == [1, 6]
    assert new["misses"][:5].tolist() == [0, 1, 2, 1, 1] and new["steps"][:5].tolist() == [3, 3, 2, 2, 2]
    assert src.tolist() == [0, -1, -1, -1, -1, 1]
    valid = np.flatnonzero(table["out_valid"])
    assert valid.tolist() == [0, 1, 3, 5, C + 3, C + 4]                          # row C + 4: the newborn that found no slot
    assert table["out_ids"][valid].tolist() == [10, 11, 13, 21, 20, 22]
    assert table["out_flags"][valid].tolist() == [0, 2, 1, 0, 1, 0]
    assert table["out_scores"][1] == np.float32(np.float32(0.5) * np.float32(0.01))
    assert (table["out_ids"][[2, 4]] == -1).all() and (table["out_boxes"][[2, 4]] == 0).all()


# ---- the log ----------------------------------------------------------------------------------------------------------------
def test_log_compacts_in_row_order_counts_overflow_and_advances_the_frame():
    g = np.random.default_rng(3)
    rows, width = 10, 7
    log = U.new_log(12, width)
    want_ids, want_frames, lost = [], [], 0
    for f in range(4):
        table = U.new_table(rows, width)
        table["out_valid"][:] = g.random(rows) < 0.5
        table["out_ids"][:] = 100 * f + np.arange(rows)
        table["out_boxes"][:] = g.standard_normal((rows, width))
        table["out_flags"][:] = g.integers(0, 4, rows)
        before = log
        log = U.log_append(log, table)
        assert before["frame_no"][0] == f and log["frame_no"][0] == f + 1        # (and the input log is left alone)
        ids = table["out_ids"][table["out_valid"] != 0].tolist()
        room = 12 - len(want_ids)
        want_ids += ids[:room]
        want_frames += [f] * len(ids[:room])
        lost += len(ids) - len(ids[:room])
        rec = U.log_records(log)
        assert rec["id"].tolist() == want_ids and rec["frame"].tolist() == want_frames
        assert log["cursor"][0] == len(want_ids) and log["dropped"][0] == lost
    assert lost > 0 and log["cursor"][0] == 12
    assert rec["box"].shape == (12, width) and rec["box"].dtype == np.float32
