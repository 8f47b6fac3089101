"""GPU: the updater as configured and the scene log (include/pcr.h section A11, pcr_amd/tracks.py) against the numpy
restatement of tests/update_ref.py.  Every comparison is bit for bit: the state arrays, src, det_slot, det_id, info, the
whole output table and the log.  A scene carries its state over 12 frames, on the device and in the restatement, so
that slots freed by one frame are taken again by a later one."""
import numpy as np
import pytest
import torch

import track_ref as R
import update_ref as U

pytestmark = pytest.mark.gpu

FRAMES = 12
STATE = R.STATE[:-1]                                         # (the bank's own info is the first entry of the launch's info)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_rules(rules):
    from pcr_amd import tracks as T
    return T.UpdateRules.from_words(rules["match_rule"], rules["det_rule"], rules["trk_rule"], rules["trk_kind"])


def scene_rules(g, dd, td):
    """random rule words; the last detection decision makes tracks that stay, so that every scene has births"""
    rules = U.random_rules(g, dd, td)
    if dd:
        rules["det_rule"][-1] = U.OUTPUT | U.ACTIVE
    return rules


def run_scene(C, D, W, dd, td, seed, with_carry, rules=None, frame_limit=3, rows_max=None, p_active=0.5, frames=FRAMES,
              **frame_args):
    """one scene on the device, every frame held against the restatement -> (the per-frame snapshots of everything the
    launches wrote, the restatement's per-frame info, the log's records)"""
    from pcr_amd import tracks as T
    g = np.random.default_rng([C, D, W, dd, td, seed])
    rules = scene_rules(g, dd, td) if rules is None else rules
    rules_d = device_rules(rules)
    st = R.random_state(g, C, W, p_active)
    carry = R.rigid(g)[0] if with_carry else None
    d_st = {k: dev(st[k]) for k in STATE}
    src = torch.full((C,), 99, dtype=torch.int32, device="cuda")
    det_slot, det_id = (torch.full((D,), 99, dtype=torch.int32, device="cuda") for _ in range(2))
    info = torch.full((2,), 99, dtype=torch.int32, device="cuda")
    table = {k: torch.full_like(v, 77) for k, v in T.new_table(C + D, W, "cuda").items()}       # every element is written
    rows_max = FRAMES * (C + D) if rows_max is None else rows_max
    log, want_log = T.SceneLog(rows_max, C + D, W), U.new_log(rows_max, W)
    snaps, infos = [], []
    for f in range(frames):
        fr = U.make_frame(g, st, D, W, dd, td, **frame_args)
        st, w_src, w_slot, w_id, w_info, w_table = U.plan_frame(st, fr, rules, carry=carry, frame_limit=frame_limit,
                                                                reset_on_match=bool(seed & 1), replace_all=bool(seed & 2))
        T.plan_rules(d_st, dev(fr["track_to_det"]), dev(fr["det_to_track"]), dev(fr["labels"]), dev(fr["lengths"]),
                     dev(fr["boxes"]), dev(fr["scores"]), dev(fr["det_decision"]), dev(fr["track_decision"]), rules_d, src,
                     det_slot, det_id, info, table, carry=dev(carry), frame_limit=frame_limit,
                     reset_on_match=bool(seed & 1), replace_all=bool(seed & 2))
        log.append(table)
        want_log = U.log_append(want_log, w_table)
        got = [host(d_st[k]).copy() for k in STATE] + [host(t).copy() for t in (src, det_slot, det_id, info)] + \
              [host(table[k]).copy() for k in U.TABLE]
        want = [st[k] for k in STATE] + [w_src, w_slot, w_id, w_info] + [w_table[k] for k in U.TABLE]
        names = list(STATE) + ["src", "det_slot", "det_id", "info"] + list(U.TABLE)
        for k, a, b in zip(names, got, want):
            assert same_bits(a, b), "frame %d: %s differs" % (f, k)
        snaps.append(got)
        infos.append(w_info)
    rec, want_rec = log.records(), U.log_records(want_log)
    for k in want_rec:
        assert same_bits(rec[k], want_rec[k]), "log column %s differs" % k
    assert rec["dropped"] == int(want_log["dropped"][0]) and rec["frames"] == frames == int(want_log["frame_no"][0])
    return snaps, np.array(infos), rec


# (C, D): the ballot-word boundaries on both sides, no detection at all, and the bench shape
SHAPES = [(1, 0), (1, 1), (5, 3), (64, 64), (65, 70), (200, 100)]
DECISIONS = [(2, 0), (1, 1), (2, 2), (4, 4)]


@pytest.mark.parametrize("dd,td", DECISIONS)
@pytest.mark.parametrize("C,D", SHAPES)
def test_plan_rules_and_the_log_equal_the_restatement_over_twelve_frames(C, D, dd, td):
    seen = np.zeros(2, np.int64)
    for seed, (W, with_carry) in enumerate(((9, True), (7, False), (9, False), (7, True))):
        _, infos, rec = run_scene(C, D, W, dd, td, seed, with_carry)
        seen += infos.sum(axis=0)
        assert rec["dropped"] == 0 and len(rec["id"]) == infos[:, 1].sum()
        assert (np.diff(rec["frame"]) >= 0).all()
    if C >= 64:
        assert seen[1] > 50                                  # rows were output


def test_free_slots_run_out_drops_are_counted_and_ids_still_advance():
    rules = dict(match_rule=U.OUTPUT | U.ACTIVE, det_rule=[U.OUTPUT | U.ACTIVE, U.ACTIVE], trk_rule=[U.OUTPUT | U.ACTIVE],
                 trk_kind=[U.MISS])
    snaps, infos, rec = run_scene(8, 40, 9, 2, 1, 5, True, rules=rules, frame_limit=4, p_active=0.5, p_new=0.9)
    assert (infos[:, 0] > 0).sum() >= 6                      # most frames drop newborns
    next_id = [int(s[len(STATE) - 1][0]) for s in snaps]
    det_id = [s[len(STATE) + 2] for s in snaps]
    for f in range(1, FRAMES):
        numbered = int((det_id[f] >= next_id[f - 1]).sum())
        assert next_id[f] == next_id[f - 1] + numbered > next_id[f - 1]          # every newborn is numbered, slot or not
    # an output newborn that found no slot is output from its detection's row
    valid = snaps[-1][len(STATE) + 4]
    assert valid[8:].sum() > 0


def test_frame_limit_one_frees_every_missed_track_at_once():
    snaps, infos, _ = run_scene(65, 30, 9, 2, 2, 3, True, frame_limit=1)
    run_scene(65, 30, 7, 1, 1, 4, False, frame_limit=1, junk=False)


def test_two_runs_give_identical_bits():
    a = run_scene(65, 70, 9, 2, 2, 9, True)[0]
    b = run_scene(65, 70, 9, 2, 2, 9, True)[0]
    for f, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert same_bits(u, v), f


def test_log_overflow_is_counted_and_nothing_is_written_past_the_end():
    _, infos, rec = run_scene(65, 70, 9, 2, 1, 6, True, rows_max=100)
    assert rec["dropped"] > 0 and len(rec["id"]) == 100 and rec["dropped"] + 100 == infos[:, 1].sum()
    assert rec["frames"] == FRAMES


# ---- one captured frame ------------------------------------------------------------------------------------------------------
FEAT = (3, 5)


def sequence(C, D, W, frames, rules, seed):
    g = np.random.default_rng(seed)
    st = R.new_state(C, W)
    out = []
    for f in range(frames):
        fr = U.make_frame(g, st, D, W, len(rules["det_rule"]), len(rules["trk_rule"]))
        fr["det_f"] = g.standard_normal((D,) + FEAT).astype(np.float32)
        fr["det_x"] = g.standard_normal((D, FEAT[1], 3)).astype(np.float32)
        fr["carry"] = R.rigid(g, span=1.0)[0]
        st = U.plan_frame(st, fr, rules, carry=fr["carry"], frame_limit=3)[0]
        out.append((fr, st))
    return out


def test_one_captured_frame_replayed_on_evolving_inputs_equals_the_eager_chain():
    from pcr_amd import tracks as T
    C, D, W = 40, 30, 9
    rules = dict(match_rule=U.OUTPUT | U.ACTIVE, det_rule=[U.OUTPUT | U.DECOM, U.OUTPUT | U.ACTIVE],
                 trk_rule=[U.OUTPUT | U.ACTIVE, U.DECOM], trk_kind=[U.MISS, U.KEEP])
    rules_d = device_rules(rules)
    seq = sequence(C, D, W, 4, rules, seed=21)
    bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)
    log = T.SceneLog(4 * (C + D), C + D, W)
    names = ("track_to_det", "det_to_track", "labels", "lengths", "boxes", "scores", "det_decision", "track_decision",
             "det_f", "det_x", "carry")
    S = {k: dev(seq[0][0][k]) for k in names}                # the static inputs of the capture

    def load(fr):
        for k in names:
            S[k].copy_(dev(fr[k]))

    def step():
        det_slot, det_id, info, table = bank.update_rules(
            (S["track_to_det"], S["det_to_track"]),
            dict(labels=S["labels"], lengths=S["lengths"], boxes=S["boxes"], scores=S["scores"], feats=S["det_f"], xyz=S["det_x"]),
            S["det_decision"], S["track_decision"], rules_d, carry=S["carry"], frame_limit=3)
        log.append(table)
        return [det_slot, det_id, info] + [table[k] for k in U.TABLE]

    def snapshot(outs):
        n = int(host(log.cursor)[0])                         # (a reset log keeps its old rows behind the cursor)
        return [host(t).copy() for t in outs] + [host(getattr(bank, k)).copy() for k in R.STATE] + \
               [host(bank.feats).copy(), host(bank.xyz).copy()] + \
               [host(getattr(log, k))[:n].copy() for k in ("frame", "id", "label", "flags", "score", "box")] + \
               [host(log._counters).copy()]

    eager = []
    for f, (fr, st) in enumerate(seq):
        load(fr)
        outs = step()
        for k in STATE:
            assert same_bits(host(getattr(bank, k)), st[k]), (f, k)
        assert host(bank.info)[0] == st["info"][0]
        eager.append(snapshot(outs))
    assert eager[-1][-1].tolist()[2] == 4 and eager[-1][-1][0] > 20              # four frames, rows logged
    # the same frames from ONE captured graph (the eager run above was the warm-up: nothing is loaded inside the capture)
    bank.reset()
    log.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    load(seq[0][0])
    with torch.cuda.graph(graph):                            # a device-to-host copy in here would fail the capture
        outs = step()
    bank.reset()                                             # (a capture records, it does not run)
    log.reset()
    for f, (fr, _) in enumerate(seq):
        load(fr)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(snapshot(outs), eager[f]):
            assert same_bits(a, b), f
