#!/usr/bin/env python3
"""Writes tests/golden/updater_rules.npz: what the reference's own TrackingUpdater (trackers/deprecated/
tracking_updater.py:22-203) does with scripted decision lists under several update_configs -- which tracks stay active,
which are decommissioned, which are output, how the ids are numbered and how the unmatched-frame counts move.  The tests
read the file and import neither torch nor the reference.

The reference file is loaded by path, as tools/make_decisions_golden.py loads its file: mmdet3d.models.builder.TRACKERS is
stubbed, and a recording stand-in takes the place of `.track.Track` (it counts what the updater calls on it).  What is
pinned is the updater's LIST logic; the propagation arithmetic is pinned by tests/track_ref.py.

Scenes: every (dd, td) of make_decisions_golden.DECISIONS whose names exist in the updater (at most det_false_positive,
det_newborn / track_false_negative, track_false_positive; one decision of a side is det_newborn / track_false_negative),
times the update_configs of CONFIGS, 12 frames each.  Per frame the active tracks and up to MAX_DETS detections are
partitioned at random into matches, decisions and unmatched ones.  The capacity recorded for a scene is the smallest at
which nothing is dropped (the most `active tracks + ACTIVE newborns` of any frame).  The tool asserts that every scene with a
detection decision has births and outputs and that expiries and propagations occur; it discards nothing.

Per scene i (all int32): dd_i, td_i, capacity_i, frame_limit_i, config_i (5, 3) = output / active / decom of RULE_KEYS,
det_names_i / trk_names_i (indices into RULE_KEYS), and per name below the values of all frames concatenated plus
<name>_n_i (FRAMES,) = how many belong to each frame:
  det_decision   (D per frame) 0 = matched, 1 + k = detection decision k, 1 + dd = unmatched
  trk_ids, trk_codes   every track active before the frame and its decision code (0, 1 + k, 1 + td)
  match_ids, match_dets   the matched (track id, detection) pairs
  active_ids, active_misses, active_steps   activeTracks after the updater with unmatchedFrameCount and the number of
                 timesteps the stand-in holds (1 at birth, +1 per addTimestep and per add_false_negative_timestep)
  decom_ids      the ids added to decomTracks by this frame
  output_ids     the ids of the returned output list, in its order
  track_count    (1 per frame) the returned trackCount

    PCR_REFERENCE_ROOT=/path/to/reference python tools/make_updater_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_decisions_golden import DECISIONS, REF_ROOT, ROOT  # noqa: E402

RULE_KEYS = ("match", "det_newborn", "det_false_positive", "track_false_positive", "track_false_negative")
FRAMES = 12
MAX_DETS = 7
FRAME_LIMIT = 3
NAMES = ("det_decision", "trk_ids", "trk_codes", "match_ids", "match_dets", "active_ids", "active_misses", "active_steps",
         "decom_ids", "output_ids", "track_count")


def cfg(output, active, decom=False):
    return dict(output=output, active=active, decom=decom)


# match, det_newborn, det_false_positive, track_false_positive, track_false_negative
CONFIGS = (
    # the reference's usual run: false positives are dropped, false negatives propagated and output
    dict(match=cfg(True, True), det_newborn=cfg(True, True), det_false_positive=cfg(False, False, True),
         track_false_positive=cfg(False, False, True), track_false_negative=cfg(True, True)),
    # det_false_positive is kept (active) but not output; false negatives wait silently; false-positive tracks are output
    dict(match=cfg(True, True), det_newborn=cfg(True, True), det_false_positive=cfg(False, True),
         track_false_positive=cfg(True, False, True), track_false_negative=cfg(False, True)),
    # match is output and dropped: every track lives for one match
    dict(match=cfg(True, False, True), det_newborn=cfg(False, True), det_false_positive=cfg(True, False),
         track_false_positive=cfg(True, True), track_false_negative=cfg(True, False, True)),
    # everything is output, false-positive detections too; false-positive tracks stay
    dict(match=cfg(True, True), det_newborn=cfg(True, True), det_false_positive=cfg(True, True),
         track_false_positive=cfg(False, True), track_false_negative=cfg(True, True)),
    # nothing is output but matches; false-positive detections are numbered and not kept, a missed track is dropped
    dict(match=cfg(True, True), det_newborn=cfg(False, True), det_false_positive=cfg(False, False),
         track_false_positive=cfg(False, False), track_false_negative=cfg(False, False)),
)


class RecordingTrack:
    """what the updater touches of a Track, counted"""

    def __init__(self, id_, **_):
        self.id, self.unmatchedFrameCount, self.steps = id_, 0, 1

    def addTimestep(self, **_):
        self.steps += 1

    def unmatched_step(self):
        self.unmatchedFrameCount += 1

    def add_false_negative_timestep(self, **_):
        self.steps += 1


def load_reference():
    class _Registry:
        def register_module(self):
            return lambda cls: cls
    for name in ("mmdet3d", "mmdet3d.models", "mmdet3d.models.builder"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mmdet3d.models.builder"].TRACKERS = _Registry()
    pkg = types.ModuleType("_pcr_ref_trackers")
    pkg.__path__ = []
    track = types.ModuleType("_pcr_ref_trackers.track")
    track.Track = RecordingTrack
    sys.modules["_pcr_ref_trackers"], sys.modules["_pcr_ref_trackers.track"] = pkg, track
    path = os.path.join(REF_ROOT, "mmdet3d", "models", "trackers", "deprecated", "tracking_updater.py")
    spec = importlib.util.spec_from_file_location("_pcr_ref_trackers.tracking_updater", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def decision_names(dd, td):
    det = {0: [], 1: ["det_newborn"], 2: ["det_false_positive", "det_newborn"]}[dd]
    trk = {0: [], 1: ["track_false_negative"], 2: ["track_false_negative", "track_false_positive"]}[td]
    return det, trk


def main():
    import torch
    ref = load_reference()

    class Boxes:
        def __init__(self, tensor):
            self.tensor = tensor

        def __getitem__(self, idx):
            return self.tensor[idx]

    out, scene, overall = {}, 0, dict(born=0, expired=0, output=0, propagated=0)
    for ci, (dd, td) in enumerate(d for d in DECISIONS if d[0] <= 2 and d[1] <= 2):
        det_names, trk_names = decision_names(dd, td)
        for ui, update_config in enumerate(CONFIGS):
            g = np.random.default_rng(7000 + 100 * ci + ui)
            updater = ref.TrackingUpdater(dict(update_config, track_unmatched=None))
            tracker = types.SimpleNamespace(detection_decisions=det_names, tracking_decisions=trk_names, tracks=[],
                                            activeTracks=[], decomTracks=[], frameLimit=FRAME_LIMIT,
                                            propagation_method="velocity", non_max_suppression=lambda device: None)
            rec = {k: [] for k in NAMES}
            count, capacity, seen = 0, 1, dict(born=0, expired=0, output=0, propagated=0)
            for f in range(FRAMES):
                D = int(g.integers(2, MAX_DETS + 1))
                act = list(tracker.activeTracks)
                T = len(act)
                ddec, tdec = np.full(D, 1 + dd, np.int32), np.full(T, 1 + td, np.int32)
                n_match = int(g.integers(0, min(T, D) + 1)) if g.random() < 0.9 else 0
                m_trk, m_det = g.permutation(T)[:n_match], g.permutation(D)[:n_match]
                tdec[m_trk], ddec[m_det] = 0, 0
                for d in range(D):
                    if ddec[d] != 0 and dd > 0 and g.random() < 0.8:
                        ddec[d] = 1 + int(g.integers(0, dd))
                for t in range(T):
                    if tdec[t] != 0 and td > 0 and g.random() < 0.7:
                        tdec[t] = 1 + int(g.integers(0, td))
                as_t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
                decisions = dict(det_match=as_t(m_det), track_match=as_t(m_trk),
                                 det_unmatched=as_t(np.flatnonzero(ddec == 1 + dd)),
                                 track_unmatched=as_t(np.flatnonzero(tdec == 1 + td)))
                decisions.update({k: as_t(np.flatnonzero(ddec == 1 + i)) for i, k in enumerate(det_names)})
                decisions.update({k: as_t(np.flatnonzero(tdec == 1 + j)) for j, k in enumerate(trk_names)})
                new_active = sum(int((ddec == 1 + i).sum()) for i, k in enumerate(det_names) if update_config[k]["active"])
                capacity = max(capacity, T + new_active)
                ids_before = [tracker.tracks[i].id for i in act]
                steps_before = {tracker.tracks[i].id: tracker.tracks[i].steps for i in act}
                decom_before = len(tracker.decomTracks)
                count, output = updater(tracker, pred_cls=torch.zeros(D, dtype=torch.long), det_confidence=torch.ones(D),
                                        trackCount=count, bbox=Boxes(torch.zeros(D, 9)), decisions=decisions,
                                        sample_token="s%d" % f, refine_preds=torch.ones(D, 4),
                                        forecast_preds=torch.zeros(D, 2), timestep=f, ego=None, device="cpu")
                live = [tracker.tracks[i] for i in tracker.activeTracks]
                assert len({t.id for t in live}) == len(live)
                rec["det_decision"].append(ddec)
                rec["trk_ids"].append(ids_before)
                rec["trk_codes"].append(tdec)
                rec["match_ids"].append([ids_before[t] for t in m_trk])
                rec["match_dets"].append(m_det)
                rec["active_ids"].append([t.id for t in live])
                rec["active_misses"].append([t.unmatchedFrameCount for t in live])
                rec["active_steps"].append([t.steps for t in live])
                rec["decom_ids"].append([tracker.tracks[i].id for i in tracker.decomTracks[decom_before:]])
                rec["output_ids"].append([tracker.tracks[i].id for i in output])
                rec["track_count"].append([count])
                seen["born"] += new_active
                seen["output"] += len(output)
                seen["expired"] += sum(1 for t, i in enumerate(act) if tdec[t] != 0 and ids_before[t] not in
                                       {x.id for x in live} and tracker.tracks[i].unmatchedFrameCount >= FRAME_LIMIT)
                seen["propagated"] += sum(1 for t, i in enumerate(act) if tdec[t] != 0 and
                                          tracker.tracks[i].steps > steps_before[ids_before[t]])
            # (without a detection decision the updater never makes a track: such a scene pins that nothing appears)
            assert dd == 0 or (seen["born"] > 0 and seen["output"] > 0), (dd, td, ui, seen)
            for k, v in seen.items():
                overall[k] += v
            for k in NAMES:
                out["%s_n_%d" % (k, scene)] = np.array([len(v) for v in rec[k]], np.int32)
                out["%s_%d" % (k, scene)] = np.concatenate([np.asarray(v, np.int32).reshape(-1) for v in rec[k]])
            for k, v in (("dd", dd), ("td", td), ("capacity", capacity), ("frame_limit", FRAME_LIMIT)):
                out["%s_%d" % (k, scene)] = np.array(v, np.int32)
            out["config_%d" % scene] = np.array([[update_config[k][f] for f in ("output", "active", "decom")]
                                                 for k in RULE_KEYS], np.int32)
            out["det_names_%d" % scene] = np.array([RULE_KEYS.index(k) for k in det_names], np.int32)
            out["trk_names_%d" % scene] = np.array([RULE_KEYS.index(k) for k in trk_names], np.int32)
            scene += 1
    assert min(overall.values()) > 0, overall
    out["scenes"] = np.array(scene, np.int32)
    out["frames"] = np.array(FRAMES, np.int32)
    path = os.path.join(ROOT, "tests", "golden", "updater_rules.npz")
    np.savez_compressed(path, **out)
    print("%s: %d scenes of %d frames, %s, %d bytes" % (path, scene, FRAMES, overall, os.path.getsize(path)))


if __name__ == "__main__":
    main()
