"""GPU: ReIDNet.track_step(decisions=, update_config=, log=) on the toy Point-Transformer: a scripted 8-frame scene whose
bank state and output table equal, frame by frame, the restatement of tests/update_ref.py applied to that frame's own
decoded assignment and decisions; the log holds the valid rows of every frame; truth= and identity= keep working on top;
and a frame without the two arguments returns what it always returned."""
import numpy as np
import pytest
import torch

import nms_ref as NR
import track_ref as R
import update_ref as U
from test_gpu_tracks import dev, host, same_bits, toy_frames

pytestmark = pytest.mark.gpu

C, D, M, W, N = 16, 8, 6, 9, 128
FRAMES, LIMIT, THRESH = 8, 3, 0.15
SHIFT = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0], np.float32)        # previous frame -> current
BACK = np.array([1, 0, 0, -0.5, 0, 1, 0, 0.25, 0, 0, 1, 0], np.float32)
flags = lambda output, active, decom=False: dict(output=output, active=active, decom=decom)
CONFIG = dict(match=flags(True, True), det_newborn=flags(True, True), det_false_positive=flags(True, False, True),
              track_false_positive=flags(False, False, True), track_false_negative=flags(True, True))
DECISIONS = dict(detection=("det_newborn", "det_false_positive"), tracking=("track_false_positive", "track_false_negative"))
# the keys of a frame without decisions= (the parent commit's) and what decisions= adds to them
PLAIN_KEYS = {"track_to_det", "det_to_track", "pairs", "count", "logits", "cost", "info", "det_slot", "det_id", "bank_info",
              "dist", "lengths"}
DECISION_KEYS = {"det_decision", "track_decision", "born", "kill", "decode_info"}


@pytest.fixture(scope="module")
def toy():
    import bench
    model, _ = bench.build_pt_model([N, 64, 32])
    frames = toy_frames(FRAMES, M, N + 20, W, seed=31)
    with torch.no_grad():
        boxes0 = np.concatenate([frames[0][1], np.zeros((D - M, W), np.float32)])
        c0 = model.forward_inference_boxes(dev(frames[0][0]), dev(boxes0[:, :7].copy()), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])
    return model, frames


def present(f):
    """the objects the detector reports in frame f: object 3 is missed in frames 2 .. 5 (its track is propagated and then
    expires), one more object is missed in turn"""
    return [m for m in range(M) if f == 0 or not (m == f % M or (m == 3 and 2 <= f <= 5))]


def values(f, keep):
    """scripted costs, margin kind, rows in the sorted order of the names: (det_false_positive, det_newborn) per reported
    detection and (track_false_negative, track_false_positive) per slot.  Frame 0 bears everything; later a match is
    cheaper than any decision, a track without a detection is a false negative, in frame 4 the first detection is a false
    positive and in frame 6 slot 1 is a false-positive track"""
    det = np.zeros((2, len(keep)), np.float32)
    det[0], det[1] = 7.0, 6.0
    trk = np.zeros((2, C), np.float32)
    trk[0], trk[1] = 8.0, 9.0
    if f == 0:
        det[1] = -1.0 - 0.1 * np.arange(len(keep))
    if f == 4:
        det[0, 0] = -50.0
    if f == 6:
        trk[1, 1] = -70.0
    return det, trk


def run_scene(model, frames, log=None, truth_books=None, update_config=CONFIG):
    from pcr_amd import tracks as T
    bank = T.TrackBank(C, D, feat_shape=(64, N), box_width=W)
    got = []
    with torch.no_grad():
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            keep = present(f)
            det, trk = values(f, keep)
            truth = None
            if truth_books is not None:
                book, ident = truth_books(bank) if f == 0 else got[0]["books"]
                truth = dict(book=book, identity=ident, boxes=dev(boxes), labels=dev(labels),
                             ids=dev(np.arange(M, dtype=np.int32) * 5 + 2), tte=dev(np.full(M, FRAMES - 1 - f, np.int32)))
            out = model.track_step(bank, dev(pts), dev(boxes[keep]), dev(labels[keep]), dev(scores[keep]), carry=dev(SHIFT),
                                   carry_inv=dev(BACK), crop_args=dict(seed=5 + f), frame_limit=LIMIT,
                                   suppress_threshold=THRESH, decisions=dict(DECISIONS, det_values=dev(det), track_values=dev(trk)),
                                   update_config=update_config, log=log, truth=truth)
            got.append(dict(out={k: host(v).copy() for k, v in out.items() if v is not None},
                            st={k: host(v).copy() for k, v in bank.state().items()}, feats=host(bank.feats).copy(),
                            xyz=host(bank.xyz).copy(), det_feats=host(bank.det_feats).copy(), det_xyz=host(bank.det_xyz).copy(),
                            books=(truth["book"], truth["identity"]) if truth else None))
    return got


def test_scripted_scene_equals_the_restatement_frame_by_frame(toy):
    from pcr_amd import tracks as T
    model, frames = toy
    log = T.SceneLog(FRAMES * (C + D), C + D, W)
    got = run_scene(model, frames, log=log)
    rules = U.rules_from_config(CONFIG, sorted(DECISIONS["detection"]), sorted(DECISIONS["tracking"]))
    pad = lambda a, fill: np.concatenate([a, np.full((D - len(a),) + a.shape[1:], fill, a.dtype)])
    st = R.new_state(C, W)
    feats, xyz = np.zeros((C, 64, N), np.float32), np.zeros((C, N, 3), np.float32)
    rows = {k: [] for k in ("frame", "id", "label", "flags", "score", "box")}
    seen = dict(propagated=0, expired=0, fp_det=0, fp_track=0, born_later=0)
    for f, (pts, boxes, labels, scores) in enumerate(frames):
        keep = present(f)
        o = got[f]["out"]
        assert set(o) == PLAIN_KEYS | DECISION_KEYS | set(U.TABLE), f
        before = st
        st, src, det_slot, det_id, info, table = U.plan_rules(
            st, o["track_to_det"], o["det_to_track"], pad(labels[keep], -1), o["lengths"], pad(boxes[keep], 0),
            pad(scores[keep], 0), o["det_decision"], o["track_decision"], rules, carry=SHIFT, frame_limit=LIMIT)
        feats, xyz = R.move(src, got[f]["det_feats"], got[f]["det_xyz"], feats, xyz)
        for k in U.TABLE:
            assert same_bits(o[k], table[k]), (f, k)
        assert same_bits(o["det_slot"], det_slot) and same_bits(o["det_id"], det_id) and same_bits(o["bank_info"], info), f
        valid = table["out_valid"] != 0
        for k, col in (("id", "out_ids"), ("label", "out_labels"), ("flags", "out_flags"), ("score", "out_scores"), ("box", "out_boxes")):
            rows[k].append(table[col][valid])
        rows["frame"].append(np.full(int(valid.sum()), f, np.int32))
        seen["propagated"] += int((table["out_flags"][valid] & 2 != 0).sum())
        seen["expired"] += int(((before["ids"] >= 0) & (st["ids"] < 0) & (st["misses"] >= LIMIT)).sum())
        seen["fp_det"] += int(valid[C:].sum())
        seen["fp_track"] += int((o["track_decision"] == 2).sum())
        seen["born_later"] += int(f > 0 and (o["det_decision"] == 2).any())
        # the track NMS after the update, as in the frame
        score = (st["steps"].astype(np.float32) + st["scores"]).astype(np.float32)
        st = R.retire(NR.track_nms(NR.nearest_bev(st["boxes"][:, :7]), st["labels"], score, THRESH), st)
        for k in R.STATE:
            assert same_bits(got[f]["st"][k], st[k]), (f, k)
        assert same_bits(got[f]["feats"], feats) and same_bits(got[f]["xyz"], xyz), f
    assert min(seen.values()) > 0, seen                      # the script reaches every branch it was written for
    rec = log.records()
    for k, parts in rows.items():
        assert same_bits(rec[k], np.concatenate(parts)), k
    assert rec["dropped"] == 0 and rec["frames"] == FRAMES and len(rec["id"]) > FRAMES * (M - 2)


def test_truth_and_identity_keep_working_on_top(toy):
    from pcr_amd import identity as ID
    from pcr_amd import truth as TU
    model, frames = toy

    def books(bank):
        book = TU.TruthBook(bank, D, 40)
        return book, ID.IdentityBook(book, id_cap=32, gt_rows=30, max_rows=16, max_cols=32)
    plain = run_scene(model, frames)
    scored = run_scene(model, frames, truth_books=books)
    for f, (a, b) in enumerate(zip(plain, scored)):
        assert set(b["out"]) - set(a["out"]) == {"det_gt", "true_track_to_det", "true_det_to_track", "det_truth", "track_truth"}
        for k in a["out"]:
            assert same_bits(a["out"][k], b["out"][k]), (f, k)
        for k in a["st"]:
            assert same_bits(a["st"][k], b["st"][k]), (f, k)
    book, ident = scored[0]["books"]
    ident.close_scene()
    for name, m in (("truth", book.metrics()), ("identity", ident.metrics())):
        numbers = [v for v in m.values() if isinstance(v, (int, float))]
        assert numbers and all(np.isfinite(v) for v in numbers), (name, m)


def test_a_frame_without_the_two_arguments_returns_what_it_always_returned(toy):
    from pcr_amd import tracks as T
    from pcr_amd._lib import PcrError
    model, frames = toy
    pts, boxes, labels, scores = (dev(x) for x in frames[0])
    det, trk = values(0, list(range(M)))
    with torch.no_grad():
        bank = T.TrackBank(C, D, feat_shape=(64, N), box_width=W)
        out = model.track_step(bank, pts, boxes, labels, scores, crop_args=dict(seed=5))
        assert set(out) == PLAIN_KEYS and out["bank_info"].shape == (1,)
        bank.reset()
        out = model.track_step(bank, pts, boxes, labels, scores, crop_args=dict(seed=5),
                               decisions=dict(DECISIONS, det_values=dev(det), track_values=dev(trk)))
        assert set(out) == PLAIN_KEYS | DECISION_KEYS and out["bank_info"].shape == (1,)
        with pytest.raises(PcrError, match="pass decisions= with it"):
            model.track_step(bank, pts, boxes, labels, scores, update_config=CONFIG)
        with pytest.raises(PcrError, match="no entry for 'det_false_positive'"):
            model.track_step(bank, pts, boxes, labels, scores, decisions=dict(DECISIONS),
                             update_config={k: v for k, v in CONFIG.items() if k != "det_false_positive"})
        with pytest.raises(PcrError, match="SceneLog of %d rows per frame" % (C + D)):
            model.track_step(bank, pts, boxes, labels, scores, decisions=dict(DECISIONS), update_config=CONFIG,
                             log=T.SceneLog(100, C + D - 1, W))
