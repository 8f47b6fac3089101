"""numpy restatements of the ground-truth scoring (include/pcr.h section A7), written from the header's rules:

(a) the ARRAY form -- cost, decide, record over a bank of C slots and a book (slot_gt, slot_tte, gt_last, stats); the GPU
    tests compare the kernels with it bit for bit;
(b) a LIST form that keeps the books the way the reference's tracker does (index lists, np.intersect1d, masks, a
    track-id -> ground-truth mapping that grows with the tracks, a logging dict); the CPU test holds (a) against it.

`random_case` draws one frame with entries that the rules must ignore; `Scene` scripts a sequence of frames with births,
ends of ground-truth tracks, missed and false detections, a ground-truth id held by two slots and reused slots."""
import numpy as np

import assoc_ref as AR
import track_ref as TR

F = np.float32
KINDS = ("det_match", "det_newborn", "det_false_positive", "track_false_negative", "track_false_positive")
TOTAL_GT, TOTAL_CORRECT, FRAMES, GT_TOTAL, TP, FP, FN, SWITCHES, UNTRACKED, STATS = 15, 16, 17, 18, 19, 20, 21, 22, 23, 24
MOT = dict(frames=FRAMES, gt_total=GT_TOTAL, tp=TP, fp=FP, fn=FN, switches=SWITCHES, untracked=UNTRACKED)


# ---- (a) the array form ---------------------------------------------------------------------------------------------
def new_book(C, gt_cap):
    return dict(slot_gt=np.full(C, -1, np.int32), slot_tte=np.full(C, -1, np.int32), gt_last=np.full(gt_cap, -1, np.int32),
                stats=np.zeros(STATS, np.int32))


def copy_book(b):
    return {k: v.copy() for k, v in b.items()}


def gt_valid(gt_labels, gt_ids, gt_cap):
    gt_labels, gt_ids = np.asarray(gt_labels), np.asarray(gt_ids)
    return (gt_labels >= 0) & (gt_ids >= 0) & (gt_ids < gt_cap)


def cost(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, gt_cap, iou=None):
    """(D, G) float32: the centre distance in the direct form (or -iou) plus the 10000 mask"""
    D, G = len(det_labels), len(gt_labels)
    if iou is not None:
        base = (-np.asarray(iou, F)).astype(F).reshape(D, G)
    else:
        dx = (det_boxes[:, None, 0] - gt_boxes[None, :, 0]).astype(F)
        dy = (det_boxes[:, None, 1] - gt_boxes[None, :, 1]).astype(F)
        base = np.sqrt(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)).astype(F)      # numpy's float32 sqrt is correctly rounded
    same = (np.asarray(det_labels)[:, None] >= 0) & gt_valid(gt_labels, gt_ids, gt_cap)[None, :] & \
           (np.asarray(det_labels)[:, None] == np.asarray(gt_labels)[None, :])
    return (base + np.where(same, F(0), F(10000))).astype(F)


def own_decisions(ids, det_labels, track_to_det, det_to_track, born, kill):
    """pcr_bank_plan_i32's classes of the tracker's own decisions -> killed, matched, missed (C,), det_matched, det_born,
    det_rejected (D,), all bool"""
    C, D = len(ids), len(det_labels)
    active = np.asarray(ids) >= 0
    killed = active & (np.asarray(kill) != 0) if kill is not None else np.zeros(C, bool)
    matched = np.zeros(C, bool)
    for s in range(C):
        d = int(track_to_det[s])
        matched[s] = active[s] and not killed[s] and 0 <= d < D and det_labels[d] >= 0 and det_to_track[d] == s
    missed = active & ~killed & ~matched
    det_matched = np.zeros(D, bool)
    for d in range(D):
        t = int(det_to_track[d])
        det_matched[d] = det_labels[d] >= 0 and 0 <= t < C and track_to_det[t] == d and matched[t]
    valid = np.asarray(det_labels) >= 0
    det_born = valid & ~det_matched & (np.ones(D, bool) if born is None else np.asarray(born) != 0)
    return killed, matched, missed, det_matched, det_born, valid & ~det_matched & ~det_born


def truth(book, ids, col4row, row4col, info, cost_m, thresh, gt_labels, gt_ids, gt_cap, det_labels):
    """the true decisions of a frame -> dict(det_gt, true_t2d, true_d2t, det_truth, track_truth)"""
    C, D, G = len(ids), len(det_labels), len(gt_labels)
    ok = gt_valid(gt_labels, gt_ids, gt_cap)
    det_gt = np.full(D, -1, np.int32)
    if D > 0 and G > 0 and int(np.asarray(info).reshape(-1)[0]) == 0:
        for d in range(D):
            j = int(col4row[d])
            if det_labels[d] >= 0 and 0 <= j < G and row4col[j] == d and ok[j] and gt_labels[j] == det_labels[d] and \
                    F(cost_m[d, j]) < F(thresh):
                det_gt[d] = j
    true_t2d, true_d2t = np.full(C, -1, np.int32), np.full(D, -1, np.int32)
    holder = {}
    for s in range(C):                                       # the lowest slot that holds an id
        if ids[s] >= 0 and book["slot_gt"][s] >= 0:
            holder.setdefault(int(book["slot_gt"][s]), s)
    for d in range(D):                                       # the lowest true positive of an id takes the holder
        if det_gt[d] >= 0:
            s = holder.get(int(gt_ids[det_gt[d]]), -1)
            if s >= 0 and true_t2d[s] < 0:
                true_t2d[s], true_d2t[d] = d, s
    det_truth = np.where(np.asarray(det_labels) < 0, -1, np.where(true_d2t >= 0, 0, np.where(det_gt >= 0, 1, 2))).astype(np.int32)
    fp = (book["slot_gt"] < 0) | (book["slot_tte"] < 0)
    track_truth = np.where(np.asarray(ids) < 0, -1, np.where(true_t2d >= 0, 0, np.where(fp, 2, 1))).astype(np.int32)
    return dict(det_gt=det_gt, true_t2d=true_t2d, true_d2t=true_d2t, det_truth=det_truth, track_truth=track_truth)


def decide(book, ids, col4row, row4col, info, cost_m, thresh, gt_labels, gt_ids, gt_cap, det_labels, track_to_det,
           det_to_track, born=None, kill=None, skip_empty=True, forced=False):
    """-> (the new book, truth()'s dict); `book` itself is left alone.  forced: the tracker's decisions ARE the true ones"""
    out = truth(book, ids, col4row, row4col, info, cost_m, thresh, gt_labels, gt_ids, gt_cap, det_labels)
    if forced:
        track_to_det, det_to_track = out["true_t2d"], out["true_d2t"]
        born, kill = (out["det_truth"] == 1).astype(np.int32), (out["track_truth"] == 2).astype(np.int32)
    killed, matched, missed, det_matched, det_born, det_rejected = own_decisions(ids, det_labels, track_to_det, det_to_track,
                                                                                 born, kill)
    tt, dt = out["track_truth"], out["det_truth"]
    pairs = matched & (tt == 0) & (np.asarray(track_to_det) == out["true_t2d"])
    sets = ((tt == 0, pairs, matched), (dt == 1, det_born & (dt == 1), det_born), (dt == 2, det_rejected & (dt == 2), det_rejected),
            (tt == 1, missed & (tt == 1), missed), (tt == 2, killed & (tt == 2), killed))
    book = copy_book(book)
    for k, (gt, both, pred) in enumerate(sets):
        if skip_empty and gt.sum() == 0:
            continue
        book["stats"][3 * k:3 * k + 3] += np.array([gt.sum(), both.sum(), pred.sum()], np.int32)
        book["stats"][TOTAL_GT] += gt.sum()
        book["stats"][TOTAL_CORRECT] += both.sum()
    return book, out


def record(book, ids_now, track_truth, det_gt, det_slot, det_id, gt_labels, gt_ids, gt_tte, gt_cap, det_labels):
    """-> the new book, after the update and the track NMS"""
    C, D, G = len(ids_now), len(det_labels), len(gt_labels)
    ok = gt_valid(gt_labels, gt_ids, gt_cap)
    book = copy_book(book)
    tp = np.array([det_labels[d] >= 0 and 0 <= det_gt[d] < G and ok[det_gt[d]] for d in range(D)], bool).reshape(D)
    book["slot_tte"][np.asarray(track_truth) >= 0] -= 1
    for d in range(D - 1, -1, -1):                           # descending: the lowest detection of a slot writes last
        s = int(det_slot[d])
        if 0 <= s < C:
            book["slot_gt"][s], book["slot_tte"][s] = (gt_ids[det_gt[d]], gt_tte[det_gt[d]]) if tp[d] else (-1, -1)
    free = np.asarray(ids_now) < 0
    book["slot_gt"][free] = book["slot_tte"][free] = -1
    st = book["stats"]
    st[FRAMES] += 1
    st[GT_TOTAL] += ok.sum()
    st[TP] += tp.sum()
    st[FP] += ((np.asarray(det_labels) >= 0) & ~tp).sum()
    hit = np.zeros(G, bool)
    hit[[int(det_gt[d]) for d in range(D) if tp[d]]] = True
    st[FN] += (ok & ~hit).sum()
    seen = set()
    for d in range(D):
        if not tp[d]:
            continue
        g, i = int(gt_ids[det_gt[d]]), int(det_id[d])
        st[UNTRACKED] += i < 0
        if g in seen:
            continue
        seen.add(g)
        st[SWITCHES] += book["gt_last"][g] >= 0 and book["gt_last"][g] != i
        book["gt_last"][g] = i
    return book


def metrics(stats):
    """get_scene_metrics (virtual_tracker.py:1008-1017) over the table, plus MOTA and the raw counters"""
    stats = np.asarray(stats).astype(np.int64)
    out = {}
    for k, name in enumerate(KINDS):
        gt, correct, pred = (float(x) for x in stats[3 * k:3 * k + 3])
        r, p = correct / (gt + 1e-12), correct / (pred + 1e-12)
        out["recall_" + name], out["precision_" + name], out["f1_" + name] = r, p, 2 * ((r * p) / (r + p + 1e-12))
        out[name + "_gt"], out[name + "_correct"], out[name + "_num_pred"] = int(gt), int(correct), int(pred)
    out["total_gt"], out["total_correct"] = int(stats[TOTAL_GT]), int(stats[TOTAL_CORRECT])
    out["acc_total"] = stats[TOTAL_CORRECT] / (stats[TOTAL_GT] + 1e-12)
    for name, i in MOT.items():
        out[name] = int(stats[i])
    out["mota"] = 1.0 - (out["fn"] + out["fp"] + out["switches"]) / out["gt_total"] if out["gt_total"] else float("nan")
    return out


# ---- (b) the list form ------------------------------------------------------------------------------------------------
class ListTruth:
    """TrackingDecisionModifier.__call__ / get_stats / update_gt_track_mapping the reference's way: the tracks are known by
    their global id, `trkid_to_gt` / `trkid_to_tte` grow with the ids, the sets are index lists over the ACTIVE tracks (in
    the order given) and over the frame's real detections (no padding exists there)."""

    def __init__(self):
        self.trkid_to_gt, self.trkid_to_tte = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.logging = {}

    def decisions(self, prev_at, tp_det_idx, tp_gt_idx, gt_tracks, num_dets):
        """prev_at: the active tracks' ids; tp_*: get_iou_idx's index lists -> tp_decisions (index lists)"""
        n_trk = len(prev_at)
        active_gt = self.trkid_to_gt[prev_at] if n_trk else np.zeros(0, np.int64)
        active_tte = self.trkid_to_tte[prev_at] if n_trk else np.zeros(0, np.int64)
        det_to_gt = np.full(num_dets, -5, np.int64)
        det_to_gt[tp_det_idx] = gt_tracks[tp_gt_idx]
        _, trk_pos, det_pos = np.intersect1d(active_gt, det_to_gt, return_indices=True)
        tp = dict(pos_track_match=trk_pos, pos_det_match=det_pos)
        mask = np.zeros(num_dets)                             # det_false_positive (:35-39)
        mask[tp_det_idx] = 1
        tp["pos_det_false_positive"] = np.where(mask == 0)[0]
        mask = np.zeros(num_dets)                             # det_newborn (:41-46)
        mask[tp_det_idx] = 1
        mask[det_pos] = 0
        tp["pos_det_newborn"] = np.where(mask == 1)[0]
        mask = np.zeros(n_trk)                                # track_false_positive (:48-52)
        mask[(active_gt == -1) | (active_tte < 0)] = 1
        tp["pos_track_false_positive"] = np.where(mask == 1)[0]
        mask = np.zeros(n_trk)                                # track_false_negative (:54-59)
        mask[(active_gt != -1) & (active_tte >= 0)] = 1
        mask[trk_pos] = 0
        tp["pos_track_false_negative"] = np.where(mask == 1)[0]
        return tp

    def get_stats(self, decisions, tp):
        """decisions: the tracker's own index lists (track_match and det_match are parallel)"""
        for k in KINDS:
            if len(tp["pos_" + k]) == 0:
                continue
            gt, pred = tp["pos_" + k], decisions[k]
            if k == "det_match":
                sgt = set(zip(tp["pos_track_match"].tolist(), gt.tolist()))
                spred = set(zip(list(decisions["track_match"]), list(pred)))
                n = len(sgt & spred)
            else:
                n = len(np.intersect1d(pred, gt))
            for key, v in ((k + "_gt", len(gt)), (k + "_correct", n), (k + "_num_pred", len(pred)), ("total_gt", len(gt)),
                           ("total_correct", n)):
                self.logging[key] = self.logging.get(key, 0) + v

    def update_mapping(self, n_tracks, gt_tte, gt_tracks, tp_det_idx, tp_gt_idx, dets_to_trk):
        """update_gt_track_mapping (:297-347): n_tracks ids exist after the frame; dets_to_trk: the id every kept
        detection joined"""
        trkid = np.full(n_tracks, -2, np.int64)
        tte = np.full(n_tracks, -1, np.int64)
        trkid[:len(self.trkid_to_gt)] = self.trkid_to_gt
        tte[:len(self.trkid_to_tte)] += self.trkid_to_tte
        temp = np.ones(len(dets_to_trk), np.int64)
        temp[tp_det_idx] = 0
        fp = np.where(temp == 1)[0]
        trkid[dets_to_trk[tp_det_idx]] = gt_tracks[tp_gt_idx]
        tte[dets_to_trk[tp_det_idx]] = gt_tte[tp_gt_idx]
        trkid[dets_to_trk[fp]] = -1
        tte[dets_to_trk[fp]] = -1
        trkid[trkid == -2] = -1
        self.trkid_to_gt, self.trkid_to_tte = trkid, tte


# ---- frames ---------------------------------------------------------------------------------------------------------------
def lsa_maps(cost_m):
    """assoc_ref.lsa over cost (D, G) with the wrapper's convention for an empty problem -> col4row, row4col, info (1,)"""
    D, G = cost_m.shape
    if D == 0 or G == 0:
        return np.full(D, -1, np.int32), np.full(G, -1, np.int32), np.zeros(1, np.int32)
    c, r, _, _, info = AR.lsa(cost_m)
    return c, r, np.array([info], np.int32)


def random_case(g, C, D, G, W, gt_cap=64, masks=True, p_active=0.6):
    """one frame over a bank and a book in mid-sequence, with what the rules must ignore: padding on both sides, ids at and
    beyond gt_cap, ids that two slots hold and that two ground-truth boxes carry, stale entries in free slots, tracker maps
    that disagree -> a dict of everything decide and record read"""
    st = TR.random_state(g, C, W, p_active)
    fr = TR.make_frame(g, st, D, W, masks=masks, p_valid=0.85, span=20.0)
    gt_boxes = TR.det_boxes(g, G, W, span=20.0)
    gt_labels = np.where(g.random(G) < 0.85, g.integers(0, 3, G), -1).astype(np.int32)
    gt_ids = g.integers(0, min(gt_cap, max(2 * G, 4)), G).astype(np.int32)       # some ids twice
    if G > 2:
        gt_ids[0], gt_ids[1] = gt_cap, -1                       # padding by the id alone
    gt_tte = g.integers(0, 9, G).astype(np.int32)
    det_boxes = fr["boxes"]
    for d in range(min(D, G)):                                 # most detections sit on a ground-truth box
        if g.random() < 0.7:
            j = (d * 7) % G
            det_boxes[d, :2] = gt_boxes[j, :2] + g.uniform(-0.4, 0.4, 2).astype(F)
            det_boxes[d, 3:7] = gt_boxes[j, 3:7]
            if fr["labels"][d] >= 0 and gt_labels[j] >= 0 and g.random() < 0.8:
                fr["labels"][d] = gt_labels[j]                  # ... and often carry its class
    book = new_book(C, gt_cap)
    book["slot_gt"] = np.where(g.random(C) < 0.7, g.integers(0, max(len(set(gt_ids.tolist())), 1) + 2, C), -1).astype(np.int32)
    if G:
        pick = g.random(C) < 0.5
        book["slot_gt"][pick] = np.clip(gt_ids[g.integers(0, G, C)], -1, gt_cap - 1)[pick]
    book["slot_tte"] = g.integers(-2, 6, C).astype(np.int32)
    book["gt_last"] = np.where(g.random(gt_cap) < 0.5, g.integers(0, 3 * C + 40, gt_cap), -1).astype(np.int32)
    book["stats"] = g.integers(0, 50, STATS).astype(np.int32)
    return dict(st=st, fr=fr, book=book, det_boxes=det_boxes, det_labels=fr["labels"], gt_boxes=gt_boxes, gt_labels=gt_labels,
                gt_ids=gt_ids, gt_tte=gt_tte, gt_cap=gt_cap)


class Scene:
    """A scripted sequence.  Ground-truth objects of three classes stand on a grid at least 8 m apart and drift slowly; each
    lives from its first to its last frame (tte = the frames it still has).  A frame's detections are: a ground-truth box
    moved by up to 0.3 m (a true positive), or none (a missed object) and a false box 3 m from the missed object, beyond
    the 2 m threshold of `thresh`.  The detections are shuffled and padded to D, the ground truth to G.  A frame holds as
    many valid detections as valid ground-truth boxes (n_false caps the false boxes: fewer make it unbalanced): then, with
    D == G, the padding rows take the padding columns at 10000 flat and the assignment of the real boxes is the one
    of the unpadded problem -- an unbalanced frame leaves padding rows to real columns at 10000 + their distance from the
    origin, and which columns are left to them is part of the optimum (include/pcr.h)."""

    def __init__(self, n_obj, frames, D, G, W, seed, p_seen=0.8, n_false=1 << 20, thresh=2.0):
        g = self.g = np.random.default_rng(seed)
        self.D, self.G, self.W, self.frames, self.thresh, self.p_seen, self.n_false = D, G, W, frames, thresh, p_seen, n_false
        self.pos = np.stack([np.array([8.0 * (i % 6), 8.0 * (i // 6)]) + g.uniform(-0.5, 0.5, 2) for i in range(n_obj)])
        self.vel = g.uniform(-0.1, 0.1, (n_obj, 2))
        self.cls = g.integers(0, 3, n_obj).astype(np.int32)
        self.first = g.integers(0, max(frames // 2, 1), n_obj)
        self.first[:max(n_obj // 2, 1)] = 0
        self.last = np.minimum(self.first + g.integers(3, frames, n_obj), frames + 3)
        self.last[0] = min(5, frames - 1)                     # an object that ends early
        self.gt_id = g.permutation(4 * n_obj)[:n_obj].astype(np.int32)
        self.gt_cap = 4 * n_obj

    def frame(self, f):
        """-> dict(det_boxes (D, W), det_labels, det_scores, gt_boxes (G, W), gt_labels, gt_ids, gt_tte, pairs): `pairs` lists
        the (detection, ground-truth row) pairs that are true positives by construction"""
        g, D, G, W = self.g, self.D, self.G, self.W
        alive = [i for i in range(len(self.cls)) if self.first[i] <= f <= self.last[i]][:G]
        rows = g.permutation(G)[:len(alive)]
        gt_boxes, gt_labels = np.zeros((G, W), F), np.full(G, -1, np.int32)
        gt_ids, gt_tte = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
        det, missed = [], []
        for i, j in zip(alive, rows):
            p = self.pos[i] + f * self.vel[i]
            gt_boxes[j, :2], gt_boxes[j, 3:6], gt_labels[j] = p, (2.0, 4.0, 1.5), self.cls[i]
            gt_ids[j], gt_tte[j] = self.gt_id[i], self.last[i] - f
            if g.random() < self.p_seen:
                r, a = g.uniform(0.0, 0.3), g.uniform(0, 2 * np.pi)
                det.append((p + r * np.array([np.cos(a), np.sin(a)]), self.cls[i], j))
            else:
                missed.append((p, self.cls[i]))
        for p, c in missed[:self.n_false]:
            det.append((p + np.array([3.0, 0.0]), c, -1))
        det = [det[k] for k in g.permutation(len(det))][:D]
        rows_d = np.sort(g.permutation(D)[:len(det)])
        det_boxes, det_labels = np.zeros((D, W), F), np.full(D, -1, np.int32)
        pairs = []
        for d, (p, c, j) in zip(rows_d, det):
            det_boxes[d, :2], det_boxes[d, 3:6], det_labels[d] = p, (2.0, 4.0, 1.5), c
            if j >= 0:
                pairs.append((int(d), int(j)))
        return dict(det_boxes=det_boxes, det_labels=det_labels, det_scores=g.uniform(0.3, 1.0, D).astype(F), gt_boxes=gt_boxes,
                    gt_labels=gt_labels, gt_ids=gt_ids, gt_tte=gt_tte, pairs=sorted(pairs))


def corrupt(g, tr, ids, det_labels):
    """the tracker's own decisions for a frame: the true ones with a head's mistakes -- a match not made (the detection
    is born instead: its id then lives in two slots), a newborn rejected, a false detection let in, a missed track
    matched to a false detection, a false-positive track kept, a good track killed"""
    t2d, d2t = tr["true_t2d"].copy(), tr["true_d2t"].copy()
    born, kill = (tr["det_truth"] == 1).astype(np.int32), (tr["track_truth"] == 2).astype(np.int32)
    for s in np.nonzero(t2d >= 0)[0]:
        if g.random() < 0.2:
            born[t2d[s]] = 1
            d2t[t2d[s]], t2d[s] = -1, -1
    for d in np.nonzero(tr["det_truth"] == 1)[0]:
        born[d] = g.random() < 0.85
    false = [int(d) for d in np.nonzero(tr["det_truth"] == 2)[0]]
    for s in np.nonzero(tr["track_truth"] == 1)[0]:
        if false and g.random() < 0.4:
            d = false.pop()
            t2d[s], d2t[d] = d, s
    for d in false:
        born[d] = g.random() < 0.5
    for s in np.nonzero(ids >= 0)[0]:
        if kill[s]:
            kill[s] = g.random() < 0.7
        elif t2d[s] < 0 and g.random() < 0.05:
            kill[s] = 1
    return t2d, d2t, born, kill


# ---- generated cases of the fixture tool (tools/make_truth_golden.py) and the tests ------------------------------------------
LSA_SHAPES = ((1, 1), (3, 5), (5, 3), (17, 33), (30, 30), (64, 64), (67, 66), (100, 37))
LSA_SEEDS = 3
LSA_THRESH = dict(centre=2.0, iou=0.3)


def lsa_case(D, G, seed, kind="centre", W=9, classes=3):
    """detections and ground truth of a get_iou_idx call, padding included: the ground truth stands on a 14 m grid,
    jittered by 0.5 m, so any two boxes are at least 6 m apart; a detection lies within 0.5 m of one ground-truth box (at
    most one detection per box, often of its class) or in the middle of a cell, beyond 6 m of all (the CPU test checks
    both promises) -> dict(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, gt_cap, cost, thresh, iou)"""
    import nms_ref as NR
    g = np.random.default_rng([D, G, seed, kind == "iou"])
    gt_cap = 2 * G + 3
    side = int(np.ceil(np.sqrt(G))) + 1
    cells = g.permutation(side * side)[:G]
    gt_boxes = TR.det_boxes(g, G, W)
    gt_boxes[:, 0] = 14.0 * (cells % side) + g.uniform(-0.5, 0.5, G)
    gt_boxes[:, 1] = 14.0 * (cells // side) + g.uniform(-0.5, 0.5, G)
    gt_boxes[:, 3:6] = (2.0, 4.0, 1.5)
    gt_labels = np.where(g.random(G) < 0.9, g.integers(0, classes, G), -1).astype(np.int32)
    gt_ids = g.permutation(gt_cap + 2)[:G].astype(np.int32)                      # an id or two at or beyond gt_cap: padding
    det_boxes = TR.det_boxes(g, D, W)
    det_boxes[:, 3:6] = (2.0, 4.0, 1.5)
    det_labels = np.where(g.random(D) < 0.9, g.integers(0, classes, D), -1).astype(np.int32)
    owners = g.permutation(G)
    for d in range(D):
        if d < G and g.random() < 0.7:                                           # on a ground-truth box, often of its class
            j = owners[d]
            r, a = g.uniform(0.0, 0.5), g.uniform(0, 2 * np.pi)
            det_boxes[d, :2] = gt_boxes[j, :2] + r * np.array([np.cos(a), np.sin(a)])
            det_boxes[d, 6] = gt_boxes[j, 6]
            if gt_labels[j] >= 0 and g.random() < 0.85:
                det_labels[d] = gt_labels[j]
        else:                                                                    # in the middle of a cell: 7 m x 7 m from the nodes
            c = g.integers(0, side * side)
            det_boxes[d, 0] = 14.0 * (c % side) + 7.0 + g.uniform(-0.5, 0.5)
            det_boxes[d, 1] = 14.0 * (c // side) + 7.0 + g.uniform(-0.5, 0.5)
    iou = NR.iou_axis(NR.nearest_bev(det_boxes[:, :7]), NR.nearest_bev(gt_boxes[:, :7])) if kind == "iou" else None
    thresh = LSA_THRESH[kind] if kind == "centre" else -LSA_THRESH[kind]
    return dict(det_boxes=det_boxes, det_labels=det_labels, gt_boxes=gt_boxes, gt_labels=gt_labels, gt_ids=gt_ids,
                gt_cap=gt_cap, cost=cost(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, gt_cap, iou=iou), thresh=thresh,
                iou=iou)


def lsa_cases():
    """[(name, case)] in the order of the fixture file"""
    out = []
    for D, G in LSA_SHAPES:
        for s in range(LSA_SEEDS):
            kind = "iou" if s == LSA_SEEDS - 1 else "centre"
            out.append(("%s_%d_%d_%d" % (kind, D, G, s), lsa_case(D, G, s, kind)))
    return out


def thresholded(col_of_row, cost_m, thresh):
    """get_iou_idx's outcome: the assigned (row, column) pairs whose cost is below thresh, as a sorted list"""
    return sorted((int(d), int(j)) for d, j in enumerate(col_of_row) if j >= 0 and F(cost_m[d, j]) < F(thresh))
