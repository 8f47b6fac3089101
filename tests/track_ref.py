"""numpy restatements of the track state (include/pcr.h section A5), written from the header's rules:

(a) the ARRAY form -- plan, move, dist, retire over a bank of C slots, float32 operation for operation; the GPU tests
    compare the kernels with it bit for bit;
(b) a LIST form that keeps the books the way the reference's tracker does (a feature store that grows with one row per
    track and replace_old's rule, a list of track records with per-track lists, an activeTracks list); the CPU test holds
    (a) against it.

`make_frame` draws one frame of detections and an assignment for a given bank state, with entries that the rules must
ignore (maps that disagree, indices out of range, matches to free slots and to invalid detections)."""
import numpy as np

F = np.float32
STATE = ("lengths", "boxes", "scores", "labels", "ids", "steps", "misses", "next_id", "info")


def affine_row(m, x, y, z):
    """((m0 * x + m1 * y) + m2 * z) + m3, each operation rounded to float32"""
    a, b, c = F(m[0]) * F(x), F(m[1]) * F(y), F(m[2]) * F(z)
    return F(F(F(a + b) + c) + F(m[3]))


# ---- (a) the array form ---------------------------------------------------------------------------------------------
def new_state(C, W):
    return dict(lengths=np.zeros(C, np.int32), boxes=np.zeros((C, W), F), scores=np.zeros(C, F),
                labels=np.full(C, -1, np.int32), ids=np.full(C, -1, np.int32), steps=np.zeros(C, np.int32),
                misses=np.zeros(C, np.int32), next_id=np.zeros(1, np.int32), info=np.zeros(1, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def propagate_box(box, carry):
    """a missed track's box one frame on: the centre moves by half the velocity (W == 9) and through carry"""
    b = box.copy()
    x, y, z = b[0], b[1], b[2]
    if len(b) == 9:
        x, y = F(x + F(b[7] / F(2))), F(y + F(b[8] / F(2)))
    if carry is not None:
        m = np.asarray(carry, F).reshape(12)
        b[0], b[1], b[2] = affine_row(m[0:4], x, y, z), affine_row(m[4:8], x, y, z), affine_row(m[8:12], x, y, z)
    else:
        b[0], b[1] = x, y
    return b


def plan(st, track_to_det, det_to_track, det_labels, det_lengths, det_boxes, det_scores, born=None, kill=None, carry=None,
         frame_limit=10, replace_all=False, reset_on_match=False, propagate=True):
    """-> (the new state, src (C,), det_slot (D,), det_id (D,)); `st` itself is left alone"""
    old, st = st, copy_state(st)
    C, D = len(old["ids"]), len(det_labels)
    active = old["ids"] >= 0
    killed = active & (np.asarray(kill) != 0) if kill is not None else np.zeros(C, bool)
    matched = np.zeros(C, bool)
    for s in range(C):
        d = int(track_to_det[s])
        matched[s] = active[s] and not killed[s] and 0 <= d < D and det_labels[d] >= 0 and det_to_track[d] == s
    src = np.full(C, -1, np.int32)
    det_slot, det_id = np.full(D, -1, np.int32), np.full(D, -1, np.int32)
    taken = np.zeros(D, bool)
    for s in np.nonzero(active)[0]:
        if killed[s]:
            st["ids"][s] = st["labels"][s] = -1
            st["lengths"][s] = 0
        elif matched[s]:
            d = int(track_to_det[s])
            taken[d] = True
            det_slot[d], det_id[d] = s, old["ids"][s]
            st["boxes"][s], st["scores"][s], st["labels"][s] = det_boxes[d], det_scores[d], det_labels[d]
            st["steps"][s] += 1
            if reset_on_match:
                st["misses"][s] = 0
            if replace_all or old["lengths"][s] <= det_lengths[d]:
                st["lengths"][s] = det_lengths[d]
                src[s] = d
        else:
            st["misses"][s] += 1
            if st["misses"][s] >= frame_limit:
                st["ids"][s] = st["labels"][s] = -1
                st["lengths"][s] = 0
            elif propagate:
                st["boxes"][s] = propagate_box(old["boxes"][s], carry)
                st["scores"][s] = F(old["scores"][s] * F(0.01))
                st["steps"][s] += 1
    free = np.nonzero(~active)[0]
    newborn = [d for d in range(D) if det_labels[d] >= 0 and not taken[d] and (born is None or born[d] != 0)]
    n_born = min(len(newborn), len(free))
    for k in range(n_born):
        s, d = free[k], newborn[k]
        st["ids"][s] = old["next_id"][0] + k
        st["steps"][s], st["misses"][s] = 1, 0
        st["labels"][s], st["lengths"][s] = det_labels[d], det_lengths[d]
        st["boxes"][s], st["scores"][s] = det_boxes[d], det_scores[d]
        src[s] = d
        det_slot[d], det_id[d] = s, st["ids"][s]
    st["next_id"][0] = old["next_id"][0] + n_born
    st["info"][0] = len(newborn) - n_born
    return st, src, det_slot, det_id


def move(src, det_feats, det_xyz, feats, xyz):
    feats, xyz = feats.copy(), xyz.copy()
    for s, d in enumerate(src):
        if 0 <= d < len(det_feats):
            feats[s], xyz[s] = det_feats[d], det_xyz[d]
    return feats, xyz


def dist_sq(boxes, ids, det_boxes, carry_inv=None):
    """(C, D) float32: dx * dx + dy * dy of the header's rule (0 in a free slot's row)"""
    C, D = len(ids), len(det_boxes)
    out = np.zeros((C, D), F)
    px, py = det_boxes[:, 0].copy(), det_boxes[:, 1].copy()
    if carry_inv is not None:
        m = np.asarray(carry_inv, F).reshape(12)
        for d in range(D):
            x, y, z = det_boxes[d, 0], det_boxes[d, 1], det_boxes[d, 2]
            px[d], py[d] = affine_row(m[0:4], x, y, z), affine_row(m[4:8], x, y, z)
    for s in range(C):
        if ids[s] >= 0:
            dx, dy = (boxes[s, 0] - px).astype(F), (boxes[s, 1] - py).astype(F)
            out[s] = (dx * dx).astype(F) + (dy * dy).astype(F)
    return out


def dist(boxes, ids, det_boxes, carry_inv=None):
    return np.sqrt(dist_sq(boxes, ids, det_boxes, carry_inv)).astype(F)       # numpy's float32 sqrt is correctly rounded


def retire(mask, st):
    st = copy_state(st)
    hit = (st["ids"] >= 0) & (np.asarray(mask) != 0)
    st["ids"][hit] = st["labels"][hit] = -1
    st["lengths"][hit] = 0
    return st


# ---- (b) the list form ------------------------------------------------------------------------------------------------
class ListTracker:
    """The reference's bookkeeping: `tracks` only grows, `active` lists indices into it, the feature store holds one row
    per track in the order the tracks were made."""

    def __init__(self, replace_all=False):
        self.tracks, self.active, self.count = [], [], 0
        self.feats = self.xyz = self.lengths = None
        self.replace_all = replace_all

    def store_new(self, xyz, feats, lengths):
        if self.feats is None:
            self.feats, self.xyz, self.lengths = feats.copy(), xyz.copy(), lengths.copy()
        else:
            self.feats = np.concatenate([self.feats, feats], 0)
            self.xyz = np.concatenate([self.xyz, xyz], 0)
            self.lengths = np.concatenate([self.lengths, lengths], 0)

    def replace_old(self, index, xyz, feats, lengths):
        index = np.asarray(index, np.int64)
        if not self.replace_all:
            keep = np.nonzero(self.lengths[index] <= lengths)[0]
            index, xyz, feats, lengths = index[keep], xyz[keep], feats[keep], lengths[keep]
        self.feats[index], self.xyz[index], self.lengths[index] = feats, xyz, lengths

    def step(self, frame_no, matches, kills, det, born=None, carry=None, frame_limit=10, reset_on_match=False,
             propagate=True):
        """matches [(track id, detection)], kills [track id]; det: dict(labels, lengths, boxes, scores, feats, xyz)
        -> the id every detection joined (-1: none)"""
        by_id = {self.tracks[i]["id"]: i for i in self.active}
        killed = {by_id[k] for k in kills}
        # a killed track's match is void, and so is a match to a detection without a class
        matches = [(by_id[t], d) for t, d in matches if by_id[t] not in killed and det["labels"][d] >= 0]
        taken = {d for _, d in matches}
        D = len(det["labels"])
        det_id = np.full(D, -1, np.int32)
        newborn = [d for d in range(D) if det["labels"][d] >= 0 and d not in taken and (born is None or born[d] != 0)]
        new_active = []
        if newborn:
            for i, d in enumerate(newborn):
                new_active.append(len(self.tracks))
                self.tracks.append(dict(id=self.count + i, cls=[det["labels"][d]], boxes=[det["boxes"][d].copy()],
                                        scores=[det["scores"][d]], misses=0, absorbed=[(frame_no, d)]))
                det_id[d] = self.count + i
            self.count += len(newborn)
            self.store_new(det["xyz"][newborn], det["feats"][newborn], det["lengths"][newborn])
        for i, d in matches:
            t = self.tracks[i]
            t["cls"].append(det["labels"][d])
            t["boxes"].append(det["boxes"][d].copy())
            t["scores"].append(det["scores"][d])
            t["absorbed"].append((frame_no, d))
            if reset_on_match:
                t["misses"] = 0
            det_id[d] = t["id"]
            new_active.append(i)
        if matches:
            index, dets = [i for i, _ in matches], [d for _, d in matches]
            self.replace_old(index, det["xyz"][dets], det["feats"][dets], det["lengths"][dets])
        held = {i for i, _ in matches}
        for i in self.active:
            if i in held or i in killed:
                continue
            t = self.tracks[i]
            t["misses"] += 1
            if t["misses"] >= frame_limit:
                continue
            if propagate:
                t["boxes"].append(propagate_box(t["boxes"][-1], carry))
                t["scores"].append(F(t["scores"][-1] * F(0.01)))
                t["cls"].append(t["cls"][-1])
            new_active.append(i)
        self.active = new_active
        return det_id

    def live(self):
        """{track id: index} of the active tracks"""
        return {self.tracks[i]["id"]: i for i in self.active}


# ---- frames ---------------------------------------------------------------------------------------------------------------
def rigid(g, span=100.0):
    """a row-major 3 x 4 rigid motion (a turn about z and a small tilt, translation within +-span) and its inverse"""
    yaw, tilt = g.uniform(-np.pi, np.pi), g.uniform(-0.05, 0.05)
    cz, sz, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(tilt), np.sin(tilt)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    t = g.uniform(-span, span, 3)
    fwd = np.concatenate([R, t[:, None]], 1)
    inv = np.concatenate([R.T, -(R.T @ t)[:, None]], 1)
    return fwd.astype(F).reshape(12), inv.astype(F).reshape(12)


def det_boxes(g, D, W, span=100.0):
    b = np.zeros((D, W), F)
    b[:, :3] = g.uniform(-span, span, (D, 3))
    b[:, 3:6] = g.uniform(0.5, 5.0, (D, 3))
    b[:, 6] = g.uniform(-np.pi, np.pi, D)
    if W == 9:
        b[:, 7:9] = g.uniform(-10.0, 10.0, (D, 2))
    return b


def random_state(g, C, W, p_active=0.6):
    """a bank in mid-sequence: a random mixture of active and free slots; the free ones hold stale numbers"""
    st = new_state(C, W)
    act = g.random(C) < p_active
    n = int(act.sum())
    st["ids"][act] = g.permutation(3 * C)[:n]
    st["labels"][act] = g.integers(0, 3, n)
    st["lengths"] = g.integers(0, 6, C).astype(np.int32) * act
    st["boxes"] = det_boxes(g, C, W)
    st["scores"] = g.uniform(0.05, 1.0, C).astype(F)
    st["steps"] = g.integers(1, 9, C).astype(np.int32)
    st["misses"] = g.integers(0, 3, C).astype(np.int32)
    st["next_id"][0] = 3 * C + 5
    st["info"][0] = 77
    return st


def make_frame(g, st, D, W, masks=True, junk=True, p_match=0.6, p_valid=0.85, span=100.0):
    """-> dict(track_to_det, det_to_track, labels, lengths, boxes, scores, born, kill, intended): `intended` lists the
    (slot, detection) pairs the assignment really makes; everything else in the two maps is there to be ignored"""
    C = len(st["ids"])
    labels = np.where(g.random(D) < p_valid, g.integers(0, 3, D), -1).astype(np.int32)
    lengths = g.integers(0, 6, D).astype(np.int32)
    t2d, d2t = np.full(C, -1, np.int32), np.full(D, -1, np.int32)
    active, free = np.nonzero(st["ids"] >= 0)[0], np.nonzero(st["ids"] < 0)[0]
    pool = list(g.permutation(np.nonzero(labels >= 0)[0]))
    intended = []
    for s in active:
        if pool and g.random() < p_match:
            d = int(pool.pop())
            t2d[s], d2t[d] = d, s
            intended.append((int(s), d))
    if junk and D > 0:
        invalid = np.nonzero(labels < 0)[0]
        loose = [int(s) for s in active if t2d[s] < 0]
        if len(invalid) and loose:                           # both maps agree, but the detection has no class
            s = loose.pop()
            t2d[s], d2t[invalid[0]] = invalid[0], s
        if pool and len(free):                               # both maps agree, but the slot is free
            d = int(pool.pop())
            t2d[free[0]], d2t[d] = d, free[0]
        for d in range(D):                                   # a detection that names a track which does not name it
            if d2t[d] < 0 and g.random() < 0.3:
                d2t[d] = [C + 5, -3, int(g.integers(0, C))][int(g.integers(0, 3))]
                if 0 <= d2t[d] < C and t2d[d2t[d]] == d:
                    d2t[d] = -1
        for s in loose:                                      # a track that names a detection which does not name it
            if g.random() < 0.5:
                t2d[s] = [D + 2, -9, int(g.integers(0, D))][int(g.integers(0, 3))]
                if 0 <= t2d[s] < D and d2t[t2d[s]] == s:
                    t2d[s] = -1
    born = (g.random(D) < 0.8).astype(np.int32) if masks else None
    kill = (g.random(C) < 0.1).astype(np.int32) if masks else None
    return dict(track_to_det=t2d, det_to_track=d2t, labels=labels, lengths=lengths, boxes=det_boxes(g, D, W, span),
                scores=g.uniform(0.05, 1.0, D).astype(F), born=born, kill=kill, intended=intended)


def plan_frame(st, fr, **args):
    return plan(st, fr["track_to_det"], fr["det_to_track"], fr["labels"], fr["lengths"], fr["boxes"], fr["scores"],
                born=fr["born"], kill=fr["kill"], **args)
