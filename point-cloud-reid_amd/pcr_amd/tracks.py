"""Track state on the device (include/pcr.h sections A5 and A11, csrc/track_kernels.hip).

`ReIDNet.associate` ends with `track_to_det` / `det_to_track`; the reference's tracker then goes to the host to decide
what is stored where: `PointFeatureSet` grows by `torch.cat` and replaces through a `torch.where` of data-dependent shape
(trackers/deprecated/tracking_feature_set.py:11-63), `TrackingUpdater.__call__` walks `decisions[...].cpu().numpy()`
and lists of `Track` objects (tracking_updater.py:22-98), missed tracks are propagated in numpy (track.py:116-183) and
the distance prior copies the detections to the host and back (virtual_tracker.py:287-295).  `TrackBank` is that state
with a fixed capacity: every step is a fixed-shape launch without a host read and with the same bits on every run, so a
whole tracker frame can be captured in a HIP graph.  INTEGRATION.md ("2e. Track state") has the mapping;
`ReIDNet.track_step` chains a frame.

`UpdateRules`, `plan_rules` / `TrackBank.update_rules` and `SceneLog` (section A11) run the update the way the reference's
updater is configured: an `update_config` with output / active / decom flags per decision, a fixed-shape table of the
tracks the frame outputs, and a device-side log of those rows that a result file is written from.
"""
import ctypes

import torch

from . import _lib as L
from . import abi
from . import nms as NMS


_WHO = "pcr_amd.tracks"
STATE = ("lengths", "boxes", "scores", "labels", "ids", "steps", "misses", "next_id", "info")
TABLE = ("out_valid", "out_ids", "out_labels", "out_scores", "out_boxes", "out_flags")
RULE_OUTPUT, RULE_ACTIVE, RULE_DECOM = 1, 2, 4              # PCR_RULE_*
TRK_KEEP, TRK_MISS = 0, 1                                   # PCR_TRK_*
MAX_DECISIONS = 4                                           # PCR_ASSOC_MAX_DECISIONS
_RULE_KEYS = ("match", "det_newborn", "det_false_positive", "track_false_positive", "track_false_negative")
_RULE_FLAGS = (("output", RULE_OUTPUT), ("active", RULE_ACTIVE), ("decom", RULE_DECOM))


def bank_ok(C, D, W=9, feat_floats=0, xyz_floats=0):
    """whether the section-A5 entry points take a bank of C slots, D detections, box width W and these row sizes"""
    return bool(L.load().pcr_bank_ok(int(C), int(D), int(W), int(feat_floats), int(xyz_floats)))


def _vec(t, dtype, n, name):
    """a contiguous (n,) tensor of dtype (int64 labels / lengths are converted on the device), or None"""
    return L.tensor(t, _WHO, name, dtype, shape=(n,), optional=True, cast_int64=dtype is torch.int32, copy=True)


def plan(state, track_to_det, det_to_track, det_labels, det_lengths, det_boxes, det_scores, src, det_slot, det_id,
         born=None, kill=None, carry=None, frame_limit=10, replace_all=False, reset_on_match=False, propagate=True):
    """pcr_bank_plan_i32 on explicit tensors.  state = dict(lengths, boxes, scores, labels, ids, steps, misses, next_id,
    info), updated in place; src (C,), det_slot (D,), det_id (D,) are written."""
    L.require(isinstance(state, dict) and all(k in state for k in STATE), _WHO, "state must hold %s", ", ".join(STATE))
    boxes = state["boxes"]
    L.require(isinstance(boxes, torch.Tensor) and boxes.dim() == 2, _WHO, "boxes must be (C, W)")
    L.require(isinstance(det_boxes, torch.Tensor) and det_boxes.dim() == 2, _WHO, "det_boxes must be (D, W)")
    (C, W), D = boxes.shape, det_boxes.shape[0]
    L.require(bank_ok(C, D, W), _WHO, "C=%d D=%d W=%d is out of range (pcr_bank_ok)", C, D, W)
    L.require(int(frame_limit) >= 1, _WHO, "frame_limit must be at least 1")
    sizes = dict(lengths=C, boxes=C * W, scores=C, labels=C, ids=C, steps=C, misses=C, next_id=1, info=1, track_to_det=C,
                 det_to_track=D, det_labels=D, det_lengths=D, det_boxes=D * W, det_scores=D, born=D, kill=C, carry=12, src=C,
                 det_slot=D, det_id=D)
    p = abi.BankParams()
    p.C, p.D, p.W = C, D, W
    p.frame_limit, p.replace_all, p.reset_on_match, p.propagate = int(frame_limit), int(bool(replace_all)), \
        int(bool(reset_on_match)), int(bool(propagate))
    abi.fill(p, dict({k: state[k] for k in STATE}, track_to_det=track_to_det, det_to_track=det_to_track,
                     det_labels=det_labels, det_lengths=det_lengths, det_boxes=det_boxes, det_scores=det_scores, born=born,
                     kill=kill, carry=carry, src=src, det_slot=det_slot, det_id=det_id), sizes, who=_WHO)
    L.run.pcr_bank_plan_i32(ctypes.byref(p), L.stream_ptr())
    return src, det_slot, det_id


class UpdateRules:
    """The reference's `update_config` (tracking_updater.py:14-19, :189-203) as rule words for one set of decisions.

    update_config  the keys match, det_newborn, det_false_positive, track_false_positive, track_false_negative, each
                   dict(output=, active=, decom=); every decision name in use and `match` need an entry
    det_names, trk_names  the sorted decision names of the frame, as `pcr_amd.frame.decision_set` produces them
    -> match_rule, det_rule (dd,), trk_rule (td,), trk_kind (td,): `track_false_negative` is TRK_MISS (the track is
    propagated), every other tracking decision TRK_KEEP.  active and decom together are refused, as the reference does."""

    def __init__(self, update_config, det_names=(), trk_names=()):
        L.require(isinstance(update_config, dict), _WHO, "update_config must be a dict of dict(output=, active=, decom=)")
        det_names, trk_names = list(det_names), list(trk_names)
        L.require(len(det_names) <= MAX_DECISIONS and len(trk_names) <= MAX_DECISIONS, _WHO,
                  "at most %d decisions per side", MAX_DECISIONS)
        for k in update_config:
            L.require(k in _RULE_KEYS, _WHO, "update_config has the unknown key %r (known: %s)", k, ", ".join(_RULE_KEYS))
        words = {}
        for k, cfg in update_config.items():
            L.require(isinstance(cfg, dict) and set(cfg) == {"output", "active", "decom"}, _WHO,
                      "update_config[%r] must be dict(output=, active=, decom=)", k)
            L.require(not (cfg["active"] and cfg["decom"]), _WHO, "update_config[%r]: cannot be both active and decom", k)
            words[k] = sum(bit for name, bit in _RULE_FLAGS if cfg[name])
        for k in ["match"] + det_names + trk_names:
            L.require(k in words, _WHO, "update_config has no entry for %r", k)
        self.det_names, self.trk_names = det_names, trk_names
        self.match_rule = words["match"]
        self.det_rule = tuple(words[k] for k in det_names)
        self.trk_rule = tuple(words[k] for k in trk_names)
        self.trk_kind = tuple(TRK_MISS if k == "track_false_negative" else TRK_KEEP for k in trk_names)

    @classmethod
    def from_words(cls, match_rule, det_rule=(), trk_rule=(), trk_kind=()):
        """the rule words themselves (RULE_OUTPUT | RULE_ACTIVE | RULE_DECOM) and the kinds of the tracking decisions, for
        up to MAX_DECISIONS decisions per side whatever their names"""
        r = cls.__new__(cls)
        r.det_names = r.trk_names = None
        r.match_rule, r.det_rule = int(match_rule), tuple(int(w) for w in det_rule)
        r.trk_rule, r.trk_kind = tuple(int(w) for w in trk_rule), tuple(int(k) for k in trk_kind)
        L.require(len(r.det_rule) <= MAX_DECISIONS and len(r.trk_rule) <= MAX_DECISIONS, _WHO,
                  "at most %d decisions per side", MAX_DECISIONS)
        L.require(len(r.trk_kind) == len(r.trk_rule) and set(r.trk_kind) <= {TRK_KEEP, TRK_MISS}, _WHO,
                  "trk_kind holds TRK_KEEP or TRK_MISS for every tracking decision")
        for w in (r.match_rule,) + r.det_rule + r.trk_rule:
            L.require(0 <= w < 8 and not (w & RULE_ACTIVE and w & RULE_DECOM), _WHO,
                      "a rule word is a sum of RULE_OUTPUT, RULE_ACTIVE, RULE_DECOM, never active and decom together")
        return r


def new_table(rows, W, device):
    """an output table of `rows` rows as pcr_bank_plan_rules_i32 writes it, every row invalid"""
    i32 = dict(dtype=torch.int32, device=device)
    f32 = dict(dtype=torch.float32, device=device)
    return dict(out_valid=torch.zeros(rows, **i32), out_ids=torch.full((rows,), -1, **i32),
                out_labels=torch.full((rows,), -1, **i32), out_scores=torch.zeros(rows, **f32),
                out_boxes=torch.zeros((rows, W), **f32), out_flags=torch.zeros(rows, **i32))


def plan_rules(state, track_to_det, det_to_track, det_labels, det_lengths, det_boxes, det_scores, det_decision,
               track_decision, rules, src, det_slot, det_id, info, table, carry=None, frame_limit=10, replace_all=False,
               reset_on_match=False):
    """pcr_bank_plan_rules_i32 on explicit tensors.  state = dict(lengths, boxes, scores, labels, ids, steps, misses,
    next_id), updated in place (an `info` entry is not looked at); det_decision (D,) / track_decision (C,) as
    associate.decode_assignment writes them; rules = an UpdateRules; src (C,), det_slot (D,), det_id (D,), info (2,) and
    table = dict(out_valid, out_ids, out_labels, out_scores, out_flags (C + D,), out_boxes (C + D, W)) are written."""
    keys = STATE[:-1]
    L.require(isinstance(state, dict) and all(k in state for k in keys), _WHO, "state must hold %s", ", ".join(keys))
    L.require(isinstance(rules, UpdateRules), _WHO, "rules must be a pcr_amd.tracks.UpdateRules")
    L.require(isinstance(table, dict) and set(table) == set(TABLE), _WHO, "table must hold %s", ", ".join(TABLE))
    boxes = state["boxes"]
    L.require(isinstance(boxes, torch.Tensor) and boxes.dim() == 2, _WHO, "boxes must be (C, W)")
    L.require(isinstance(det_boxes, torch.Tensor) and det_boxes.dim() == 2, _WHO, "det_boxes must be (D, W)")
    (C, W), D = boxes.shape, det_boxes.shape[0]
    dd, td = len(rules.det_rule), len(rules.trk_rule)
    L.require(bool(L.load().pcr_bank_rules_ok(C, D, W, dd, td)), _WHO,
              "C=%d D=%d W=%d with %d / %d decisions is out of range (pcr_bank_rules_ok)", C, D, W, dd, td)
    L.require(int(frame_limit) >= 1, _WHO, "frame_limit must be at least 1")
    R = C + D
    sizes = dict(lengths=C, boxes=C * W, scores=C, labels=C, ids=C, steps=C, misses=C, next_id=1, track_to_det=C,
                 det_to_track=D, det_labels=D, det_lengths=D, det_boxes=D * W, det_scores=D, det_decision=D,
                 track_decision=C, carry=12, src=C, det_slot=D, det_id=D, info=2, out_valid=R, out_ids=R, out_labels=R,
                 out_scores=R, out_boxes=R * W, out_flags=R)
    p = abi.BankRulesParams()
    p.C, p.D, p.W, p.dd, p.td = C, D, W, dd, td
    p.frame_limit, p.replace_all, p.reset_on_match = int(frame_limit), int(bool(replace_all)), int(bool(reset_on_match))
    p.match_rule = rules.match_rule
    for i, w in enumerate(rules.det_rule):
        p.det_rule[i] = w
    for j, (w, kind) in enumerate(zip(rules.trk_rule, rules.trk_kind)):
        p.trk_rule[j], p.trk_kind[j] = w, kind
    abi.fill(p, dict({k: state[k] for k in keys}, track_to_det=track_to_det, det_to_track=det_to_track,
                     det_labels=det_labels, det_lengths=det_lengths, det_boxes=det_boxes, det_scores=det_scores,
                     det_decision=det_decision, track_decision=track_decision, carry=carry, src=src, det_slot=det_slot,
                     det_id=det_id, info=info, **table), sizes, who=_WHO)
    L.run.pcr_bank_plan_rules_i32(ctypes.byref(p), L.stream_ptr())
    return src, det_slot, det_id, info, table


def move(src, det_feats, det_xyz, feats, xyz):
    """pcr_bank_move_f32: feats[s] = det_feats[src[s]] and xyz[s] = det_xyz[src[s]] for every slot with src[s] in [0, D);
    feats (C, ...), det_feats (D, ...) of one row shape, likewise xyz; rows must be dense (a view may start anywhere)"""
    f32 = torch.float32
    feats, det_feats = L.tensor(feats, _WHO, "feats", f32), L.tensor(det_feats, _WHO, "det_feats", f32)
    xyz, det_xyz = L.tensor(xyz, _WHO, "xyz", f32), L.tensor(det_xyz, _WHO, "det_xyz", f32)
    L.require(feats.dim() >= 1 and det_feats.dim() >= 1, _WHO, "feats and det_feats must have rows")
    C, D = feats.shape[0], det_feats.shape[0]
    src = L.tensor(src, _WHO, "src", torch.int32, shape=(C,))
    L.require(xyz.shape[:1] == (C,) and det_xyz.shape[:1] == (D,), _WHO, "feats / xyz must agree on C, det_feats / det_xyz on D")
    L.require(feats.shape[1:] == det_feats.shape[1:] and xyz.shape[1:] == det_xyz.shape[1:], _WHO,
              "the bank's rows and the detections' rows must have one shape")
    ff = feats[0].numel() if C else 0
    xf = xyz[0].numel() if C else 0
    L.require(bank_ok(C, D, 7, ff, xf), _WHO, "C=%d D=%d rows of %d and %d floats are out of range (pcr_bank_ok)", C, D, ff, xf)
    L.require_cuda(src, det_feats, det_xyz, feats, xyz)
    L.run.pcr_bank_move_f32(src, det_feats, det_xyz, feats, xyz, C, D, ff, xf, L.stream_ptr())


def distances(boxes, ids, det_boxes, carry_inv=None, out=None):
    """pcr_bank_dist_f32: boxes (C, W), ids (C,), det_boxes (D, W) -> (C, D) float32, every element written: the BEV
    distance between a stored centre and a detection's centre taken back into the previous frame by carry_inv (3 x 4,
    None = identity); 0 in a free slot's row.  It is the `dist=` operand of associate.association_cost."""
    f32 = torch.float32
    boxes = L.tensor(boxes, _WHO, "boxes", f32, shape=(None, None))
    C, W = boxes.shape
    det_boxes = L.tensor(det_boxes, _WHO, "det_boxes", f32, shape=(None, W))
    D = det_boxes.shape[0]
    ids = L.tensor(ids, _WHO, "ids", torch.int32, shape=(C,))
    carry_inv = L.tensor(carry_inv, _WHO, "carry_inv", f32, numel=12, optional=True)
    L.require(bank_ok(C, D, W), _WHO, "C=%d D=%d W=%d is out of range (pcr_bank_ok)", C, D, W)
    out = L.out_tensor(out, _WHO, "out", f32, (C, D), boxes.device)
    L.require_cuda(boxes, ids, det_boxes, carry_inv, out)
    L.run.pcr_bank_dist_f32(boxes, ids, det_boxes, carry_inv, out, C, D, W, L.stream_ptr())
    return out


def retire(mask, labels, ids, lengths):
    """pcr_bank_retire_i32: the active slots with mask != 0 are freed"""
    ids = L.tensor(ids, _WHO, "ids", torch.int32, shape=(None,))
    C = ids.shape[0]
    mask, labels, lengths = (L.tensor(t, _WHO, name, torch.int32, shape=(C,))
                             for t, name in ((mask, "mask"), (labels, "labels"), (lengths, "lengths")))
    L.require(bank_ok(C, 0), _WHO, "C=%d is out of range (pcr_bank_ok)", C)
    L.require_cuda(mask, labels, ids, lengths)
    L.run.pcr_bank_retire_i32(mask, labels, ids, lengths, C, L.stream_ptr())


class TrackBank:
    """`capacity` track slots and the room for `max_dets` detections of a frame, all on `device`.

    The features live in ONE gallery buffer (capacity + max_dets, *feat_shape): `feats` is `gallery[:capacity]` and a
    frame's detections are written to `det_feats` = `gallery[capacity:]` (likewise `gallery_xyz`, rows (feat_shape[1],
    3)), so that ReIDNet.match_gallery needs no per-frame torch.cat of the bank.  A slot is active iff ids >= 0; a free
    slot has label -1, which compare_pairs' class gate leaves out.  Differences from the reference's store (deliberate):
    the capacity is fixed and freed slots are reused, while PointFeatureSet grows for the whole scene; ids are numbered
    over the born tracks in detection order.

    Every method launches on the current stream, returns fixed-shape tensors and never reads the device.  The tensors
    `update` / `update_rules` return are the bank's own and are overwritten by the next update."""

    STATE = STATE

    def __init__(self, capacity, max_dets, feat_shape=(64, 128), box_width=9, device=None):
        C, D = int(capacity), int(max_dets)
        L.require(len(feat_shape) == 2 and min(feat_shape) >= 1, _WHO, "feat_shape must be (channels, points)")
        ch, n = int(feat_shape[0]), int(feat_shape[1])
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise L.PcrError("pcr_amd.tracks: the bank lives on an MI355X device (got %s); there is no CPU fallback" % device)
        L.require(bank_ok(C, D, box_width, ch * n, n * 3), _WHO,
                  "capacity=%d max_dets=%d box_width=%d feat_shape=%s is out of range (pcr_bank_ok)",
                  C, D, box_width, tuple(feat_shape))
        self.capacity, self.max_dets, self.box_width, self.feat_shape, self.device = C, D, int(box_width), (ch, n), device
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.gallery = torch.zeros((C + D, ch, n), **f32)
        self.gallery_xyz = torch.zeros((C + D, n, 3), **f32)
        self.feats, self.det_feats = self.gallery[:C], self.gallery[C:]
        self.xyz, self.det_xyz = self.gallery_xyz[:C], self.gallery_xyz[C:]
        self.lengths, self.labels, self.ids = torch.zeros(C, **i32), torch.zeros(C, **i32), torch.zeros(C, **i32)
        self.steps, self.misses = torch.zeros(C, **i32), torch.zeros(C, **i32)
        self.boxes, self.scores = torch.zeros((C, self.box_width), **f32), torch.zeros(C, **f32)
        self.next_id, self.rules_info = torch.zeros(1, **i32), torch.zeros(2, **i32)
        self.info = self.rules_info[:1]             # the drops of the last plan, whichever entry point made it
        self.table = new_table(C + D, self.box_width, device)
        self.src, self.det_slot, self.det_id = torch.zeros(C, **i32), torch.zeros(D, **i32), torch.zeros(D, **i32)
        self._dist = torch.zeros((C, D), **f32)
        self._track_scores, self._suppressed = torch.zeros(C, **f32), torch.zeros(C, **i32)
        self.reset()

    def state(self):
        return {k: getattr(self, k) for k in self.STATE}

    def reset(self):
        """every slot free, ids from 0 again"""
        for t in (self.gallery, self.gallery_xyz, self.lengths, self.steps, self.misses, self.boxes, self.scores,
                  self.next_id, self.rules_info):
            t.zero_()
        for t in (self.labels, self.ids, self.src, self.det_slot, self.det_id):
            t.fill_(-1)
        for k, t in self.table.items():
            t.fill_(-1) if k in ("out_ids", "out_labels") else t.zero_()

    def distances(self, det_boxes, carry_inv=None):
        """det_boxes (D <= max_dets, box_width) -> (capacity, D): see `distances`; the bank's own buffer when D == max_dets"""
        L.require(isinstance(det_boxes, torch.Tensor) and det_boxes.dim() == 2, _WHO, "det_boxes must be a (D, W) tensor")
        D = det_boxes.shape[0]
        L.require(D <= self.max_dets, _WHO, "%d detections, the bank was made for %d", D, self.max_dets)
        return distances(self.boxes, self.ids, det_boxes, carry_inv, out=self._dist if D == self.max_dets else None)

    def update(self, assignment, dets, born=None, kill=None, carry=None, frame_limit=10, replace_all=False,
               reset_on_match=False, propagate=True):
        """One frame: pcr_bank_plan_i32, then pcr_bank_move_f32.

        assignment  a dict with track_to_det (capacity,) and det_to_track (D,) as ReIDNet.associate returns them, or
                    that pair
        dets        a dict: labels, lengths (D,) int, boxes (D, box_width), scores (D,), and feats (D, *feat_shape) /
                    xyz (D, points, 3); without feats / xyz the first D rows of det_feats / det_xyz are the frame's
        born, kill  (D,) / (capacity,) int32 masks: the learned newborn and false-positive decisions; None = every
                    unmatched valid detection is born, no track is killed
        carry       (12,) or (3, 4) float32: previous sweep's frame -> the current one (None = identity)
        -> det_slot (D,), det_id (D,), info (1,)"""
        if isinstance(assignment, dict):
            t2d, d2t = assignment["track_to_det"], assignment["det_to_track"]
        else:
            t2d, d2t = assignment
        C = self.capacity
        boxes = L.tensor(dets["boxes"], _WHO, "dets['boxes']", torch.float32, shape=(None, self.box_width), copy=True)
        D = boxes.shape[0]
        L.require(D <= self.max_dets, _WHO, "%d detections, the bank was made for %d", D, self.max_dets)
        labels, lengths = _vec(dets["labels"], torch.int32, D, "dets['labels']"), _vec(dets["lengths"], torch.int32, D, "dets['lengths']")
        scores = _vec(dets["scores"], torch.float32, D, "dets['scores']")
        t2d, d2t = _vec(t2d, torch.int32, C, "track_to_det"), _vec(d2t, torch.int32, D, "det_to_track")
        born, kill = _vec(born, torch.int32, D, "born"), _vec(kill, torch.int32, C, "kill")
        feats, xyz = dets.get("feats"), dets.get("xyz")
        L.require((feats is None) == (xyz is None), _WHO, "dets['feats'] and dets['xyz'] come together")
        if feats is None:
            feats, xyz = self.det_feats[:D], self.det_xyz[:D]
        det_slot, det_id = self.det_slot[:D], self.det_id[:D]
        plan(self.state(), t2d, d2t, labels, lengths, boxes, scores, self.src, det_slot, det_id, born=born,
             kill=kill, carry=carry, frame_limit=frame_limit, replace_all=replace_all, reset_on_match=reset_on_match,
             propagate=propagate)
        move(self.src, feats, xyz, self.feats, self.xyz)
        return det_slot, det_id, self.info

    def update_rules(self, assignment, dets, det_decision, track_decision, rules, carry=None, frame_limit=10,
                     replace_all=False, reset_on_match=False):
        """One frame under the reference's update_config: pcr_bank_plan_rules_i32, then pcr_bank_move_f32.

        assignment, dets, carry, frame_limit, replace_all, reset_on_match  as in `update`
        det_decision (D,), track_decision (capacity,)  as associate.decode_assignment returns them
        rules       an UpdateRules over the frame's decision names
        -> det_slot (D,), det_id (D,), info (2,) = [newborns dropped for want of a slot, valid output rows], and the
        output table, a dict of out_valid, out_ids, out_labels, out_scores, out_flags (capacity + D,) and out_boxes
        (capacity + D, box_width): rows < capacity are the slots', row capacity + d is detection d's (a new track that
        took no slot).  The table is the bank's own and is overwritten by the next update_rules."""
        if isinstance(assignment, dict):
            t2d, d2t = assignment["track_to_det"], assignment["det_to_track"]
        else:
            t2d, d2t = assignment
        C = self.capacity
        boxes = L.tensor(dets["boxes"], _WHO, "dets['boxes']", torch.float32, shape=(None, self.box_width), copy=True)
        D = boxes.shape[0]
        L.require(D <= self.max_dets, _WHO, "%d detections, the bank was made for %d", D, self.max_dets)
        labels, lengths = _vec(dets["labels"], torch.int32, D, "dets['labels']"), _vec(dets["lengths"], torch.int32, D, "dets['lengths']")
        scores = _vec(dets["scores"], torch.float32, D, "dets['scores']")
        t2d, d2t = _vec(t2d, torch.int32, C, "track_to_det"), _vec(d2t, torch.int32, D, "det_to_track")
        ddec, tdec = _vec(det_decision, torch.int32, D, "det_decision"), _vec(track_decision, torch.int32, C, "track_decision")
        L.require(ddec is not None and tdec is not None, _WHO, "det_decision and track_decision are needed")
        feats, xyz = dets.get("feats"), dets.get("xyz")
        L.require((feats is None) == (xyz is None), _WHO, "dets['feats'] and dets['xyz'] come together")
        if feats is None:
            feats, xyz = self.det_feats[:D], self.det_xyz[:D]
        det_slot, det_id = self.det_slot[:D], self.det_id[:D]
        table = self.table if D == self.max_dets else {k: t[:C + D] for k, t in self.table.items()}
        plan_rules(self.state(), t2d, d2t, labels, lengths, boxes, scores, ddec, tdec, rules, self.src, det_slot, det_id,
                   self.rules_info, table, carry=carry, frame_limit=frame_limit, replace_all=replace_all,
                   reset_on_match=reset_on_match)
        move(self.src, feats, xyz, self.feats, self.xyz)
        return det_slot, det_id, self.rules_info, table

    def track_scores(self):
        """(capacity,) float32: steps + scores, the reference's `len(det_bboxes) + scores[-1]` (stale in a free slot)"""
        return torch.add(self.steps, self.scores, out=self._track_scores)

    def suppress(self, thresh):
        """The reference's track NMS after the update (tracking_updater.py:96): nms.suppress_tracks over the bank, then
        the suppressed active slots are freed.  A free slot has class -1 and so cannot suppress an active one.
        thresh: a Python float or a (1,) float32 device tensor.  -> suppressed (capacity,) int32"""
        NMS.suppress_tracks(self.boxes[:, :7], self.labels, self.track_scores(), thresh, out=self._suppressed)
        retire(self._suppressed, self.labels, self.ids, self.lengths)
        return self._suppressed


class SceneLog:
    """The device-side record a result file is written from (pcr_scene_log_append_i32): `rows_max` rows of frame, id,
    label, flags, score and box, filled by one `append` per frame from an output table of `rows_per_frame` rows
    (capacity + max_dets for a TrackBank's).  The frame number is a device counter, so a captured frame replays correctly;
    rows that do not fit are dropped and counted.  `records` is the only method that reads the device."""

    def __init__(self, rows_max, rows_per_frame, box_width=9, device=None):
        N, R, W = int(rows_max), int(rows_per_frame), int(box_width)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise L.PcrError("pcr_amd.tracks: the log lives on an MI355X device (got %s); there is no CPU fallback" % device)
        L.require(bool(L.load().pcr_scene_log_ok(N, R, W)), _WHO,
                  "rows_max=%d rows_per_frame=%d box_width=%d is out of range (pcr_scene_log_ok)", N, R, W)
        self.rows_max, self.rows_per_frame, self.box_width, self.device = N, R, W, device
        i32 = dict(dtype=torch.int32, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        self.frame, self.id, self.label, self.flags = (torch.zeros(N, **i32) for _ in range(4))
        self.score, self.box = torch.zeros(N, **f32), torch.zeros((N, W), **f32)
        self._counters = torch.zeros(3, **i32)
        self.cursor, self.dropped, self.frame_no = self._counters[0:1], self._counters[1:2], self._counters[2:3]

    def reset(self):
        """an empty log, frame 0 next (the rows are left as they are: `records` trims to the cursor)"""
        self._counters.zero_()

    def append(self, table):
        """table: dict(out_valid, out_ids, out_labels, out_scores, out_flags (rows_per_frame,), out_boxes (rows_per_frame,
        box_width)), as TrackBank.update_rules returns it"""
        L.require(isinstance(table, dict) and set(table) == set(TABLE), _WHO, "table must hold %s", ", ".join(TABLE))
        N, R, W = self.rows_max, self.rows_per_frame, self.box_width
        p = abi.SceneLogParams()
        p.rows_max, p.R, p.W = N, R, W
        sizes = dict(in_valid=R, in_ids=R, in_labels=R, in_scores=R, in_boxes=R * W, in_flags=R, frame=N, id=N, label=N,
                     flags=N, score=N, box=N * W, cursor=1, dropped=1, frame_no=1)
        abi.fill(p, dict(in_valid=table["out_valid"], in_ids=table["out_ids"], in_labels=table["out_labels"],
                         in_scores=table["out_scores"], in_boxes=table["out_boxes"], in_flags=table["out_flags"],
                         frame=self.frame, id=self.id, label=self.label, flags=self.flags, score=self.score, box=self.box,
                         cursor=self.cursor, dropped=self.dropped, frame_no=self.frame_no), sizes, required=tuple(sizes),
                 who=_WHO)
        L.run.pcr_scene_log_append_i32(ctypes.byref(p), L.stream_ptr())

    def records(self):
        """-> dict of numpy columns frame, id, label, flags, score, box trimmed to the rows written, and the ints
        dropped (rows lost to a full log) and frames (appends so far)"""
        n, dropped, frames = self._counters.tolist()
        cols = {k: getattr(self, k)[:n].cpu().numpy() for k in ("frame", "id", "label", "flags", "score", "box")}
        return dict(cols, dropped=dropped, frames=frames)
