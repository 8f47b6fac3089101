"""Scoring the tracker against ground-truth tracks on the device (include/pcr.h section A7, csrc/truth_kernels.hip).

`ReIDNet.track_step` turns a sweep and boxes into track ids without a host read; the reference's tracker then goes to the
host to find out whether they are right: get_iou_idx matches detections to ground-truth boxes through scipy on a host
copy (trackers/deprecated/virtual_tracker.py:186-229), TrackingDecisionModifier derives the frame's true decisions with
np.intersect1d (tracking_decision_modifier.py:62-129), get_stats counts them (:132-172) and update_gt_track_mapping carries
every track's ground-truth id and time to end to the next frame (virtual_tracker.py:297-347).  `TruthBook` is that half
with fixed shapes: a cost launch, the linear assignment of pcr_amd/associate.py, one launch before the bank's update and
one after it, no host read and the same bits on every run, so a scored frame can still be captured in a HIP graph.
`metrics()` is the one host read.  INTEGRATION.md ("2g. Ground truth") has the mapping.
"""
import ctypes

import torch

from . import _lib as L
from . import abi
from . import associate as A
from . import nms as NMS

KINDS = ("det_match", "det_newborn", "det_false_positive", "track_false_negative", "track_false_positive")
STATS = 24                                                  # PCR_TRUTH_STATS
TOTAL_GT, TOTAL_CORRECT = 15, 16
MOT = dict(frames=17, gt_total=18, tp=19, fp=20, fn=21, switches=22, untracked=23)
_WHO = "pcr_amd.truth"


def truth_ok(C, D, G, W=9, gt_cap=1):
    """whether the section-A7 entry points take C slots, D detections, G ground-truth boxes of width W and gt_cap ids"""
    return bool(L.load().pcr_truth_ok(int(C), int(D), int(G), int(W), int(gt_cap)))


def cost(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, gt_cap, iou=None, out=None):
    """pcr_truth_cost_f32: det_boxes (D, W), det_labels (D,), gt_boxes (G, W), gt_labels / gt_ids (G,) [, iou (D, G)] ->
    cost (D, G) float32, every element written: the BEV centre distance (or -iou) plus 10000 where the labels differ or a
    side is padding (a label < 0, a ground-truth id outside [0, gt_cap))"""
    f32, i32 = torch.float32, torch.int32
    det_boxes = L.tensor(det_boxes, _WHO, "det_boxes", f32, shape=(None, None))
    D, W = det_boxes.shape
    gt_boxes = L.tensor(gt_boxes, _WHO, "gt_boxes", f32, shape=(None, W))
    G = gt_boxes.shape[0]
    det_labels = L.tensor(det_labels, _WHO, "det_labels", i32, shape=(D,))
    gt_labels, gt_ids = L.tensor(gt_labels, _WHO, "gt_labels", i32, shape=(G,)), L.tensor(gt_ids, _WHO, "gt_ids", i32, shape=(G,))
    iou = L.tensor(iou, _WHO, "iou", f32, shape=(D, G), optional=True)
    L.require(truth_ok(1, D, G, W, gt_cap), _WHO, "D=%d G=%d W=%d gt_cap=%d is out of range (pcr_truth_ok)", D, G, W, gt_cap)
    out = L.out_tensor(out, _WHO, "out", f32, (D, G), det_boxes.device)
    L.require_cuda(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, iou, out)
    L.run.pcr_truth_cost_f32(det_boxes, det_labels, gt_boxes, gt_labels, gt_ids, iou, out, D, G, W, int(gt_cap),
                             L.stream_ptr())
    return out


def _params(t, gt_cap, skip_empty, forced=False):
    """the parameter block over a dict of explicit tensors (None = NULL); shapes are read off ids, det_labels, gt_labels"""
    for k in ("ids", "det_labels", "gt_labels"):
        L.require(isinstance(t.get(k), torch.Tensor) and t[k].dim() == 1, _WHO, "%s must be a 1-D tensor", k)
    C, D, G = t["ids"].shape[0], t["det_labels"].shape[0], t["gt_labels"].shape[0]
    L.require(truth_ok(C, D, G, 7, gt_cap), _WHO, "C=%d D=%d G=%d gt_cap=%d is out of range (pcr_truth_ok)", C, D, G, gt_cap)
    sizes = dict(ids=C, slot_gt=C, slot_tte=C, gt_last=int(gt_cap), stats=STATS, col4row=D, row4col=G, info=1, cost=D * G,
                 thresh=1, gt_labels=G, gt_ids=G, gt_tte=G, det_labels=D, track_to_det=C, det_to_track=D, born=D, kill=C,
                 det_gt=D, true_t2d=C, true_d2t=D, det_truth=D, track_truth=C, det_slot=D, det_id=D)
    p = abi.TruthParams()
    p.C, p.D, p.G, p.gt_cap, p.skip_empty, p.forced = C, D, G, int(gt_cap), int(bool(skip_empty)), int(bool(forced))
    return abi.fill(p, t, sizes, who=_WHO)


def decide(tensors, gt_cap, skip_empty=True, forced=False):
    """pcr_truth_decide_i32 on explicit tensors: a dict with ids, slot_gt, slot_tte (C,), stats (24,), col4row (D,), row4col
    (G,), info (1,), cost (D, G), thresh (1,), gt_labels / gt_ids / gt_tte (G,), det_labels (D,), track_to_det (C,),
    det_to_track (D,) [, born (D,), kill (C,)] and the outputs det_gt, true_d2t, det_truth (D,), true_t2d, track_truth
    (C,).  stats is added to, the outputs are written.  forced: the frame applies the true decisions (teacher forcing), and
    they are what is counted; the tracker's own maps and masks are not read."""
    L.run.pcr_truth_decide_i32(ctypes.byref(_params(tensors, gt_cap, skip_empty, forced)), L.stream_ptr())


def record(tensors, gt_cap):
    """pcr_truth_record_i32 on explicit tensors: ids (C,) as they are after the update and the track NMS, the book slot_gt,
    slot_tte (C,), gt_last (gt_cap,), stats (24,), gt_labels / gt_ids / gt_tte (G,), det_labels (D,), decide's det_gt (D,)
    and track_truth (C,), the plan's det_slot and det_id (D,).  The book is updated in place."""
    L.run.pcr_truth_record_i32(ctypes.byref(_params(tensors, gt_cap, False)), L.stream_ptr())


def metrics_of(stats):
    """the stats table (a sequence of PCR_TRUTH_STATS ints on the host) -> the reference's recall_ / precision_ / f1_ per
    decision and acc_total (get_scene_metrics, virtual_tracker.py:1008-1017, with its 1e-12), mota and the raw counters"""
    s = [int(v) for v in stats]
    out = {}
    for k, name in enumerate(KINDS):
        gt, correct, pred = (float(v) for v in s[3 * k:3 * k + 3])
        r, p = correct / (gt + 1e-12), correct / (pred + 1e-12)
        out["recall_" + name], out["precision_" + name], out["f1_" + name] = r, p, 2 * ((r * p) / (r + p + 1e-12))
        out[name + "_gt"], out[name + "_correct"], out[name + "_num_pred"] = s[3 * k], s[3 * k + 1], s[3 * k + 2]
    out["total_gt"], out["total_correct"] = s[TOTAL_GT], s[TOTAL_CORRECT]
    out["acc_total"] = s[TOTAL_CORRECT] / (s[TOTAL_GT] + 1e-12)
    for name, i in MOT.items():
        out[name] = s[i]
    out["mota"] = 1.0 - (out["fn"] + out["fp"] + out["switches"]) / out["gt_total"] if out["gt_total"] else float("nan")
    return out


class TruthBook:
    """The ground-truth side of a `TrackBank`: per slot the ground-truth track id its track was last seen as and that
    track's time to end (`slot_gt`, `slot_tte`), per ground-truth id the tracker id it was last given (`gt_last`), the
    counters (`stats`) and the frame buffers, all on the bank's device.

    max_gt     the number of ground-truth boxes a frame is padded to (label -1 is padding)
    gt_cap     ground-truth track ids lie in [0, gt_cap); a box with any other id is padding
    kind       "centre": BEV centre distance, a true positive is closer than `thresh` metres (Center2DRange);
               "iou": axis-aligned IoU of the nearest_bev boxes, a true positive overlaps by more than `thresh`
               (tp_threshold; the device float holds -thresh, as the cost is -iou)
    skip_empty the reference's quirk: a decision kind without a true instance in a frame adds nothing that frame

    Padding rows and real columns.  With max_gt == bank.max_dets, a frame with fewer valid detections than valid
    ground-truth boxes (any missed object) leaves padding ROWS to real columns at 10000 + the box's distance from the
    origin, and which columns are left to them is part of the optimum: a missed object roughly behind a detected one,
    seen from the origin, can pull that detection away from its own box (include/pcr.h, "Validity").  It is avoidable:
    with max_gt >= bank.max_dets + (the most valid ground-truth boxes of a frame) every row finds a padding column of
    its own at a flat 10000, and no padding row ever takes a real column.

    Every method but `metrics` launches on the current stream, returns the book's own fixed-shape tensors (overwritten by
    the next frame) and never reads the device.  The book's own steps write into buffers made here; what still makes a
    tensor per call is the conversion of int64 labels or masks, as everywhere in `track_step` (inside a captured graph
    such tensors come from the graph's private pool).  Deliberate differences from the reference are listed in
    INTEGRATION.md."""

    def __init__(self, bank, max_gt, gt_cap, kind="centre", thresh=2.0, skip_empty=True):
        from . import tracks as TR
        L.require(isinstance(bank, TR.TrackBank), _WHO, "bank must be a pcr_amd.tracks.TrackBank")
        L.require(kind in ("centre", "iou"), _WHO, "kind must be 'centre' or 'iou', got %r", kind)
        C, D, G = bank.capacity, bank.max_dets, int(max_gt)
        L.require(truth_ok(C, D, G, bank.box_width, gt_cap), _WHO,
                  "capacity=%d max_dets=%d max_gt=%d gt_cap=%d is out of range (pcr_truth_ok)", C, D, G, gt_cap)
        self.bank, self.max_gt, self.gt_cap, self.kind, self.skip_empty = bank, G, int(gt_cap), kind, bool(skip_empty)
        dev = bank.device
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.slot_gt, self.slot_tte, self.gt_last, self.stats = i32(C), i32(C), i32(self.gt_cap), i32(STATS)
        self.thresh = torch.full((1,), float(thresh) if kind == "centre" else -float(thresh), dtype=torch.float32, device=dev)
        self.gt_boxes, self.gt_labels, self.gt_ids, self.gt_tte = f32(G, bank.box_width), i32(G), i32(G), i32(G)
        self.cost, self.col4row, self.row4col, self.info = f32(D, G), i32(1, D), i32(1, G), i32(1)
        self.det_gt, self.true_d2t, self.det_truth = i32(D), i32(D), i32(D)
        self.true_t2d, self.track_truth = i32(C), i32(C)
        self._born, self._kill = i32(D), i32(C)
        if kind == "iou":
            self._det7, self._gt7, self._det_bev, self._gt_bev, self._iou = f32(D, 7), f32(G, 7), f32(D, 5), f32(G, 5), f32(D, G)
        self._det_labels = self._det_id = None
        self.reset()

    def reset(self):
        """an empty book: no slot is booked, no id was seen, every counter 0"""
        for t in (self.slot_gt, self.slot_tte, self.gt_last):
            t.fill_(-1)
        self.stats.zero_()
        self._det_id = None                                 # (an IdentityBook's record follows a record of THIS book's life)

    def _load(self, gt):
        """the frame's ground truth into the book's buffers, padded to max_gt with label -1"""
        boxes = L.tensor(gt["boxes"], _WHO, "gt['boxes']", torch.float32, shape=(None, self.bank.box_width), copy=True)
        n = boxes.shape[0]
        L.require(n <= self.max_gt, _WHO, "%d ground-truth boxes, the book was made for %d", n, self.max_gt)
        L.require_cuda(boxes)
        self.gt_boxes.zero_()
        self.gt_boxes[:n].copy_(boxes)
        for k, buf in (("labels", self.gt_labels), ("ids", self.gt_ids), ("tte", self.gt_tte)):
            t = gt[k]
            L.require(isinstance(t, torch.Tensor) and t.shape == (n,), _WHO, "gt[%r] must be a (%d,) tensor", k, n)
            L.require_cuda(t)
            L.require(t.dtype in (torch.int32, torch.int64), _WHO, "gt[%r] must be an integer tensor", k)
            buf.fill_(-1)
            buf[:n].copy_(t)

    def match(self, det_boxes, det_labels, gt):
        """get_iou_idx without its threshold: det_boxes (max_dets, W), det_labels (max_dets,) int32 (-1 = padding), gt =
        dict(boxes (G <= max_gt, W), labels, ids, tte (G,)) -> (col4row (max_dets,), row4col (max_gt,), info (1,)) of the
        linear assignment over the cost (max_dets, max_gt), which stays in `self.cost`"""
        D, W = self.bank.max_dets, self.bank.box_width
        L.require(isinstance(det_boxes, torch.Tensor) and det_boxes.shape == (D, W), _WHO, "det_boxes must be (%d, %d)", D, W)
        self._load(gt)
        iou = None
        if self.kind == "iou":
            self._det7.copy_(det_boxes[:, :7])
            self._gt7.copy_(self.gt_boxes[:, :7])
            NMS.nearest_bev(self._det7, out=self._det_bev)
            NMS.nearest_bev(self._gt7, out=self._gt_bev)
            iou = NMS.iou_bev(self._det_bev, self._gt_bev, kind="axis", out=self._iou)
        cost(det_boxes, det_labels, self.gt_boxes, self.gt_labels, self.gt_ids, self.gt_cap, iou=iou, out=self.cost)
        A.linear_assignment(self.cost, out=(self.col4row, self.row4col, self.info))
        return self.col4row[0], self.row4col[0], self.info

    def _tensors(self, det_labels):
        return dict(ids=self.bank.ids, slot_gt=self.slot_gt, slot_tte=self.slot_tte, gt_last=self.gt_last, stats=self.stats,
                    gt_labels=self.gt_labels, gt_ids=self.gt_ids, gt_tte=self.gt_tte, det_labels=det_labels,
                    det_gt=self.det_gt, track_truth=self.track_truth)

    def decide(self, assignment, det_labels, born=None, kill=None, forced=False):
        """pcr_truth_decide_i32 over the bank as it is BEFORE `bank.update`, after `match`: assignment = the tracker's own
        (track_to_det (capacity,), det_to_track (max_dets,)) or a dict holding them, born / kill its masks as
        `TrackBank.update` takes them; forced: the frame applies `forced()`'s decisions, and the counters score those
        (every kind then has gt == correct == num_pred) -> dict(det_gt, true_track_to_det, true_det_to_track, det_truth,
        track_truth)"""
        if isinstance(assignment, dict):
            t2d, d2t = assignment["track_to_det"], assignment["det_to_track"]
        else:
            t2d, d2t = assignment
        C, D = self.bank.capacity, self.bank.max_dets
        vec = lambda t, n, name: L.tensor(t, _WHO, name, torch.int32, shape=(n,), optional=True, cast_int64=True, copy=True)
        det_labels = vec(det_labels, D, "det_labels")
        t2d, d2t = vec(t2d, C, "track_to_det"), vec(d2t, D, "det_to_track")
        born, kill = vec(born, D, "born"), vec(kill, C, "kill")
        t = self._tensors(det_labels)
        t.update(col4row=self.col4row, row4col=self.row4col, info=self.info, cost=self.cost, thresh=self.thresh,
                 track_to_det=t2d, det_to_track=d2t, born=born, kill=kill, true_t2d=self.true_t2d, true_d2t=self.true_d2t,
                 det_truth=self.det_truth)
        decide(t, self.gt_cap, self.skip_empty, forced)
        self._det_labels = det_labels
        return dict(det_gt=self.det_gt, true_track_to_det=self.true_t2d, true_det_to_track=self.true_d2t,
                    det_truth=self.det_truth, track_truth=self.track_truth)

    def forced(self):
        """teacher forcing in mode 'gt': decide's truth as `TrackBank.update` takes decisions ->
        ((track_to_det, det_to_track), born, kill)"""
        torch.eq(self.det_truth, 1, out=self._born)
        torch.eq(self.track_truth, 2, out=self._kill)
        return (self.true_t2d, self.true_d2t), self._born, self._kill

    def record(self, det_slot, det_id):
        """pcr_truth_record_i32 AFTER `bank.update` and `bank.suppress`: det_slot / det_id (max_dets,) as the update
        returned them.  The book moves on one frame and the MOT counters are added to."""
        L.require(self._det_labels is not None, _WHO, "record follows decide")
        t = self._tensors(self._det_labels)
        t.update(det_slot=det_slot, det_id=det_id)
        record(t, self.gt_cap)
        self._det_id = det_id                               # (what an IdentityBook over this book records next)

    def metrics(self):
        """THE host read: see `metrics_of`"""
        return metrics_of(self.stats.cpu().tolist())
