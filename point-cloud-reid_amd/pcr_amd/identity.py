"""Identity preservation on the device (include/pcr.h section A9, csrc/ident_kernels.hip).

`TruthBook` counts a frame's decisions and the MOT counters; MOTA hardly moves when a tracker swaps two identities half-way
through a scene, and `switches` counts that event once, however long the wrong identity is then kept.  `IdentityBook` keeps
what answers "did an object keep one identity over its whole life?": per ground-truth track its presence, tracked frames,
fragments and gaps, and the co-occurrence counts of ground-truth ids and tracker ids; at the end of a scene the global
identity assignment (the linear assignment of pcr_amd/associate.py over the compacted counts) gives IDTP, and a persistent
64-bit table pools scene after scene.  One launch per frame, four entry points per scene, fixed shapes, no host read and the
same bits on every run, so a frame with it can still be captured in a HIP graph.  `metrics()` is the one host read.
INTEGRATION.md ("2i. Identity metrics") lists the deliberate choices.
"""
import ctypes

import torch

from . import _lib as L
from . import abi
from . import associate as A

TRACK_COLS = ("present", "tracked", "frags", "first_gap", "longest_gap", "cur_gap", "ever", "last")   # PCR_IDENT_PRESENT ..
TOTALS = dict(frames=0, gt_total=1, pred_total=2, tp=3, dropped_gt=4, dropped_id=5)                  # PCR_IDENT_T_*
N_TOTALS, N_COUNTS = 8, 4
COUNTS = dict(n_rows=0, n_cols=1, max_count=2)
TABLE = ("idtp", "frames", "gt_total", "pred_total", "tp", "tracks", "mt", "pt", "ml", "frag", "tid_sum", "lgd_sum",
         "overflow", "inexact", "dropped_gt", "dropped_id")                                         # PCR_IDENT_IDTP ..
_WHO = "pcr_amd.identity"


def ident_ok(D, G, gt_cap, gt_rows, id_cap, max_rows=1, max_cols=1):
    """whether the section-A9 entry points take D detections, G ground-truth boxes with ids in [0, gt_cap), a
    (gt_rows, id_cap) co-occurrence matrix and a (max_rows, max_cols) assignment"""
    return bool(L.load().pcr_ident_ok(int(D), int(G), int(gt_cap), int(gt_rows), int(id_cap), int(max_rows), int(max_cols)))


def record(tensors, gt_cap, gt_rows, id_cap):
    """pcr_ident_record_i32 on explicit tensors: a dict with det_labels, det_gt, det_id (D,), gt_labels, gt_ids (G,), cost
    (D, G) float32 and the scene state cooc (gt_rows, id_cap), gt_track (gt_rows, 8), totals (8,) int32, dist_sum (1,)
    float64.  The scene state is added to in place."""
    t = tensors
    for k in ("det_labels", "gt_labels"):
        L.require(isinstance(t.get(k), torch.Tensor) and t[k].dim() == 1, _WHO, "%s must be a 1-D tensor", k)
    D, G = t["det_labels"].shape[0], t["gt_labels"].shape[0]
    L.require(ident_ok(D, G, gt_cap, gt_rows, id_cap), _WHO, "D=%d G=%d gt_cap=%d gt_rows=%d id_cap=%d is out of range (pcr_ident_ok)",
              D, G, gt_cap, gt_rows, id_cap)
    sizes = dict(det_labels=D, det_gt=D, det_id=D, gt_labels=G, gt_ids=G, cost=D * G, cooc=gt_rows * id_cap,
                 gt_track=gt_rows * len(TRACK_COLS), totals=N_TOTALS, dist_sum=1)
    p = abi.IdentParams()
    p.D, p.G, p.gt_cap, p.gt_rows, p.id_cap = D, G, int(gt_cap), int(gt_rows), int(id_cap)
    L.run.pcr_ident_record_i32(ctypes.byref(abi.fill(p, t, sizes, required=sizes, who=_WHO)), L.stream_ptr())


def _close_params(t, gt_rows, id_cap, max_rows, max_cols, required):
    L.require(ident_ok(0, 0, 1, gt_rows, id_cap, max_rows, max_cols), _WHO,
              "gt_rows=%d id_cap=%d max_rows=%d max_cols=%d is out of range (pcr_ident_ok)", gt_rows, id_cap, max_rows, max_cols)
    sizes = dict(cooc=gt_rows * id_cap, gt_track=gt_rows * len(TRACK_COLS), totals=N_TOTALS, dist_sum=1,
                 flags=gt_rows + id_cap, counts=N_COUNTS, row_list=max_rows, col_list=max_cols, cost=max_rows * max_cols,
                 col4row=max_rows, info=1, id_map=gt_rows, table=len(TABLE), dist_total=1)
    p = abi.IdentCloseParams()
    p.gt_rows, p.id_cap, p.max_rows, p.max_cols = int(gt_rows), int(id_cap), int(max_rows), int(max_cols)
    return abi.fill(p, t, sizes, required=required, who=_WHO)


def compact(tensors, gt_rows, id_cap, max_rows, max_cols):
    """pcr_ident_compact_f32 on explicit tensors: cooc (gt_rows, id_cap) -> flags (gt_rows + id_cap,) workspace, counts (4,),
    row_list (max_rows,), col_list (max_cols,) int32 and cost (max_rows, max_cols) float32, every element written"""
    p = _close_params(tensors, gt_rows, id_cap, max_rows, max_cols,
                      ("cooc", "flags", "counts", "row_list", "col_list", "cost"))
    L.run.pcr_ident_compact_f32(ctypes.byref(p), L.stream_ptr())


def score(tensors, gt_rows, id_cap, max_rows, max_cols):
    """pcr_ident_score_i32 on explicit tensors: the scene state, compact's counts, row_list and col_list, the assignment's
    col4row (max_rows,) and info (1,) -> id_map (gt_rows,) written; table (16,) int64 and dist_total (1,) float64 added to"""
    p = _close_params(tensors, gt_rows, id_cap, max_rows, max_cols,
                      ("cooc", "gt_track", "totals", "dist_sum", "counts", "row_list", "col_list", "col4row", "info", "id_map",
                       "table", "dist_total"))
    L.run.pcr_ident_score_i32(ctypes.byref(p), L.stream_ptr())


def metrics_of(table, dist_total, fp=0):
    """the pooled table (16 ints on the host), the pooled distance sum and the TruthBook's fp counter -> the identity
    metrics.  A ratio without a denominator is nan."""
    t = dict(zip(TABLE, (int(v) for v in table)))
    div = lambda a, b: a / b if b else float("nan")
    out = dict(idtp=t["idtp"], idfn=t["gt_total"] - t["idtp"], idfp=t["pred_total"] - t["idtp"])
    out["idp"], out["idr"] = div(t["idtp"], t["pred_total"]), div(t["idtp"], t["gt_total"])
    out["idf1"] = div(2 * t["idtp"], t["gt_total"] + t["pred_total"])
    for k in ("mt", "pt", "ml", "tracks", "frag", "frames", "gt_total", "pred_total", "tp"):
        out[k] = t[k]
    out["tid"], out["lgd"] = div(t["tid_sum"], t["tracks"]), div(t["lgd_sum"], t["tracks"])
    out["motp"] = div(float(dist_total), t["tp"])
    out["faf"] = div(int(fp), t["frames"])
    for k in ("overflow", "inexact", "dropped_gt", "dropped_id"):
        out[k] = t[k]
    return out


class IdentityBook:
    """The identity side of a `TruthBook`: the scene state (`cooc`, `gt_track`, `totals`, `dist_sum`), the buffers of the
    scene's assignment and the pooled `table` / `dist_total`, all on the book's device.

    truth_book the `TruthBook` whose frame buffers (`det_gt`, the padded ground truth, `cost`) `record` reads
    id_cap     tracker ids lie in [0, id_cap); a pair with a larger id is counted in dropped_id, not recorded
    gt_rows    ground-truth ids below gt_rows have a row (default: the book's gt_cap); others count in dropped_gt
    max_rows, max_cols   the most ground-truth ids / tracker ids of ONE scene that take part in the assignment; a scene
               with more sets `overflow` and adds no idtp

    Every method but `metrics` launches on the current stream and never reads the device."""

    def __init__(self, truth_book, id_cap, gt_rows=None, max_rows=256, max_cols=512):
        from . import truth as TU
        L.require(isinstance(truth_book, TU.TruthBook), _WHO, "truth_book must be a pcr_amd.truth.TruthBook")
        book = self.book = truth_book
        L.require(book.bank.device.type == "cuda", _WHO, "the book lives on %s; there is no CPU fallback", book.bank.device)
        gt_rows = book.gt_cap if gt_rows is None else int(gt_rows)
        D, G = book.bank.max_dets, book.max_gt
        L.require(ident_ok(D, G, book.gt_cap, gt_rows, id_cap, max_rows, max_cols), _WHO,
                  "gt_rows=%d id_cap=%d max_rows=%d max_cols=%d is out of range (pcr_ident_ok)", gt_rows, id_cap, max_rows, max_cols)
        self.gt_rows, self.id_cap, self.max_rows, self.max_cols = gt_rows, int(id_cap), int(max_rows), int(max_cols)
        dev = book.bank.device
        z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=dev)
        i32, f64 = torch.int32, torch.float64
        self.cooc, self.gt_track = z(i32, gt_rows, self.id_cap), z(i32, gt_rows, len(TRACK_COLS))
        self.totals, self.dist_sum = z(i32, N_TOTALS), z(f64, 1)
        self.flags, self.counts = z(i32, gt_rows + self.id_cap), z(i32, N_COUNTS)
        self.row_list, self.col_list = z(i32, self.max_rows), z(i32, self.max_cols)
        self.cost = z(torch.float32, self.max_rows, self.max_cols)
        self.col4row, self.row4col, self.info = z(i32, 1, self.max_rows), z(i32, 1, self.max_cols), z(i32, 1)
        self.id_map = torch.full((gt_rows,), -1, dtype=i32, device=dev)
        self.table, self.dist_total = z(torch.int64, len(TABLE)), z(f64, 1)

    def _scene(self):
        return dict(cooc=self.cooc, gt_track=self.gt_track, totals=self.totals, dist_sum=self.dist_sum)

    def record(self, det_id=None):
        """pcr_ident_record_i32 right AFTER `TruthBook.record`, over the book's buffers as they stand; det_id (max_dets,):
        the update's (default: the one the book's `record` was given)"""
        book = self.book
        L.require(book._det_labels is not None, _WHO, "record follows TruthBook.decide")
        if det_id is None:
            det_id = getattr(book, "_det_id", None)
            L.require(det_id is not None, _WHO, "record follows TruthBook.record")
        t = self._scene()
        t.update(det_labels=book._det_labels, det_gt=book.det_gt, det_id=det_id, gt_labels=book.gt_labels, gt_ids=book.gt_ids,
                 cost=book.cost)
        record(t, book.gt_cap, self.gt_rows, self.id_cap)

    def close_scene(self, reset=True):
        """the end of a scene: compaction, the linear assignment, the score launch (the pooled table is added to, `id_map`
        written), then `reset_scene` (reset=False leaves the scene state: closing it again would add it again).  No host
        read."""
        t = self._scene()
        t.update(flags=self.flags, counts=self.counts, row_list=self.row_list, col_list=self.col_list, cost=self.cost)
        shape = (self.gt_rows, self.id_cap, self.max_rows, self.max_cols)
        compact(t, *shape)
        A.linear_assignment(self.cost, out=(self.col4row, self.row4col, self.info))
        del t["flags"], t["cost"]
        t.update(col4row=self.col4row, info=self.info, id_map=self.id_map, table=self.table, dist_total=self.dist_total)
        score(t, *shape)
        if reset:
            self.reset_scene()

    def reset_scene(self):
        """an empty scene: no count, no track, the totals 0.  The pooled table stays."""
        for t in (self.cooc, self.gt_track, self.totals, self.dist_sum):
            t.zero_()

    def reset(self):
        """an empty scene and an empty pooled table"""
        self.reset_scene()
        self.table.zero_()
        self.dist_total.zero_()
        self.id_map.fill_(-1)

    def metrics(self):
        """THE host read -- the table, the distance sum's bits and the TruthBook's own fp counter (for `faf`) packed into one
        int64 tensor on the device and copied once: see `metrics_of`"""
        from . import truth as TU
        fp = TU.MOT["fp"]
        packed = torch.cat([self.table, self.dist_total.view(torch.int64), self.book.stats[fp:fp + 1].to(torch.int64)]).cpu()
        n = len(TABLE)
        return metrics_of(packed[:n].tolist(), packed[n:n + 1].view(torch.float64).item(), int(packed[n + 1]))
