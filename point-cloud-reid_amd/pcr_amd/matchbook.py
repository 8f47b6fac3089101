"""Scoring a validation split on the device (include/pcr.h section A13, csrc/match_kernels.hip).

`RankBook`, `TruthBook` and `IdentityBook` keep their scores in device tables; `val_match_acc` and the reference's
`MatchingEval` tables -- what `evaluate_checkpoint` reports and the acceptance criterion is stated in -- took the reference's
host route: five per-pair tensors of every batch kept, gathered column by column and copied to the CPU, where
pcr_amd/metrics.py selects subsets.  `MatchBook` is the same answer from ONE table of 64-bit integer counters: `add` is a
fixed-shape launch per batch (no host read, no allocation, integer atomics only, so the same bits on every run and legal
inside a HIP-graph capture), `reduce` one all-reduce of the table, `metrics()` / `tables()` the one host read.

The float entries are derived from the counts by the float32 operations of `metrics.f1_precision_recall` and
`metrics._entry` (a sum of 0 / 1 values below 2^24 of them is the exact integer), so they equal the host route's bit for bit
while the split has fewer than 2^24 pairs; beyond that they are computed from the exact counts in float64 and the dicts
carry `counts_beyond_f32 = True`.  The decision is `logit > 0`, not the host route's `sigmoid(logit) > 0.5` in float32: the
two differ for logits in about (0, 2e-7] ("validation on the device").
"""
import ctypes
import itertools

import numpy as np
import torch

from . import _lib as L
from . import abi
from . import shard

CELLS, KEY_BINS, PTS_BINS = 6, 64, 32                        # PCR_MATCH_CELLS, _KEY_BINS, _PTS_BINS
ALL, CLS0, CLSMAX, PTS, VIS, OBJ, TABLE = 0, 6, 390, 774, 6918, 31494, 31498      # PCR_MATCH_ALL .. PCR_MATCH_TABLE
OBJECTS = dict(cls_correct=0, cls_total=1, fp_correct=2, fp_total=3)               # PCR_MATCH_CLS_CORRECT ..
INFO = dict(nan=1, gt=2, cls=4, pts=8, vis=16)                                     # PCR_MATCH_INFO_*
KEY_MIN, KEY_MAX = -1, KEY_BINS - 2                          # the range of a cls / vis value
F32_EXACT = 1 << 24
_WHO = "pcr_amd.matchbook"
_COLS = dict(logit="val_match_preds", gt="val_match_gt", cls="match_classes", num_points="num_points", vis="val_vis_gt_all")


def match_ok(P=0, M=0, C=1):
    return bool(L.load().pcr_match_ok(int(P), int(M), int(C)))


def _columns(logit, gt, cls, num_points, vis, count):
    """the arguments of `record` as the kernel reads them (int64 columns converted on their device); every refusal that
    does not need a device comes before the one that does"""
    f32, i32 = torch.float32, torch.int32
    logit = L.tensor(logit, _WHO, "logit", f32, shape=(None,))
    P = logit.shape[0]
    gt = L.tensor(gt, _WHO, "gt", f32, shape=(P,))
    pair = {}
    for name, t in (("cls", cls), ("num_points", num_points), ("vis", vis)):
        if isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[2] == 1:
            t = t.squeeze(2)                                 # (the reference's visibility column comes as (P, 2, 1))
        pair[name] = L.tensor(t, _WHO, name, i32, shape=(P, 2), cast_int64=True, copy=True)
    count = L.tensor(count, _WHO, "count", i32, numel=1, optional=True, cast_int64=True)
    return P, dict(logit=logit, gt=gt, count=count, **pair)


def record(table, info, logit, gt, cls, num_points, vis, count=None):
    """pcr_match_record_i64 on explicit tensors: logit, gt (P,) float32; cls, num_points, vis (P, 2) int32 (int64 is
    converted); count (1,) int32 on the device or None -> table (TABLE,) int64 added to, info (1,) int32 or-ed into"""
    P, t = _columns(logit, gt, cls, num_points, vis, count)
    L.require(match_ok(P=P), _WHO, "P=%d is out of range (pcr_match_ok)", P)
    t.update(table=table, info=info)
    sizes = dict(logit=P, gt=P, cls=2 * P, num_points=2 * P, vis=2 * P, count=1, table=TABLE, info=1)
    p = abi.MatchParams()
    p.P = P
    abi.fill(p, t, sizes, required=("logit", "gt", "cls", "num_points", "vis", "table", "info"), who=_WHO)
    L.run.pcr_match_record_i64(ctypes.byref(p), L.stream_ptr())


def record_objects(table, info, cls_logits=None, cls_gt=None, fp_logits=None, fp_gt=None, count=None, period=None):
    """pcr_match_record_objects_i64 on explicit tensors: cls_logits (M, C) float32 with cls_gt (M,) int32 / int64, fp_logits
    (M,) float32 with fp_gt (M,) float32, either pair or both; object m counts iff (m % period) < count (period: M)"""
    f32, i32 = torch.float32, torch.int32
    L.require((cls_logits is None) == (cls_gt is None) and (fp_logits is None) == (fp_gt is None), _WHO,
              "a head's logits and its targets come together")
    M, C = None, 1
    if cls_logits is not None:
        cls_logits = L.tensor(cls_logits, _WHO, "cls_logits", f32, shape=(None, None), copy=True)
        M, C = cls_logits.shape
        cls_gt = L.tensor(cls_gt, _WHO, "cls_gt", i32, shape=(M,), cast_int64=True, copy=True)
    if fp_logits is not None:
        fp_logits = L.tensor(fp_logits, _WHO, "fp_logits", f32, shape=(M,), copy=True)
        M = fp_logits.shape[0]
        fp_gt = L.tensor(fp_gt, _WHO, "fp_gt", f32, shape=(M,), copy=True)
    if M is None:
        return
    count = L.tensor(count, _WHO, "count", i32, numel=1, optional=True, cast_int64=True)
    period = M if period is None else int(period)
    L.require(M == 0 or (match_ok(M=M, C=C) and 1 <= period <= M), _WHO, "M=%d C=%d period=%d is out of range (pcr_match_ok)",
              M, C, period)
    table = L.tensor(table, _WHO, "table", torch.int64, shape=(TABLE,))
    info = L.tensor(info, _WHO, "info", i32, numel=1)
    L.require_cuda(cls_logits, cls_gt, fp_logits, fp_gt, count, table, info)
    L.run.pcr_match_record_objects_i64(cls_logits, cls_gt, fp_logits, fp_gt, count, table.data_ptr() + 8 * OBJ,
                                       info, M, C, max(period, 1), L.stream_ptr())


# ---- the host side: a table -> the dicts of pcr_amd.metrics ---------------------------------------------------------------
class _Derive:
    """the float entries of one subset's six counters n = [gt 1: pred 0, pred 1 | gt 0: .. | gt -1: ..], by the float32
    operations of metrics.f1_precision_recall / metrics._entry, or (wide) in float64 from the exact counts"""

    def __init__(self, wide):
        self.f = np.float64 if wide else np.float32

    def f1(self, n):
        f, eps = self.f, self.f(1e-6)
        tp, npos, pred1 = f(n[1]), f(n[0] + n[1]), f(n[1] + n[3] + n[5])
        tn, nneg, pred0 = f(n[2]), f(n[2] + n[3]), f(n[0] + n[2] + n[4])
        with np.errstate(invalid="ignore", divide="ignore"):
            recall_pos = tp / (npos + eps)
            precision_pos = tp / (pred1 + eps)
            f1_pos = f(2) * (precision_pos * recall_pos) / (precision_pos + recall_pos + eps)
            recall_neg = tn / nneg + eps                     # (the reference adds its 1e-6 AFTER the division here)
            precision_neg = tn / pred0 + eps
            f1_neg = f(2) * (precision_neg * recall_neg) / (precision_neg + recall_neg + eps)
        vals = (f1_pos, recall_pos, precision_pos, f1_neg, recall_neg, precision_neg)
        keys = ("val_match_f1_pos", "val_match_recall_pos", "val_match_precision_pos", "val_match_f1_neg",
                "val_match_recall_neg", "val_match_precision_neg")
        return dict(zip(keys, (float(v) for v in vals)))

    def accuracy(self, n):
        """mean(pred == gt) over the subset: a row with gt -1 is never right"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(self.f(n[1] + n[2]) / self.f(int(np.sum(n))))

    def ratio(self, a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(self.f(a) / self.f(b))

    def entry(self, n, nan_to_minus1=True):
        e = self.f1(n)
        e["accuracy"] = self.accuracy(n)
        e["num_observations_pos"] = int(n[0] + n[1])
        e["num_observations_neg"] = int(n[2] + n[3])
        if nan_to_minus1:
            e = {k: (-1 if isinstance(v, float) and v != v else v) for k, v in e.items()}
        return e


def _host_table(table):
    t = np.asarray(table, dtype=np.int64).reshape(-1)
    if t.shape[0] != TABLE:
        raise ValueError("a MatchBook table holds %d counters, got %d" % (TABLE, t.shape[0]))
    return t


def _is_wide(t):
    return int(t[ALL:ALL + CELLS].sum()) >= F32_EXACT


def metrics_of(table, cls_to_idx=None, num_classes=None):
    """a table on the host -> the dict of `metrics.evaluate`: val_match_acc, f1 / precision / recall, the per-class and
    per-point-bucket accuracies of the non-empty subsets, val_cls_acc / val_fp_acc of the heads that were added"""
    t = _host_table(table)
    wide = _is_wide(t)
    d = _Derive(wide)
    n_all = t[ALL:ALL + CELLS]
    out = {"val_match_acc": d.accuracy(n_all)}
    out.update(d.f1(n_all))
    if cls_to_idx:
        cls0 = t[CLS0:CLSMAX].reshape(KEY_BINS, CELLS)
        for name, idx in cls_to_idx.items():
            if KEY_MIN <= int(idx) <= KEY_MAX and cls0[int(idx) + 1].sum() > 0:
                out["val_match_acc_%s" % name] = d.accuracy(cls0[int(idx) + 1])
        if num_classes is not None:
            clsmax = t[CLSMAX:PTS].reshape(KEY_BINS, CELLS)
            n = clsmax[max(0, min(KEY_BINS, int(num_classes) + 1)):].sum(axis=0)
            if n.sum() > 0:
                out["val_match_acc_FP"] = d.accuracy(n)
    pts = t[PTS:VIS].reshape(PTS_BINS, PTS_BINS, CELLS)
    for i in range(_top_bin(pts)):                           # b = 2^i <= the largest cloud
        n = pts[i + 1:].sum(axis=(0, 1))                     # the sparser object has at least 2^i points
        if n.sum() > 0:
            out["val_match_acc_both_ge_%d_pts" % (1 << i)] = d.accuracy(n)
    obj = t[OBJ:OBJ + len(OBJECTS)]
    for k in ("cls", "fp"):
        if obj[OBJECTS[k + "_total"]] > 0:
            out["val_%s_acc" % k] = d.ratio(obj[OBJECTS[k + "_correct"]], obj[OBJECTS[k + "_total"]])
    if wide:
        out["counts_beyond_f32"] = True
    return out


def _top_bin(pts):
    """the highest non-empty bin of the larger point count over ALL rows, 0 for an empty table: 1 + floor(log2 max)"""
    used = np.nonzero(pts.sum(axis=(0, 2)))[0]
    return int(used.max()) if used.size else 0


def tables_of(table):
    """a table on the host -> the dict of `metrics.evaluate_tables`: results_per_points, results_per_distance,
    results_per_visibility (the last two from the one visibility column, as the reference feeds them)"""
    t = _host_table(table)
    d = _Derive(_is_wide(t))
    pts = t[PTS:VIS].reshape(PTS_BINS, PTS_BINS, CELLS)
    vis = t[VIS:OBJ].reshape(KEY_BINS, KEY_BINS, CELLS)
    out = {}
    if int(t[ALL:ALL + CELLS].sum()) == 0:
        return out

    # points: edges 2^0 .. 2^(T-1), T the top bin; bucket i = [2^i, 2^(i+1)) = bin i + 1, for i < T - 1
    nb = max(_top_bin(pts) - 1, 0)
    one = {(i, i + 1): d.entry(pts[:, i + 1:].sum(axis=(0, 1))) for i in range(nb)}
    both = {(i, i + 1): d.entry(pts[i + 1:].sum(axis=(0, 1))) for i in range(nb)}
    pair = {((i, i + 1), (j, j + 1)): d.entry(pts[i + 1, j + 1])
            for i, j in itertools.combinations_with_replacement(range(nb), 2)}
    out["results_per_points"] = dict(at_least_one=one, at_least_both=both, for_a_pair=pair)

    # distance: the raw value v sits at index v + 1; edges 5 i for i < int(max / 5) + 3
    used = np.nonzero(vis.sum(axis=(0, 2)))[0]
    if used.size == 0:                                       # (no row's visibility was in range: info says so)
        return out
    top = int(used.max()) - 1
    edges = [5 * i for i in range(int(top / 5) + 3)]
    nb = len(edges) - 1
    one = {(i, i + 1): d.entry(vis[:edges[i] + 2].sum(axis=(0, 1))) for i in range(nb)}              # near <= edge
    both = {(i, i + 1): d.entry(vis[:, :edges[i] + 2].sum(axis=(0, 1))) for i in range(nb)}          # far <= edge
    bucket = lambda i: slice(min(edges[i] + 1, KEY_BINS), min(edges[i + 1] + 1, KEY_BINS))            # noqa: E731
    pair = {((i, i + 1), (j, j + 1)): d.entry(vis[bucket(i), bucket(j)].sum(axis=(0, 1)))
            for i, j in itertools.combinations_with_replacement(range(nb), 2)}
    out["results_per_distance"] = dict(at_least_one=one, at_least_both=both, for_a_pair=pair)

    # visibility: the pairs with gt -1 are left out; only for_a_pair replaces its NaNs
    real = vis.copy()
    real[:, :, 4:] = 0
    levels = (0, 1, 2, 3)
    one = {x: d.entry(real[:, x + 1:].sum(axis=(0, 1)), nan_to_minus1=False) for x in levels}
    both = {x: d.entry(real[x + 1:].sum(axis=(0, 1)), nan_to_minus1=False) for x in levels}
    pair = {(x, y): d.entry(real[x + 1, y + 1]) for x, y in itertools.combinations_with_replacement(levels, 2)}
    out["results_per_visibility"] = dict(at_least_one=one, at_least_both=both, for_a_pair=pair)
    return out


def info_names(info):
    return [k for k, bit in INFO.items() if int(info) & bit]


class MatchBook:
    """The validation split's table and flag word on `device`.

    num_classes, cls_to_idx   what `metrics.evaluate` takes: the per-class keys and `val_match_acc_FP` (pairs with a class
                              id >= num_classes) are read from the class bins at `metrics()` time
    `add` / `add_objects` / `reset` launch on the current stream and never read the device; `reduce` is one collective;
    `metrics()` and `tables()` each make one host read and raise when the flag word is set (a row the table could not
    hold: the book is then not the host route's answer), unless `strict=False`.  A book on the CPU holds a table only
    (loaded, or reduced over gloo): there is no CPU fallback of `add`."""

    def __init__(self, device="cuda", num_classes=None, cls_to_idx=None):
        self.device = torch.device(device)
        self.num_classes = None if num_classes is None else int(num_classes)
        self.cls_to_idx = dict(cls_to_idx) if cls_to_idx else None
        self.table = torch.zeros(TABLE, dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, res=None, count=None, **cols):
        """one batch of pairs: a `forward_test`-shaped dict (val_match_preds, val_match_gt, match_classes, num_points,
        val_vis_gt_all) or the bare tensors logit=, gt=, cls=, num_points=, vis=.  count: a (1,) device tensor -- only the
        first count rows take part (a padded batch)"""
        if res is not None:
            L.require(isinstance(res, dict) and not cols, _WHO, "add takes a forward_test-shaped dict or the bare tensors")
            for k, key in _COLS.items():
                L.require(key in res, _WHO, "the result dict has no %r", key)
            cols = {k: res[key] for k, key in _COLS.items()}
        L.require(set(cols) == set(_COLS), _WHO, "add needs logit, gt, cls, num_points and vis; got %s", sorted(cols))
        record(self.table, self.flags, count=count, **cols)

    def add_objects(self, cls_logits=None, cls_gt=None, fp_logits=None, fp_gt=None, count=None, period=None):
        """the per-object heads' outputs (`val_cls_preds` / `val_cls_gt`, `val_fp_preds` / `val_fp_gt` of forward_test);
        with count, object m takes part iff (m % period) < count: period = b for the 2 b objects of b padded pairs"""
        record_objects(self.table, self.flags, cls_logits, cls_gt, fp_logits, fp_gt, count, period)

    def reduce(self):
        """ONE all_reduce(SUM) of the table (the flag word travels in it as a counter per bit); over gloo the table goes
        through the CPU, as evaluate_model's gathers do.  Nothing to do on one rank."""
        if not shard.is_dist():
            return
        import torch.distributed as dist
        bits = torch.arange(len(INFO), dtype=torch.int32, device=self.device)
        buf = torch.cat([self.table, ((self.flags >> bits) & 1).to(torch.int64)])
        if dist.get_backend() == "gloo":
            buf = buf.cpu()
        dist.all_reduce(buf)
        buf = buf.to(self.device)
        self.table.copy_(buf[:TABLE])
        self.flags.copy_(((buf[TABLE:] > 0).to(torch.int32) << bits).sum(dtype=torch.int32).reshape(1))

    def reset(self):
        self.table.zero_()
        self.flags.zero_()

    def _read(self, strict):
        """THE host read: the table and the flag word in one copy"""
        packed = torch.cat([self.table, self.flags.to(torch.int64)]).cpu().numpy()
        info = int(packed[TABLE])
        if strict and info != 0:
            raise L.PcrError("%s: the book holds rows outside the table's rules (info = %d: %s); it is not the host "
                             "route's answer" % (_WHO, info, ", ".join(info_names(info))))
        return packed[:TABLE]

    @property
    def info(self):
        """the flag word (a host read): bits INFO"""
        return int(self.flags.item())

    @property
    def num_pairs(self):
        """the rows counted so far (a host read)"""
        return int(self.table[ALL:ALL + CELLS].sum().item())

    def metrics(self, strict=True):
        return metrics_of(self._read(strict), self.cls_to_idx, self.num_classes)

    def tables(self, strict=True):
        return tables_of(self._read(strict))

    def results(self, strict=True):
        """metrics() and tables() from ONE host read: -> (metrics dict, tables dict)"""
        t = self._read(strict)
        return metrics_of(t, self.cls_to_idx, self.num_classes), tables_of(t)
