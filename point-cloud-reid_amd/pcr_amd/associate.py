"""Track / detection association on the device (include/pcr.h section A3, csrc/assoc_kernels.hip).

The reference's tracker leaves the device three times per frame between the matching logits and the track update:
`get_labels_to_compare` builds the pair list with torch.where + cartesian_prod (data-dependent shapes,
trackers/deprecated/tracking_point_reid.py:15-33), the cost matrix is filled by indexed assignment
(tracking_association.py:22-53) and the assignment is scipy's on a host copy (:141).  Here each step is a fixed-shape
launch without a host read and with the same bits on every run, so the whole per-frame path can be captured in a HIP
graph.  INTEGRATION.md ("from logits to assignments") has the mapping; `ReIDNet.associate` chains the steps.
"""
import ctypes

import torch

from . import _lib as L
from . import abi


def _labels(t, who, name, n=None, optional=False):
    """labels / lengths as the kernels read them: (n,) int32, contiguous; int64 is converted on the device"""
    return L.tensor(t, who, name, torch.int32, shape=(n,), optional=optional, cast_int64=True, copy=True)


def _pair_list(logits, pairs, count, who):
    """logits (cap,) float32, pairs (cap, 2), count (1,) int32 as compare_pairs returns them -> the three and cap"""
    pairs = L.tensor(pairs, who, "pairs", torch.int32, shape=(None, 2))
    cap = pairs.shape[0]
    return (L.tensor(logits, who, "logits", torch.float32, shape=(cap,)), pairs,
            L.tensor(count, who, "count", torch.int32, numel=1), cap)


def compare_pairs(track_labels, det_labels, track_lengths=None, det_lengths=None, min_points=2, num_classes=8, cap=None,
                  out=None):
    """track_labels (T,), det_labels (D,) [, lengths] -> pairs (cap, 2) int32, count (1,) int32.

    (t, d) is listed iff both carry the same label in [0, num_classes) and -- when lengths are given (the reference's
    use_lengths) -- both hold at least min_points points; class ascending, then track, then detection, as the reference's
    torch.cat of per-class cartesian products.  count is the true number of pairs even when it exceeds cap (the first cap
    are written); slots from count on hold (0, 0), valid indices, so the padded list can go to match_gallery as it is.
    cap defaults to T * D.  out = (pairs, count) to write into.
    """
    who = "compare_pairs"
    tl, dl = _labels(track_labels, who, "track_labels"), _labels(det_labels, who, "det_labels")
    T, D = tl.shape[0], dl.shape[0]
    tn = _labels(track_lengths, who, "track_lengths", T, optional=True)
    dn = _labels(det_lengths, who, "det_lengths", D, optional=True)
    cap = T * D if cap is None else int(cap)
    L.require(L.load().pcr_assoc_pairs_ok(T, D, int(num_classes), cap), who,
              "T=%d D=%d num_classes=%d cap=%d is out of range (pcr_assoc_pairs_ok)", T, D, num_classes, cap)
    L.require(out is None or len(out) == 2, who, "out must be (pairs, count)")
    pairs, count = out if out is not None else (None, None)
    pairs = L.out_tensor(pairs, who, "out[0] (pairs)", torch.int32, (cap, 2), tl.device)
    count = L.out_tensor(count, who, "out[1] (count)", torch.int32, (1,), tl.device)
    L.require_cuda(tl, dl, tn, dn, pairs, count)
    if T == 0 or D == 0:                 # the entry launches nothing for an empty side: the list is empty
        pairs.zero_()
        count.zero_()
        return pairs, count
    L.run.pcr_assoc_pairs_i32(tl, dl, tn, dn, pairs, count, T, D, int(num_classes), int(min_points), cap,
                              L.stream_ptr())
    return pairs, count


def association_cost(logits, pairs, count, T, D, track_miss=None, det_new=None, dist=None, dist_max=22.0,
                     dist_penalty=3.0, fill=10000.0, out=None):
    """logits (cap,), pairs (cap, 2), count (1,) -> cost (T + D, D + T) float32, every element written.

    Top-left (T, D): -logits[k] at pairs[k] for k < min(count, cap) (+ dist_penalty where dist (T, D) > dist_max: the
    reference's distance prior), fill elsewhere; top-right (T, T): track_miss on the diagonal; bottom-left (D, D):
    det_new on the diagonal; bottom-right (D, T): the transpose of the top-left block.  None for track_miss / det_new
    means zeros."""
    who, f32 = "association_cost", torch.float32
    T, D = int(T), int(D)
    logits, pairs, count, cap = _pair_list(logits, pairs, count, who)
    track_miss = L.tensor(track_miss, who, "track_miss", f32, shape=(T,), optional=True)
    det_new = L.tensor(det_new, who, "det_new", f32, shape=(D,), optional=True)
    dist = L.tensor(dist, who, "dist", f32, shape=(T, D), optional=True)
    L.require(L.load().pcr_assoc_pairs_ok(T, D, 1, cap), who,
              "T=%d D=%d cap=%d is out of range (pcr_assoc_pairs_ok)", T, D, cap)
    out = L.out_tensor(out, who, "out", f32, (T + D, D + T), logits.device)
    L.require_cuda(logits, pairs, count, track_miss, det_new, dist, out)
    L.run.pcr_assoc_cost_f32(logits, pairs, count, track_miss, det_new, dist, dist_max, dist_penalty, fill, out, T, D, cap,
                             L.stream_ptr())
    return out


_ASSIGNMENT = (("out[0] (col4row)", torch.int32), ("out[1] (row4col)", torch.int32), ("out[2] (info)", torch.int32),
               ("out[3] (u)", torch.float32), ("out[4] (v)", torch.float32))


def _assignment_out(out, return_duals, rows, cols, info, device, who):
    """the outputs of an assignment, [col4row, row4col, info, u, v] of the shapes rows, cols, info, rows, cols: the first
    three (five with duals) of the caller's out=, or new tensors; u = v = None without duals"""
    shapes = (rows, cols, info, rows, cols) if return_duals else (rows, cols, info)
    if out is None:
        res = [torch.empty(s, dtype=d, device=device) for s, (_, d) in zip(shapes, _ASSIGNMENT)]
    else:
        ok = len(out) >= len(shapes)
        res = [L.tensor(t, who, name, d) for t, (name, d), _ in zip(out, _ASSIGNMENT, shapes)]
        for t, s in zip(res, shapes):
            ok = ok and t.shape == s
        if not ok:
            L.refuse(who, "out must hold col4row %s, row4col %s and info %s" % shapes[:3] +
                     (", u %s and v %s" % shapes[3:] if return_duals else ""))
    return res if return_duals else res + [None, None]


def linear_assignment(cost, return_duals=False, out=None):
    """cost (B, R, C) float32 (a 2-D cost is a batch of one) -> col4row (B, R), row4col (B, C) int32 (-1 = unassigned),
    info (B,) int32 [, u (B, R), v (B, C)].

    The rectangular linear sum assignment of scipy.optimize.linear_sum_assignment (minimum total), solved on the device
    by the shortest augmenting path rules include/pcr.h writes down (ties to the lowest column index).  info 0 = solved;
    1 = the problem holds a NaN or an infinity: its indices are -1 and the solver did not run.  out = (col4row, row4col,
    info[, u, v]) to write into."""
    who = "linear_assignment"
    L.require(isinstance(cost, torch.Tensor) and cost.dim() in (2, 3), who, "cost must be a (B, R, C) or (R, C) tensor")
    cost = L.tensor(cost if cost.dim() == 3 else cost.unsqueeze(0), who, "cost", torch.float32)
    B, R, C = cost.shape
    L.require(L.load().pcr_lsa_ok(B, R, C), who, "B=%d R=%d C=%d is out of range (pcr_lsa_ok)", B, R, C)
    col4row, row4col, info, u, v = _assignment_out(out, return_duals, (B, R), (B, C), (B,), cost.device, who)
    L.require_cuda(cost, col4row, row4col, info, u, v)
    if B == 0 or R == 0 or C == 0:       # the entry launches nothing for an empty problem: nothing is assigned
        col4row.fill_(-1)
        row4col.fill_(-1)
        info.zero_()
        if u is not None:
            u.zero_()
            v.zero_()
    else:
        L.run.pcr_lsa_f32(cost, col4row, row4col, u, v, info, B, R, C, L.stream_ptr())
    return (col4row, row4col, info, u, v) if return_duals else (col4row, row4col, info)


def linear_assignment_blocks(cost, row_block, col_block, num_blocks, return_duals=False, out=None):
    """cost (R, C) float32, row_block (R,), col_block (C,) int32 -> col4row (R,), row4col (C,) int32 (-1 = unassigned),
    info (num_blocks,) int32 [, u (R,), v (C,)].

    The block rule of include/pcr.h: every block id g in [0, num_blocks) names the sub-problem cost[rows of g][columns of
    g] (ascending original index), solved by linear_assignment's rules by a wave of its own and written back as original
    indices; a row or column with any other id takes no part (-1, dual 0) and only the sub-problems' entries are read.
    info[g] 0 = solved, 1 = block g holds a NaN or an infinity (its rows and columns are -1; the other blocks are solved).
    One launch for all blocks.  out = (col4row, row4col, info[, u, v]) to write into."""
    who = "linear_assignment_blocks"
    cost = L.tensor(cost, who, "cost", torch.float32, shape=(None, None))
    R, C = cost.shape
    G = int(num_blocks)
    row_block = L.tensor(row_block, who, "row_block", torch.int32, shape=(R,))
    col_block = L.tensor(col_block, who, "col_block", torch.int32, shape=(C,))
    L.require(L.load().pcr_lsa_blocks_ok(R, C, G), who,
              "R=%d C=%d num_blocks=%d is out of range (pcr_lsa_blocks_ok)", R, C, G)
    col4row, row4col, info, u, v = _assignment_out(out, return_duals, (R,), (C,), (G,), cost.device, who)
    L.require_cuda(cost, row_block, col_block, col4row, row4col, info, u, v)
    L.run.pcr_lsa_blocks_f32(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, L.stream_ptr())
    return (col4row, row4col, info, u, v) if return_duals else (col4row, row4col, info)


def association_blocks(track_labels, det_labels, T, D, dd, td, num_classes=8, reduce=False):
    """track_labels (T,), det_labels (D,) -> row_block (T + de*D,), col_block (D + te*T,) int32 and the number of blocks
    num_classes + 1: the block ids of association_cost's (dd = td = 1) or association_cost_multi's matrix for
    linear_assignment_blocks.  An object's block is its label when that lies in [0, num_classes), the rest block num_classes
    otherwise (free bank slots, padded detections, foreign labels); a decision row or column takes its object's block."""
    who = "association_blocks"
    T, D, dd, td = int(T), int(D), int(dd), int(td)
    L.require(all(isinstance(t, torch.Tensor) for t in (track_labels, det_labels)) and track_labels.shape == (T,)
              and det_labels.shape == (D,), who, "labels must be (T,) = (%d,) and (D,) = (%d,)", T, D)
    tl, dl = _labels(track_labels, who, "track_labels", T), _labels(det_labels, who, "det_labels", D)
    lib = L.load()
    L.require(lib.pcr_assoc_multi_ok(T, D, dd, td, 0) and lib.pcr_assoc_pairs_ok(0, 0, int(num_classes), 0), who,
              "T=%d D=%d dd=%d td=%d num_classes=%d is out of range (pcr_assoc_multi_ok, pcr_assoc_pairs_ok)",
              T, D, dd, td, num_classes)
    L.require_cuda(tl, dl)
    R, C = multi_shape(T, D, dd, td, reduce)
    de, te = (int(dd > 0), int(td > 0)) if reduce else (dd, td)
    row_block = torch.empty((R,), dtype=torch.int32, device=tl.device)
    col_block = torch.empty((C,), dtype=torch.int32, device=tl.device)
    if R + C:                            # the entry launches nothing for two empty outputs
        L.run.pcr_assoc_blocks_i32(tl, dl, row_block, col_block, T, D, de, te, int(num_classes), L.stream_ptr())
    return row_block, col_block, int(num_classes) + 1


# ---- any set of decisions per side (pcr.h A3, "Any set of decisions") ----------------------------------------------------
KINDS = {"margin": 0, "softmax": 1}

_WS = {}          # (device index, T, D, dd, td) -> uint8 workspace of pcr_assoc_multi_ws_bytes


def _decision_rows(values, n, what):
    """decision values (k, n) -> (k, tensor or None); None = no decision on this side"""
    if values is None:
        return 0, None
    values = L.tensor(values, "association_cost_multi", what, torch.float32, shape=(None, n))
    return values.shape[0], (values if values.shape[0] else None)


def multi_shape(T, D, dd, td, reduce=False):
    """(R, C) of the matrix with dd detection and td tracking decisions; reduce keeps one diagonal block per side"""
    de, te = (int(dd > 0), int(td > 0)) if reduce else (dd, td)
    return T + de * D, D + te * T


def association_cost_multi(logits, pairs, count, T, D, det_decisions=None, track_decisions=None, kind="margin", reduce=False,
                           dist=None, dist_max=22.0, dist_penalty=3.0, fill=10000.0, out=None):
    """logits (cap,), pairs (cap, 2), count (1,), det_decisions (dd, D), track_decisions (td, T) -> cost (T + dd*D, D + td*T)
    float32, every element written: the reference's matrix for any set of decisions (tracking_association.py:22-53, :126).

    kind "margin": -logits[k] at the listed pairs (+ dist_penalty where dist > dist_max), the decision values as costs on
    the diagonals of their blocks, the transpose of the top-left block in every bottom-right block; with dd = td = 1 it is
    association_cost's matrix bit for bit.  kind "softmax" (get_cost_mat_softmax, :56-98): logits and decision values
    are scores; a listed pair holds -max(p_row, p_col), a decision -p of that decision, the softmaxes running over a
    track's (a detection's) listed pairs and its decisions only; dist must be None.  reduce (margin only,
    TrackingAssociatorMax): one diagonal block per side holding each object's cheapest decision, and the return value is
    (cost, det_choice (D,), track_choice (T,)) with the chosen decision indices (zeros for a side without decisions).
    None for det_decisions / track_decisions means no decision on that side.  out = cost, or (cost, det_choice,
    track_choice) under reduce, to write into."""
    who, f32, i32 = "association_cost_multi", torch.float32, torch.int32
    L.require(kind in KINDS, who, "kind must be 'margin' or 'softmax', got %r", kind)
    reduce = bool(reduce)
    L.require(kind != "softmax" or dist is None, who, "the softmax kind takes no distance prior (dist must be None)")
    L.require(kind != "softmax" or not reduce, who, "reduce goes with the margin kind only")
    T, D = int(T), int(D)
    logits, pairs, count, cap = _pair_list(logits, pairs, count, who)
    dist = L.tensor(dist, who, "dist", f32, shape=(T, D), optional=True)
    dd, det_dec = _decision_rows(det_decisions, D, "det_decisions")
    td, trk_dec = _decision_rows(track_decisions, T, "track_decisions")
    lib = L.load()
    L.require(lib.pcr_assoc_multi_ok(T, D, dd, td, cap), who,
              "T=%d D=%d dd=%d td=%d cap=%d is out of range (pcr_assoc_multi_ok)", T, D, dd, td, cap)
    R, C = multi_shape(T, D, dd, td, reduce)
    dev = logits.device
    L.require(out is None or not reduce or len(out) == 3, who, "under reduce out must be (cost, det_choice, track_choice)")
    cost, det_choice, trk_choice = (out if reduce else (out, None, None)) if out is not None else (None, None, None)
    cost = L.out_tensor(cost, who, "out", f32, (R, C), dev)
    if reduce:
        det_choice = torch.zeros((D,), dtype=i32, device=dev) if det_choice is None else \
            L.tensor(det_choice, who, "det_choice", i32, shape=(D,))
        trk_choice = torch.zeros((T,), dtype=i32, device=dev) if trk_choice is None else \
            L.tensor(trk_choice, who, "track_choice", i32, shape=(T,))
    L.require_cuda(logits, pairs, count, dist, det_dec, trk_dec, cost, det_choice, trk_choice)
    if R * C:                            # the entry launches nothing for an empty matrix
        p = abi.AssocMultiParams()
        p.T, p.D, p.dd, p.td, p.cap, p.kind, p.reduce = T, D, dd, td, cap, KINDS[kind], int(reduce)
        p.dist_max, p.dist_penalty, p.fill = float(dist_max), float(dist_penalty), float(fill)
        ws = None
        if kind == "softmax":
            key = (dev.index, T, D, dd, td)
            ws = _WS.get(key)
            if ws is None:
                if torch.cuda.is_current_stream_capturing():
                    raise L.PcrError("association_cost_multi: nothing is cached for %r yet; run the call once outside the "
                                     "capture" % (key,))
                ws = _WS[key] = torch.empty((max(lib.pcr_assoc_multi_ws_bytes(T, D, dd, td), 8),), dtype=torch.uint8,
                                            device=dev)
        sizes = dict(logits=cap, pairs=2 * cap, count=1, det_dec=dd * D, trk_dec=td * T, dist=T * D,
                     ws=0 if ws is None else ws.numel(), cost=R * C, det_choice=D, trk_choice=T)
        abi.fill(p, dict(logits=logits, pairs=pairs, count=count, det_dec=det_dec, trk_dec=trk_dec, dist=dist, ws=ws,
                         cost=cost, det_choice=det_choice, trk_choice=trk_choice), sizes, who=who)
        L.run.pcr_assoc_cost_multi_f32(ctypes.byref(p), L.stream_ptr())
    return (cost, det_choice, trk_choice) if reduce else cost


DECODE_OUTPUTS = ("track_to_det", "det_to_track", "det_decision", "track_decision", "born", "kill", "info")


def decode_assignment(cost, assignment, T, D, dd, td, fill=10000.0, choices=None, born_decision=-1, kill_decision=-1):
    """cost (R, C) of association_cost_multi and assignment = linear_assignment's (col4row, row4col, info) over it -> dict of
    track_to_det (T,), det_to_track (D,) [-1 = none], det_decision (D,) [0 = matched, 1 + i = detection decision i, 1 + dd =
    unmatched], track_decision (T,) [likewise with td], born (D,) = det_decision == 1 + born_decision, kill (T,) =
    track_decision == 1 + kill_decision (int32 0 / 1, what TrackBank.update takes; all zero for a decision of -1) and info
    (4,) = the solver's info, void assignments (an assigned entry that holds fill: both sides become unassigned), repaired
    tracks, repaired detections.  It is tracking_association.py:146-245 in fixed shape (pcr.h has the rules and the two
    deliberate differences).  choices = (det_choice, track_choice) of a reduce matrix."""
    T, D, dd, td = int(T), int(D), int(dd), int(td)
    reduce = choices is not None
    det_choice, trk_choice = choices if reduce else (None, None)
    who = "decode_assignment"
    L.require(len(assignment) >= 3, who, "assignment must be linear_assignment's (col4row, row4col, info)")
    L.require(L.load().pcr_assoc_multi_ok(T, D, dd, td, 0), who,
              "T=%d D=%d dd=%d td=%d is out of range (pcr_assoc_multi_ok)", T, D, dd, td)
    L.require(-1 <= int(born_decision) < dd and -1 <= int(kill_decision) < td, who,
              "born_decision must be -1 or below dd = %d, kill_decision -1 or below td = %d", dd, td)
    R, C = multi_shape(T, D, dd, td, reduce)
    L.require(isinstance(cost, torch.Tensor) and tuple(cost.shape[-2:]) == (R, C), who,
              "cost must be a contiguous (%d, %d) tensor, got %s", R, C, tuple(getattr(cost, "shape", ())))
    sizes = dict(cost=R * C, col4row=R, row4col=C, solver_info=1, det_choice=D, trk_choice=T, track_to_det=T,
                 det_to_track=D, det_decision=D, track_decision=T, born=D, kill=T, info=4)
    out = {k: torch.empty((sizes[k],), dtype=torch.int32, device=cost.device) for k in DECODE_OUTPUTS}
    given = dict(cost=cost, col4row=assignment[0], row4col=assignment[1], solver_info=assignment[2], det_choice=det_choice,
                 trk_choice=trk_choice)
    p = abi.AssocDecodeParams()
    p.T, p.D, p.dd, p.td, p.reduce = T, D, dd, td, int(reduce)
    p.born_dec, p.kill_dec, p.fill = int(born_decision), int(kill_decision), float(fill)
    abi.fill(p, dict(given, **out), sizes, required=[k for k in given if reduce or not k.endswith("choice")], who=who)
    if T + D == 0:                       # the entry launches nothing
        out["info"].zero_()
        return out
    L.run.pcr_assoc_decode_i32(ctypes.byref(p), L.stream_ptr())
    return out
