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


def _i32(t):
    """labels / lengths as the kernels read them; int64 is converted on the device"""
    if t is None:
        return None
    if t.dtype == torch.int64:
        t = t.to(torch.int32)
    L.require_i32(t)
    return t.contiguous()


def compare_pairs(track_labels, det_labels, track_lengths=None, det_lengths=None, min_points=2, num_classes=8, cap=None,
                  out=None):
    """track_labels (T,), det_labels (D,) [, lengths] -> pairs (cap, 2) int32, count (1,) int32.

    (t, d) is listed iff both carry the same label in [0, num_classes) and -- when lengths are given (the reference's
    use_lengths) -- both hold at least min_points points; class ascending, then track, then detection, as the reference's
    torch.cat of per-class cartesian products.  count is the true number of pairs even when it exceeds cap (the first cap
    are written); slots from count on hold (0, 0), valid indices, so the padded list can go to match_gallery as it is.
    cap defaults to T * D.  out = (pairs, count) to write into.
    """
    L.require_cuda(track_labels, det_labels, track_lengths, det_lengths)
    assert track_labels.dim() == 1 and det_labels.dim() == 1, "labels must be (T,) and (D,)"
    tl, dl, tn, dn = _i32(track_labels), _i32(det_labels), _i32(track_lengths), _i32(det_lengths)
    T, D = tl.shape[0], dl.shape[0]
    assert tn is None or tn.shape == (T,), "track_lengths must be (T,)"
    assert dn is None or dn.shape == (D,), "det_lengths must be (D,)"
    cap = T * D if cap is None else int(cap)
    lib = L.load()
    if not lib.pcr_assoc_pairs_ok(T, D, int(num_classes), cap):
        raise L.PcrError("compare_pairs: T=%d D=%d num_classes=%d cap=%d is out of range (pcr_assoc_pairs_ok)"
                         % (T, D, num_classes, cap))
    if out is not None:
        pairs, count = out
        L.require_cuda(pairs, count)
        L.require_i32(pairs, count)
        assert pairs.shape == (cap, 2) and pairs.is_contiguous() and count.shape == (1,)
    else:
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=tl.device)
        count = torch.empty((1,), dtype=torch.int32, device=tl.device)
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
    L.require_cuda(logits, pairs, count, track_miss, det_new, dist, out)
    L.require_f32(logits, track_miss, det_new, dist, out)
    L.require_i32(pairs, count)
    T, D = int(T), int(D)
    assert pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.is_contiguous(), "pairs must be a contiguous (cap, 2) tensor"
    cap = pairs.shape[0]
    assert logits.shape == (cap,) and logits.is_contiguous() and count.numel() == 1
    assert track_miss is None or (track_miss.shape == (T,) and track_miss.is_contiguous())
    assert det_new is None or (det_new.shape == (D,) and det_new.is_contiguous())
    assert dist is None or (dist.shape == (T, D) and dist.is_contiguous())
    lib = L.load()
    if not lib.pcr_assoc_pairs_ok(T, D, 1, cap):
        raise L.PcrError("association_cost: T=%d D=%d cap=%d is out of range (pcr_assoc_pairs_ok)" % (T, D, cap))
    if out is None:
        out = torch.empty((T + D, D + T), dtype=torch.float32, device=logits.device)
    assert out.shape == (T + D, D + T) and out.is_contiguous()
    L.run.pcr_assoc_cost_f32(logits, pairs, count, track_miss, det_new, dist, dist_max, dist_penalty, fill, out, T, D, cap,
                             L.stream_ptr())
    return out


def linear_assignment(cost, return_duals=False, out=None):
    """cost (B, R, C) float32 (a 2-D cost is a batch of one) -> col4row (B, R), row4col (B, C) int32 (-1 = unassigned),
    info (B,) int32 [, u (B, R), v (B, C)].

    The rectangular linear sum assignment of scipy.optimize.linear_sum_assignment (minimum total), solved on the device
    by the shortest augmenting path rules include/pcr.h writes down (ties to the lowest column index).  info 0 = solved;
    1 = the problem holds a NaN or an infinity: its indices are -1 and the solver did not run.  out = (col4row, row4col,
    info[, u, v]) to write into."""
    L.require_cuda(cost)
    L.require_f32(cost)
    if cost.dim() == 2:
        cost = cost.unsqueeze(0)
    assert cost.dim() == 3 and cost.is_contiguous(), "cost must be a contiguous (B, R, C) or (R, C) tensor"
    B, R, C = cost.shape
    lib = L.load()
    if not lib.pcr_lsa_ok(B, R, C):
        raise L.PcrError("linear_assignment: B=%d R=%d C=%d is out of range (pcr_lsa_ok)" % (B, R, C))
    dev = cost.device
    if out is not None:
        col4row, row4col, info = out[0], out[1], out[2]
        u, v = (out[3], out[4]) if return_duals else (None, None)
        L.require_cuda(col4row, row4col, info, u, v)
        L.require_i32(col4row, row4col, info)
        L.require_f32(u, v)
    else:
        col4row = torch.empty((B, R), dtype=torch.int32, device=dev)
        row4col = torch.empty((B, C), dtype=torch.int32, device=dev)
        info = torch.empty((B,), dtype=torch.int32, device=dev)
        u = torch.empty((B, R), dtype=torch.float32, device=dev) if return_duals else None
        v = torch.empty((B, C), dtype=torch.float32, device=dev) if return_duals else None
    assert col4row.shape == (B, R) and row4col.shape == (B, C) and info.shape == (B,)
    assert col4row.is_contiguous() and row4col.is_contiguous()
    assert u is None or (u.shape == (B, R) and v.shape == (B, C) and u.is_contiguous() and v.is_contiguous())
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
    L.require_cuda(cost, row_block, col_block)
    L.require_f32(cost)
    L.require_i32(row_block, col_block)
    if cost.dim() != 2 or not cost.is_contiguous():
        raise L.PcrError("linear_assignment_blocks: cost must be a contiguous (R, C) tensor, got %s" % (tuple(cost.shape),))
    R, C = cost.shape
    G = int(num_blocks)
    if row_block.shape != (R,) or col_block.shape != (C,) or not row_block.is_contiguous() or not col_block.is_contiguous():
        raise L.PcrError("linear_assignment_blocks: row_block must be a contiguous (%d,) and col_block a (%d,) tensor"
                         % (R, C))
    lib = L.load()
    if not lib.pcr_lsa_blocks_ok(R, C, G):
        raise L.PcrError("linear_assignment_blocks: R=%d C=%d num_blocks=%d is out of range (pcr_lsa_blocks_ok)" % (R, C, G))
    dev = cost.device
    if out is not None:
        col4row, row4col, info = out[0], out[1], out[2]
        u, v = (out[3], out[4]) if return_duals else (None, None)
        L.require_cuda(col4row, row4col, info, u, v)
        L.require_i32(col4row, row4col, info)
        L.require_f32(u, v)
    else:
        col4row = torch.empty((R,), dtype=torch.int32, device=dev)
        row4col = torch.empty((C,), dtype=torch.int32, device=dev)
        info = torch.empty((G,), dtype=torch.int32, device=dev)
        u = torch.empty((R,), dtype=torch.float32, device=dev) if return_duals else None
        v = torch.empty((C,), dtype=torch.float32, device=dev) if return_duals else None
    if col4row.shape != (R,) or row4col.shape != (C,) or info.shape != (G,) or not col4row.is_contiguous() \
            or not row4col.is_contiguous() or not info.is_contiguous():
        raise L.PcrError("linear_assignment_blocks: out must hold col4row (%d,), row4col (%d,) and info (%d,)" % (R, C, G))
    if u is not None and (u.shape != (R,) or v.shape != (C,) or not u.is_contiguous() or not v.is_contiguous()):
        raise L.PcrError("linear_assignment_blocks: the duals must be u (%d,) and v (%d,)" % (R, C))
    L.run.pcr_lsa_blocks_f32(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, L.stream_ptr())
    return (col4row, row4col, info, u, v) if return_duals else (col4row, row4col, info)


def association_blocks(track_labels, det_labels, T, D, dd, td, num_classes=8, reduce=False):
    """track_labels (T,), det_labels (D,) -> row_block (T + de*D,), col_block (D + te*T,) int32 and the number of blocks
    num_classes + 1: the block ids of association_cost's (dd = td = 1) or association_cost_multi's matrix for
    linear_assignment_blocks.  An object's block is its label when that lies in [0, num_classes), the rest block num_classes
    otherwise (free bank slots, padded detections, foreign labels); a decision row or column takes its object's block."""
    L.require_cuda(track_labels, det_labels)
    T, D, dd, td = int(T), int(D), int(dd), int(td)
    if track_labels.shape != (T,) or det_labels.shape != (D,):
        raise L.PcrError("association_blocks: labels must be (T,) = (%d,) and (D,) = (%d,)" % (T, D))
    tl, dl = _i32(track_labels), _i32(det_labels)
    lib = L.load()
    if not lib.pcr_assoc_multi_ok(T, D, dd, td, 0) or not lib.pcr_assoc_pairs_ok(0, 0, int(num_classes), 0):
        raise L.PcrError("association_blocks: T=%d D=%d dd=%d td=%d num_classes=%d is out of range (pcr_assoc_multi_ok, "
                         "pcr_assoc_pairs_ok)" % (T, D, dd, td, num_classes))
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
    L.require_cuda(values)
    L.require_f32(values)
    if values.dim() != 2 or values.shape[1] != n or not values.is_contiguous():
        raise L.PcrError("association_cost_multi: %s must be a contiguous (decisions, %d) tensor, got %s"
                         % (what, n, tuple(values.shape)))
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
    if kind not in KINDS:
        raise L.PcrError("association_cost_multi: kind must be 'margin' or 'softmax', got %r" % (kind,))
    reduce = bool(reduce)
    if kind == "softmax" and dist is not None:
        raise L.PcrError("association_cost_multi: the softmax kind takes no distance prior (dist must be None)")
    if kind == "softmax" and reduce:
        raise L.PcrError("association_cost_multi: reduce goes with the margin kind only")
    L.require_cuda(logits, pairs, count, dist)
    L.require_f32(logits, dist)
    L.require_i32(pairs, count)
    T, D = int(T), int(D)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise L.PcrError("association_cost_multi: pairs must be a contiguous (cap, 2) tensor")
    cap = pairs.shape[0]
    if logits.shape != (cap,) or not logits.is_contiguous() or count.numel() != 1:
        raise L.PcrError("association_cost_multi: logits must be a contiguous (cap,) tensor and count hold one int")
    if dist is not None and (dist.shape != (T, D) or not dist.is_contiguous()):
        raise L.PcrError("association_cost_multi: dist must be a contiguous (T, D) tensor")
    dd, det_dec = _decision_rows(det_decisions, D, "det_decisions")
    td, trk_dec = _decision_rows(track_decisions, T, "track_decisions")
    lib = L.load()
    if not lib.pcr_assoc_multi_ok(T, D, dd, td, cap):
        raise L.PcrError("association_cost_multi: T=%d D=%d dd=%d td=%d cap=%d is out of range (pcr_assoc_multi_ok)"
                         % (T, D, dd, td, cap))
    R, C = multi_shape(T, D, dd, td, reduce)
    dev = logits.device
    cost, det_choice, trk_choice = (out if reduce else (out, None, None)) if out is not None else (None, None, None)
    if cost is None:
        cost = torch.empty((R, C), dtype=torch.float32, device=dev)
    if reduce and det_choice is None:
        det_choice = torch.zeros((D,), dtype=torch.int32, device=dev)
    if reduce and trk_choice is None:
        trk_choice = torch.zeros((T,), dtype=torch.int32, device=dev)
    L.require_cuda(cost, det_choice, trk_choice)
    L.require_f32(cost)
    L.require_i32(det_choice, trk_choice)
    if cost.shape != (R, C) or not cost.is_contiguous():
        raise L.PcrError("association_cost_multi: out must be a contiguous (%d, %d) tensor" % (R, C))
    if reduce and (det_choice.shape != (D,) or trk_choice.shape != (T,)):
        raise L.PcrError("association_cost_multi: det_choice must be (D,) and track_choice (T,)")
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
        for k, t in (("logits", logits), ("pairs", pairs), ("count", count), ("det_dec", det_dec), ("trk_dec", trk_dec),
                     ("dist", dist), ("ws", ws), ("cost", cost), ("det_choice", det_choice), ("trk_choice", trk_choice)):
            setattr(p, k, L._p(t))
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
    col4row, row4col, sinfo = assignment[0], assignment[1], assignment[2]
    L.require_cuda(cost, col4row, row4col, sinfo, det_choice, trk_choice)
    L.require_f32(cost)
    L.require_i32(col4row, row4col, sinfo, det_choice, trk_choice)
    lib = L.load()
    if not lib.pcr_assoc_multi_ok(T, D, dd, td, 0):
        raise L.PcrError("decode_assignment: T=%d D=%d dd=%d td=%d is out of range (pcr_assoc_multi_ok)" % (T, D, dd, td))
    if not (-1 <= int(born_decision) < dd and -1 <= int(kill_decision) < td):
        raise L.PcrError("decode_assignment: born_decision must be -1 or below dd = %d, kill_decision -1 or below td = %d"
                         % (dd, td))
    R, C = multi_shape(T, D, dd, td, reduce)
    if tuple(cost.shape[-2:]) != (R, C) or cost.numel() != R * C or not cost.is_contiguous():
        raise L.PcrError("decode_assignment: cost must be a contiguous (%d, %d) tensor, got %s" % (R, C, tuple(cost.shape)))
    if col4row.numel() != R or row4col.numel() != C or sinfo.numel() != 1 or not col4row.is_contiguous() \
            or not row4col.is_contiguous():
        raise L.PcrError("decode_assignment: the assignment must hold col4row (%d,), row4col (%d,) and info (1,)" % (R, C))
    if reduce and (det_choice.shape != (D,) or trk_choice.shape != (T,)):
        raise L.PcrError("decode_assignment: choices must be (det_choice (D,), track_choice (T,))")
    dev = cost.device
    sizes = dict(track_to_det=T, det_to_track=D, det_decision=D, track_decision=T, born=D, kill=T, info=4)
    out = {k: torch.empty((sizes[k],), dtype=torch.int32, device=dev) for k in DECODE_OUTPUTS}
    if T + D == 0:                       # the entry launches nothing
        out["info"].zero_()
        return out
    p = abi.AssocDecodeParams()
    p.T, p.D, p.dd, p.td, p.reduce = T, D, dd, td, int(reduce)
    p.born_dec, p.kill_dec, p.fill = int(born_decision), int(kill_decision), float(fill)
    for k, t in (("cost", cost), ("col4row", col4row), ("row4col", row4col), ("solver_info", sinfo),
                 ("det_choice", det_choice), ("trk_choice", trk_choice)):
        setattr(p, k, L._p(t))
    for k in DECODE_OUTPUTS:
        setattr(p, k, L._p(out[k]))
    L.run.pcr_assoc_decode_i32(ctypes.byref(p), L.stream_ptr())
    return out
