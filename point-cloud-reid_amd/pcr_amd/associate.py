"""Track / detection association on the device (include/pcr.h section A3, csrc/assoc_kernels.hip).

The reference's tracker leaves the device three times per frame between the matching logits and the track update:
`get_labels_to_compare` builds the pair list with torch.where + cartesian_prod (data-dependent shapes,
trackers/deprecated/tracking_point_reid.py:15-33), the cost matrix is filled by indexed assignment
(tracking_association.py:22-53) and the assignment is scipy's on a host copy (:141).  Here each step is a fixed-shape
launch without a host read and with the same bits on every run, so the whole per-frame path can be captured in a HIP
graph.  INTEGRATION.md ("from logits to assignments") has the mapping; `ReIDNet.associate` chains the steps.
"""
import torch

from . import _lib as L


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
