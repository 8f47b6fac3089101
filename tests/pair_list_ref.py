"""float64 restatements of training on a pair list (include/pcr.h section C3): `index_sum`, the masked list loss, and the
linear-attention core addressed by index lists.  Plain torch / numpy on the CPU, written from the header's statements;
nothing here imports pcr_amd.  Every function computes in the dtype of its inputs.

The attention comes in two forms that test_pair_list_ref_cpu.py holds to each other:
  * GATHERED: every slot's operands are gathered and train_attn_ref.linattn_ref / linattn_bwd_ref run on the per-slot
    batch (what the library did before the indexed kernels: LinAttn on gathered tensors); the per-slot gradients go back
    to the objects through index_sum.
  * INDEXED: the decomposition the kernels use -- state per object (A, ks), apply per slot, per-slot records
    [dA | dks], their index_sum per object, dk / dv per object.

`fault=` plants one of three mistakes in the indexed form, so that the checks can be seen to catch them:
"dead" (dead slots are summed), "swap" (qi and si exchanged), "one_direction" (only the first half of the slots sends
gradients back)."""
import numpy as np
import torch

import train_attn_ref as R


def live_count(count, P):
    """None -> P; else min(max(count, 0), P)"""
    return P if count is None else min(max(int(count), 0), P)


def index_sum_ref(src, idx, count, M):
    """src (P, ...), idx (P), count (int or None), M -> dst (M, ...): dst[m] = sum over p < min(count, P) with idx[p] == m
    of src[p]; an index outside [0, M) names no row; a row nobody names is 0"""
    P = src.shape[0]
    n = live_count(count, P)
    idx = torch.as_tensor(idx).long()
    live = (torch.arange(P) < n) & (idx >= 0) & (idx < M)
    dst = torch.zeros((M,) + tuple(src.shape[1:]), dtype=src.dtype)
    dst.index_add_(0, idx[live], src[live])
    return dst


def index_sum_seq_f32(src, idx, count, M):
    """the same in numpy float32, added in increasing p from +0: what pcr_index_sum_f32 must give bit for bit"""
    src = np.asarray(src, np.float32)
    P = src.shape[0]
    dst = np.zeros((M,) + src.shape[1:], np.float32)
    for p in range(live_count(count, P)):
        m = int(idx[p])
        if 0 <= m < M:
            dst[m] = dst[m] + src[p]
    return dst


def slot_lists(pairs, count, M):
    """pairs (cap, 2), count -> (qi, si) of 2 cap slots: direction 1 of every pair, then direction 2; a dead slot (p >=
    count, or an index outside [0, M)) carries -1 in both lists"""
    pairs = torch.as_tensor(pairs).long()
    cap = pairs.shape[0]
    alive = (torch.arange(cap) < live_count(count, cap)) & ((pairs >= 0) & (pairs < M)).all(dim=1)
    i = torch.where(alive, pairs[:, 0], torch.full((cap,), -1))
    j = torch.where(alive, pairs[:, 1], torch.full((cap,), -1))
    return torch.cat([i, j]), torch.cat([j, i])


def list_loss_ref(logits, match, count):
    """sum_{p < count} bce(logit_p, match_p) / max(count, 1)"""
    cap = logits.shape[0]
    n = live_count(count, cap)
    per = torch.nn.functional.binary_cross_entropy_with_logits(logits, match, reduction="none")
    return per[:n].sum() / max(n if count is not None else cap, 1)


def _alive(qi, si, M):
    return (qi >= 0) & (qi < M) & (si >= 0) & (si < M)


def linattn_pairs_gathered(q, k, v, qi, si, H, eps, dout=None):
    """q, k, v (M,d,L) per object; qi, si (R) -> out (R,d,L) [, dq, dk, dv (M,d,L) for the output gradient dout]: the
    operands of every live slot gathered, linattn_ref / linattn_bwd_ref on the per-slot batch, the slots' gradients summed
    onto the objects.  A dead slot's output is 0."""
    M, d, Ln = q.shape
    Rn = qi.shape[0]
    alive = _alive(qi, si, M)
    ql, sl = qi[alive], si[alive]
    out = torch.zeros((Rn, d, Ln), dtype=q.dtype)
    out[alive] = R.linattn_ref(q[ql], k[sl], v[sl], H, eps)[0]
    if dout is None:
        return out
    dqs, dks_, dvs = R.linattn_bwd_ref(q[ql], k[sl], v[sl], H, eps, dout[alive])[:3]
    return out, index_sum_ref(dqs, ql, None, M), index_sum_ref(dks_, sl, None, M), index_sum_ref(dvs, sl, None, M)


def linattn_pairs_indexed(q, k, v, qi, si, H, eps, dout=None, fault=None):
    """the same through the kernels' decomposition: state per object, apply per slot, records per slot, index sums, state
    backward per object -> out [, dq, dk, dv, rec (R,H,dh,dh+1)]"""
    M, d, Ln = q.shape
    Rn = qi.shape[0]
    dh = d // H
    if fault == "swap":
        qi, si = si, qi
    heads = lambda t: t.reshape(t.shape[0], H, dh, Ln)                      # noqa: E731
    # state_fwd, per object
    Kp, Vp = R._elu1(heads(k)), heads(v) / Ln
    A = torch.einsum("mhis,mhvs->mhiv", Kp, Vp)
    ks = Kp.sum(dim=3)
    # apply_fwd, per slot
    alive = _alive(qi, si, M)
    qs, ss = qi.clamp(0, M - 1), si.clamp(0, M - 1)
    qh = heads(q)[qs]
    Qp = R._elu1(qh)
    z = 1.0 / (torch.einsum("rhil,rhi->rhl", Qp, ks[ss]) + eps)
    num = torch.einsum("rhil,rhiv->rhvl", Qp, A[ss])
    out = (num * Ln * z.unsqueeze(2)).reshape(Rn, d, Ln) * alive.view(-1, 1, 1).to(q.dtype)
    if dout is None:
        return out
    # apply_bwd, per slot: dq of the slot and its record [dA | dks]
    g = heads(dout)
    dnum = g * z.unsqueeze(2) * Ln
    dden = -z * z * Ln * (g * num).sum(dim=2)
    dqs = (torch.einsum("rhiv,rhvl->rhil", A[ss], dnum) + dden.unsqueeze(2) * ks[ss].unsqueeze(3)) * R._elu1_grad(qh)
    rec = torch.cat([torch.einsum("rhil,rhvl->rhiv", Qp, dnum), torch.einsum("rhl,rhil->rhi", dden, Qp).unsqueeze(3)],
                    dim=3)                                                  # (R,H,dh,dh+1)
    # the two index sums; a dead slot names no object
    dead = torch.full_like(qi, -1)
    sum_q, sum_s = (qs, ss) if fault == "dead" else (torch.where(alive, qi, dead), torch.where(alive, si, dead))
    n = Rn // 2 if fault == "one_direction" else None
    dq = index_sum_ref(dqs.reshape(Rn, d, Ln), sum_q, n, M)
    drec = index_sum_ref(rec, sum_s, n, M)
    # state_bwd, per object
    dA, dks = drec[..., :dh], drec[..., dh]
    dk = (torch.einsum("mhiv,mhvs->mhis", dA, Vp) + dks.unsqueeze(3)) * R._elu1_grad(heads(k))
    dv = torch.einsum("mhis,mhiv->mhvs", Kp, dA) / Ln
    return out, dq, dk.reshape(M, d, Ln), dv.reshape(M, d, Ln), rec
