"""float64 restatements of training on a pair list (include/pcr.h section C3): `index_sum`, the masked list loss, and the
linear-attention core addressed by index lists.  Plain torch / numpy on the CPU, written from the header's statements;
nothing here imports pcr_amd.  Every function computes in the dtype of its inputs.

The attention comes in two forms that test_pair_list_ref_cpu.py holds to each other:
  * GATHERED: every slot's operands are gathered and train_attn_ref.linattn_ref / linattn_bwd_ref run on the per-slot
    batch (what the library did before the indexed kernels: LinAttn on gathered tensors); the per-slot gradients go back
    to the objects through index_sum.
  * INDEXED: the decomposition the kernels use -- state per object (A, ks), apply per slot, per-slot records
    [dA | dks], their index_sum per object, dk / dv per object.

The indexed form is written launch by launch, every output in the kernel's own layout (pairs_state_fwd, pairs_apply_fwd,
pairs_apply_bwd, pairs_state_bwd), so that test_gpu_pair_list_ops.py can hold each launch on its own;
linattn_pairs_indexed chains them, and linattn_pairs_scales gives the sums of absolute per-slot contributions that a
float32 list-order sum rounds in proportion to.

`fault=` plants one mistake in the indexed form, so that the checks can be seen to catch it: "dead" (dead slots are
summed), "swap" (qi and si exchanged), "one_direction" (only the first half of the slots sends gradients back);
"pad_one" (the padding keys of the last 64-token chunk counted as K' = elu(0) + 1 = 1 in ks), "half_dead" (a slot with ONE
index outside [0, M) still sends dqs and rec back, to the object its other index names), "rec_layout" (the record
interleaved as (dh, dh + 1) rows [dA_i | dks_i] but read as the kernel's [dA | dks]), "round_1024" (the index sums stop
after their first 1024 slots)."""
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


CHUNK = 64        # tokens per staged chunk of the kernels (kAT)


def _heads(t, H):
    n, d, Ln = t.shape
    return t.reshape(n, H, d // H, Ln)


def pairs_state_fwd(k, v, H, fault=None):
    """k, v (M,d,L) -> A (M,H,dh,dh), ks (M,H,dh): A = sum_s K'_s V'_s^T, ks = sum_s K'_s, K' = elu(k) + 1, V' = v / L"""
    Ln = k.shape[2]
    Kp, Vp = R._elu1(_heads(k, H)), _heads(v, H) / Ln
    A = torch.einsum("mhis,mhvs->mhiv", Kp, Vp)
    ks = Kp.sum(dim=3)
    if fault == "pad_one":
        ks = ks + float(-Ln % CHUNK)
    return A, ks


def _slot_operands(q, A, ks, qi, si, H):
    M = q.shape[0]
    alive = _alive(qi, si, M)
    qs, ss = qi.clamp(0, M - 1), si.clamp(0, M - 1)
    qh = _heads(q, H)[qs]
    return alive, qh, R._elu1(qh), A[ss], ks[ss]


def pairs_apply_fwd(q, A, ks, qi, si, H, eps):
    """q (M,d,L), A, ks of pairs_state_fwd, qi, si (R) -> out (R,d,L): out_r = (Q'_{qi[r]}^T A_{si[r]}) L / (Q'_{qi[r]} .
    ks_{si[r]} + eps); a dead slot's block is 0"""
    M, d, Ln = q.shape
    alive, qh, Qp, As, kss = _slot_operands(q, A, ks, qi, si, H)
    z = 1.0 / (torch.einsum("rhil,rhi->rhl", Qp, kss) + eps)
    num = torch.einsum("rhil,rhiv->rhvl", Qp, As)
    return (num * Ln * z.unsqueeze(2)).reshape(-1, d, Ln) * alive.view(-1, 1, 1).to(q.dtype)


def pairs_apply_bwd(q, A, ks, qi, si, H, eps, dout, fault=None):
    """-> dqs (R,d,L), rec (R,H,dh (dh + 1)) = [dA_r (dh x dh, row-major) | dks_r (dh)], (t1, t2): the slot's query gradient
    dqs = t1 + t2 (through the numerator, through the denominator: with ONE token they cancel, train_attn_ref) and its
    record, from the GIVEN A and ks.  The launch writes nothing for a dead slot; its rows are 0 here."""
    M, d, Ln = q.shape
    Rn, dh = qi.shape[0], d // H
    alive, qh, Qp, As, kss = _slot_operands(q, A, ks, qi, si, H)
    if fault == "half_dead":                    # only a slot with BOTH indices outside [0, M) counts as dead
        alive = ((qi >= 0) & (qi < M)) | ((si >= 0) & (si < M))
    if fault == "dead":                         # no slot is: each computes with its indices clamped into [0, M)
        alive = torch.ones_like(alive)
    g = _heads(dout, H)
    z = 1.0 / (torch.einsum("rhil,rhi->rhl", Qp, kss) + eps)
    num = torch.einsum("rhil,rhiv->rhvl", Qp, As)
    dnum = g * z.unsqueeze(2) * Ln
    dden = -z * z * Ln * (g * num).sum(dim=2)
    t1 = torch.einsum("rhiv,rhvl->rhil", As, dnum) * R._elu1_grad(qh)
    t2 = dden.unsqueeze(2) * kss.unsqueeze(3) * R._elu1_grad(qh)
    dA = torch.einsum("rhil,rhvl->rhiv", Qp, dnum)
    dks = torch.einsum("rhl,rhil->rhi", dden, Qp)
    if fault == "rec_layout":
        rec = torch.cat([dA, dks.unsqueeze(3)], dim=3).reshape(Rn, H, dh * (dh + 1))
    else:
        rec = torch.cat([dA.reshape(Rn, H, dh * dh), dks], dim=2)
    a3, a4 = alive.view(-1, 1, 1).to(q.dtype), alive.view(-1, 1, 1, 1).to(q.dtype)
    return (t1 + t2).reshape(Rn, d, Ln) * a3, rec * a3, ((t1 * a4).reshape(Rn, d, Ln), (t2 * a4).reshape(Rn, d, Ln))


def pairs_state_bwd(k, v, drec, H):
    """k, v (M,d,L), drec (M,H,dh (dh + 1)) GIVEN -> dk, dv (M,d,L), (u1, u2): dk = u1 + u2 = elu'(k) (dA V' + dks),
    dv = dA^T K' / L"""
    M, d, Ln = k.shape
    dh = d // H
    kh = _heads(k, H)
    Kp, Vp = R._elu1(kh), _heads(v, H) / Ln
    dA, dks = drec[..., :dh * dh].reshape(M, H, dh, dh), drec[..., dh * dh:]
    u1 = torch.einsum("mhiv,mhvs->mhis", dA, Vp) * R._elu1_grad(kh)
    u2 = dks.unsqueeze(3) * R._elu1_grad(kh)
    dv = torch.einsum("mhis,mhiv->mhvs", Kp, dA) / Ln
    return (u1 + u2).reshape(M, d, Ln), dv.reshape(M, d, Ln), (u1.reshape(M, d, Ln), u2.reshape(M, d, Ln))


def _sum_lists(qi, si, M, fault=None):
    """the lists the two index sums run over: a dead slot names no object in EITHER"""
    if fault == "dead":
        return qi.clamp(0, M - 1), si.clamp(0, M - 1)
    if fault == "half_dead":                    # the lists as they came: the live index of a half-dead slot names its object
        return qi, si
    dead = torch.full_like(qi, -1)
    alive = _alive(qi, si, M)
    return torch.where(alive, qi, dead), torch.where(alive, si, dead)


def linattn_pairs_indexed(q, k, v, qi, si, H, eps, dout=None, fault=None):
    """the same through the kernels' decomposition: state per object, apply per slot, records per slot, index sums, state
    backward per object -> out [, dq, dk, dv, rec (R,H,dh (dh + 1)), drec (M,H,dh (dh + 1))]"""
    M = q.shape[0]
    Rn = qi.shape[0]
    if fault == "swap":
        qi, si = si, qi
    A, ks = pairs_state_fwd(k, v, H, fault)
    out = pairs_apply_fwd(q, A, ks, qi, si, H, eps)
    if dout is None:
        return out
    dqs, rec, _ = pairs_apply_bwd(q, A, ks, qi, si, H, eps, dout, fault)
    sum_q, sum_s = _sum_lists(qi, si, M, fault)
    n = Rn // 2 if fault == "one_direction" else 1024 if fault == "round_1024" else None
    dq = index_sum_ref(dqs, sum_q, n, M)
    drec = index_sum_ref(rec, sum_s, n, M)
    dk, dv, _ = pairs_state_bwd(k, v, drec, H)
    return out, dq, dk, dv, rec, drec


def linattn_pairs_scales(q, k, v, qi, si, H, eps, dout):
    """-> dict(dq, dk, dv) (M,d,L): per element, the sum over the live slots of the ABSOLUTE contributions that the
    gradient is the sum of -- |t1| + |t2| of every slot for dq, |u1| + |u2| of every slot's own record for dk, |dv| of it
    for dv.  A float32 sum in list order rounds in proportion to this, not to the (possibly cancelling) result."""
    M = q.shape[0]
    A, ks = pairs_state_fwd(k, v, H)
    _, rec, (t1, t2) = pairs_apply_bwd(q, A, ks, qi, si, H, eps, dout)
    sum_q, sum_s = _sum_lists(qi, si, M)
    ss = si.clamp(0, M - 1)
    dks_, dvs, (u1, u2) = pairs_state_bwd(k[ss], v[ss], rec, H)       # every slot's record against its own object
    return dict(dq=index_sum_ref(t1.abs() + t2.abs(), sum_q, None, M),
                dk=index_sum_ref(u1.abs() + u2.abs(), sum_s, None, M), dv=index_sum_ref(dvs.abs(), sum_s, None, M))
