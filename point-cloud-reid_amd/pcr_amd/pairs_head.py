"""The `concat` matching head over per-object embeddings (include/pcr.h, section A10; csrc/pair_kernels.hip).

A pair's head input is [e_i | e_j], and LinearRes.linear1 has no bias, so W1 [e_i ; e_j] = u[i] + v[j] with two tables
computed once per OBJECT; what is left per pair -- two GroupNorms, the n x n product with linear2, the residual and the
output dot product -- is one launch over the whole pair list (pcr_pair_head_f32).  The tables and the launch run f32-input
MFMA whatever engine.PRECISION says: a stored embedding is scored the same in every mode."""
import ctypes

import torch

from . import _lib as L
from . import engine as E
from ._lib import _p
from .abi import PairHeadParams


class PairHeadPlan:
    """packed [LinearRes(n, n, GN), Linear(n, 1)] head; n = 2F"""

    def __init__(self, match_head, device):
        from mmdet3d.models.lanegcn_nets import LinearRes
        if not (isinstance(match_head, torch.nn.Sequential) and len(match_head) == 2
                and isinstance(match_head[0], LinearRes) and isinstance(match_head[1], torch.nn.Linear)):
            raise L.PcrError("pairs_head: the match head must be [LinearRes, Linear] as in every ReID config")
        res, out = match_head[0], match_head[1]
        n = res.linear1.weight.shape[0]
        if res.transform is not None or res.linear1.weight.shape[1] != n:
            raise L.PcrError("pairs_head: LinearRes with n_in == n_out only (got %d -> %d)"
                             % (res.linear1.weight.shape[1], n))
        if tuple(out.weight.shape) != (1, n) or out.bias is None:
            raise L.PcrError("pairs_head: the head must end in Linear(%d, 1) with a bias" % n)
        L.require_default_eps(res.norm1, res.norm2)
        if res.norm1.num_groups != res.norm2.num_groups:
            raise L.PcrError("pairs_head: norm1 and norm2 must have the same groups")
        self.n, self.F, self.groups = n, n // 2, res.norm1.num_groups
        if n % 2 or not L.load().pcr_pair_head_ok(self.F, self.groups):
            raise L.PcrError("pairs_head: head width %d with %d GroupNorm groups is not covered (pcr_pair_head_ok: F in "
                             "{32, 64, 128}, groups of 4 / 8 / 16 / 32 channels)" % (n, self.groups))
        w1 = res.linear1.weight.detach()
        # f32-only images (no ._pcr_bf): engine.dense then takes the f32 launch in every precision mode
        self.wu = E.pack_weight(w1[:, :self.F], device)
        self.wv = E.pack_weight(w1[:, self.F:], device)
        self.t = dict(w2p=E.pack_weight(res.linear2.weight, device),
                      gn1_g=E._dev32(res.norm1.weight, device), gn1_b=E._dev32(res.norm1.bias, device),
                      gn2_g=E._dev32(res.norm2.weight, device), gn2_b=E._dev32(res.norm2.bias, device),
                      w_out=E._dev32(out.weight.reshape(-1), device), b_out=E._dev32(out.bias.reshape(-1), device))


def plan(match_head, device):
    """the head's plan on `device`, rebuilt when a parameter changed (engine.param_version)"""
    key = (str(device), E.param_version(match_head))
    if getattr(match_head, "_pcr_pair_key", None) != key:
        object.__setattr__(match_head, "_pcr_pair_plan", PairHeadPlan(match_head, device))
        object.__setattr__(match_head, "_pcr_pair_key", key)
    return match_head._pcr_pair_plan


def _emb(pl, emb):
    emb = L.tensor(emb, "pairs_head", "emb", torch.float32, shape=(None, pl.F), copy=True)
    L.require_cuda(emb)
    return emb


def tables(pl, emb):
    """emb (M, F) -> u, v (M, n): u = emb W1[:, :F]^T, v = emb W1[:, F:]^T, through the f32 dense launch"""
    emb = _emb(pl, emb)
    M = emb.shape[0]
    if M == 0:
        z = torch.empty((0, pl.n), dtype=torch.float32, device=emb.device)
        return z, z.clone()
    x = emb.unsqueeze(0).transpose(1, 2)            # (1, F, M) as the transposed view of a point-major tensor
    u = E.dense(x, pl.wu, pl.n)[0].t().contiguous()
    v = E.dense(x, pl.wv, pl.n)[0].t().contiguous()
    return u, v


def pair_logits(pl, emb, u, v, pairs, count=None, dead_value=0.0, out=None):
    """logits (P,) of pairs (P, 2) (any integer dtype; int32 goes in as it is) over emb (M, F) and its tables.
    count ((1,) int32 device tensor; None: every pair): pairs[count:] are neither read nor scored and get dead_value.
    A live pair with an index outside [0, M) gets NaN."""
    emb = _emb(pl, emb)
    M = emb.shape[0]
    u = L.tensor(u, "pairs_head", "u", torch.float32, shape=(M, pl.n))
    v = L.tensor(v, "pairs_head", "v", torch.float32, shape=(M, pl.n))
    if not isinstance(pairs, torch.Tensor) or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point:
        L.refuse("pairs_head", "pairs must be a (P, 2) integer tensor")
    pairs = pairs.to(device=emb.device, dtype=torch.int32).contiguous()
    P = pairs.shape[0]
    logits = L.out_tensor(out, "pairs_head", "out", torch.float32, (P,), emb.device)
    L.require_cuda(u, v, pairs, logits)
    p = PairHeadParams()
    p.M, p.F, p.n, p.groups, p.P = M, pl.F, pl.n, pl.groups, P
    p.emb, p.u, p.v, p.pairs, p.logits = _p(emb), _p(u), _p(v), _p(pairs), _p(logits)
    for k, t in pl.t.items():
        setattr(p, k, _p(t))
    live = None
    if count is not None:
        if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.numel() != 1:
            L.refuse("pairs_head", "count must be a (1,) int32 device tensor")
        live = ctypes.byref(E._live_block((count.reshape(1).contiguous(), max(P, 1), 0)))
    with E._prof("pair_head[n=%d]" % pl.n, 2.0 * P * pl.n * pl.n, 4.0 * P * (3 + 3 * pl.n), arith="lib"):
        L.run.pcr_pair_head_f32(ctypes.byref(p), live, ctypes.byref(ctypes.c_float(dead_value)), L.stream_ptr())
    return logits
