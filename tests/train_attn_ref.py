"""float64 references of the Point-Transformer training ops (pcr_amd.train_ops: LinAttn / LinAttnQKV / LinAttnKV, TNorm,
LocalAttn, PoolPair) and the conditioning of the token norm's test inputs.  Plain torch on the CPU, written from the
statements of include/pcr.h and the reference project's formulas (LinearAttention, pointnet2_utils.py:26-47;
local_self_attention, attention.py:262-296; get_pooled_feats 'both', ReIDNet.py:529-532); nothing here imports pcr_amd.
Every function computes in the dtype of its inputs: float64 is the reference, the same call on float32 tensors is the
"float32 evaluation of the same formula" that some bounds of test_gpu_train_attn_ops.py are measured with.

Every backward is written out term by term (`*_bwd_ref`); test_train_attn_ref_cpu.py holds each to float64 autograd of the
reference project's own formulation.  `linattn_bwd_ref` also returns the two terms of dq, and of dk, BEFORE their sum:
with one key (Sk = 1) out = v a / (a + eps), a = Q'.K', hardly depends on q or k, the terms cancel to eps / (a + eps) of
themselves (to nothing at eps = 0), and a comparison relative to max|dq| or max|dk| would compare rounding with rounding
-- the terms are the scale.  The local attention does the same row by row: a point whose K listed neighbours are ONE
distinct point has msg_i = v_j a / (a + eps), and `local_attn_bwd_ref` returns the scale of the two parts of da that
cancel.  (tools/fuzz_train.py avoids Sk = 1 with "one key: dq = 0 in exact arithmetic": that holds at eps = 0 only, and
dk shares it.)

Decisions.  The linear-attention and local-attention cores take NONE: elu(x) + 1 is C1, elu'(x) = 1 (x > 0) | exp(x)
is continuous at 0 (a kernel that branches on q > 0 where the reference branches on q >= 0 changes nothing), and the
maximum of PoolPair compares float32 inputs as they are.  Their inputs are used as drawn.  The token norm with a ReLU
does decide, on the sign of z = (x - mean) rstd gamma + beta [+ res]: an element is MARGINAL when |z| < REL_DELTA max|z|
(train_ref's margin: ~100 x the float32 error of z), and `condition_tnorm` moves the offending x to +- 2 delta on its own
side.  A token's mean and rstd move with the edit, hence the loop; it ends with ZERO marginal elements.  Where x has no
say -- gamma = 0, or a group of one channel, where x - mean = 0 -- z = beta [+ res], and the residual is moved instead
(without one, beta itself must be clear of zero)."""
import torch

from train_ref import MAX_PASSES, REL_DELTA, first_argmax

F64 = torch.float64


def _elu1(x):
    """elu(x) + 1"""
    return torch.where(x > 0, x + 1.0, torch.exp(torch.clamp(x, max=0.0)))


def _elu1_grad(x):
    """d (elu(x) + 1) / dx: 1 for x > 0, exp(x) else (continuous at 0)"""
    return torch.where(x > 0, torch.ones_like(x), torch.exp(torch.clamp(x, max=0.0)))


# ------------------------------------------------------------------------------------ linear attention --
def _kv_source(B, kv_roll):
    """src[b] = the cloud whose keys / values query cloud b reads"""
    return (torch.arange(B) + kv_roll) % B


def _heads(t, H):
    B, d, Ln = t.shape
    return t.reshape(B, H, d // H, Ln)


def linattn_ref(q, k, v, H, eps, kv_roll=0):
    """q (B,d,Lq), k, v (B,d,Sk) -> (out (B,d,Lq), A (B,H,dh,dh), ks (B,H,dh)): per (cloud, head) Q' = elu(q) + 1,
    K' = elu(k) + 1, V' = v / Sk, A = sum_s K'_s V'_s^T, ks = sum_s K'_s, out_l = (Q'_l^T A) Sk / (Q'_l . ks + eps); query
    cloud b reads the keys / values of cloud (b + kv_roll) mod B"""
    B, d, Lq = q.shape
    Sk = k.shape[2]
    src = _kv_source(B, kv_roll)
    Qp, Kp, Vp = _elu1(_heads(q, H)), _elu1(_heads(k[src], H)), _heads(v[src], H) / Sk
    A = torch.einsum("bhis,bhvs->bhiv", Kp, Vp)
    ks = Kp.sum(dim=3)
    den = torch.einsum("bhil,bhi->bhl", Qp, ks) + eps
    num = torch.einsum("bhil,bhiv->bhvl", Qp, A)
    out = num * Sk / den.unsqueeze(2)
    return out.reshape(B, d, Lq), A, ks


def linattn_bwd_ref(q, k, v, H, eps, dout, kv_roll=0, A=None, ks=None):
    """-> (dq, dk, dv, (t1, t2), (u1, u2)): the gradients of linattn_ref for the output gradient dout, term by term;
    dq = t1 + t2 with t1 = elu'(q) A dnum (through the numerator) and t2 = elu'(q) dden ks (through the denominator), and
    dk = u1 + u2 with u1 = elu'(k) dA V', u2 = elu'(k) dks likewise: with ONE key both pairs cancel.  A / ks: the saved
    records to differentiate with (default: the forward's own) -- the backward LAUNCH reads them, it does not recompute
    them.  dk / dv land on the clouds the keys / values were read from."""
    B, d, Lq = q.shape
    Sk = k.shape[2]
    src = _kv_source(B, kv_roll)
    qh, kh = _heads(q, H), _heads(k[src], H)
    Qp, Kp, Vp = _elu1(qh), _elu1(kh), _heads(v[src], H) / Sk
    if A is None:
        A, ks = torch.einsum("bhis,bhvs->bhiv", Kp, Vp), Kp.sum(dim=3)
    g = _heads(dout, H)
    z = 1.0 / (torch.einsum("bhil,bhi->bhl", Qp, ks) + eps)                       # (B,H,Lq)
    num = torch.einsum("bhil,bhiv->bhvl", Qp, A)
    dnum = g * z.unsqueeze(2) * Sk                                                 # (B,H,dh,Lq)
    dden = -z * z * Sk * (g * num).sum(dim=2)                                      # (B,H,Lq)
    t1 = torch.einsum("bhiv,bhvl->bhil", A, dnum) * _elu1_grad(qh)
    t2 = dden.unsqueeze(2) * ks.unsqueeze(3) * _elu1_grad(qh)
    dA = torch.einsum("bhil,bhvl->bhiv", Qp, dnum)
    dks = torch.einsum("bhl,bhil->bhi", dden, Qp)
    u1 = torch.einsum("bhiv,bhvs->bhis", dA, Vp) * _elu1_grad(kh)
    u2 = (dks.unsqueeze(3) * _elu1_grad(kh)).expand_as(u1)
    dVp = torch.einsum("bhis,bhiv->bhvs", Kp, dA)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    dk[src] = (u1 + u2).reshape(B, d, Sk)
    dv[src] = (dVp / Sk).reshape(B, d, Sk)
    return ((t1 + t2).reshape(B, d, Lq), dk, dv, (t1.reshape(B, d, Lq), t2.reshape(B, d, Lq)),
            (u1.reshape(B, d, Sk), u2.reshape(B, d, Sk)))


# ------------------------------------------------------------------------------------------ token norm --
def _groups(x, G):
    B, C, Ln = x.shape
    return x.reshape(B, G, C // G, Ln)


def tnorm_ref(x, gamma, beta, res, G, eps, relu):
    """x (B,C,L) -> (y, mean (B,G,L), rstd (B,G,L), z): every token normalised over each of its G groups of C / G
    consecutive channels with the BIASED variance, z = (x - mean) rstd gamma + beta [+ res], y = relu(z) | z"""
    B, C, Ln = x.shape
    xg = _groups(x, G)
    mean = xg.mean(dim=2)
    var = ((xg - mean.unsqueeze(2)) ** 2).mean(dim=2)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = ((xg - mean.unsqueeze(2)) * rstd.unsqueeze(2)).reshape(B, C, Ln) * gamma.view(1, C, 1) + beta.view(1, C, 1)
    if res is not None:
        z = z + res
    return (torch.relu(z) if relu else z), mean, rstd, z


def tnorm_bwd_ref(x, gamma, beta, res, G, eps, relu, g):
    """-> (dx, dgamma, dbeta, dres | None): go = g [z > 0] (relu) | g; dres = go; dbeta = sum go, dgamma = sum go xhat over
    (B, L); dx = rstd (go gamma - mean_group(go gamma) - xhat mean_group(go gamma xhat))"""
    B, C, Ln = x.shape
    _, mean, rstd, z = tnorm_ref(x, gamma, beta, res, G, eps, relu)
    go = torch.where(z > 0, g, torch.zeros_like(g)) if relu else g
    xh = ((_groups(x, G) - mean.unsqueeze(2)) * rstd.unsqueeze(2))                 # (B,G,gs,L)
    gv = _groups(go * gamma.view(1, C, 1), G)
    s1 = gv.mean(dim=2, keepdim=True)
    s2 = (gv * xh).mean(dim=2, keepdim=True)
    dx = (rstd.unsqueeze(2) * (gv - s1 - xh * s2)).reshape(B, C, Ln)
    xh = xh.reshape(B, C, Ln)
    return dx, (go * xh).sum(dim=(0, 2)), go.sum(dim=(0, 2)), (go if res is not None else None)


def _tnorm_dead(x, gamma, G):
    """elements whose z does not depend on x: gamma = 0, or a group of ONE channel (x - mean = 0)"""
    B, C, Ln = x.shape
    dead = (gamma == 0).view(1, C, 1).expand(B, C, Ln)
    return torch.ones_like(dead) if C == G else dead


def tnorm_marginals(x, gamma, beta, res, G, eps, rel=REL_DELTA):
    """number of elements of the float32 input whose ReLU argument z lies within delta = rel max|z| of zero"""
    z = tnorm_ref(x.to(F64), gamma.to(F64), beta.to(F64), None if res is None else res.to(F64), G, eps, True)[3]
    return int((z.abs() < rel * z.abs().max()).sum())


def condition_tnorm(x, gamma, beta, res, G, eps, rel=REL_DELTA):
    """float32 (x, res | None) -> (x', res', elements moved): every element with |z| < delta goes to +- 2 delta on its own
    side, through x where x has a say, through res where it has none (see the module text); repeated, with the token
    statistics of the edited x, until nothing is marginal"""
    gamma64, beta64 = gamma.to(F64), beta.to(F64)
    B, C, Ln = x.shape
    moved = 0
    for _ in range(MAX_PASSES):
        x64 = x.to(F64)
        r64 = None if res is None else res.to(F64)
        _, mean, rstd, z = tnorm_ref(x64, gamma64, beta64, r64, G, eps, True)
        delta = rel * float(z.abs().max())
        marg = z.abs() < delta
        if not bool(marg.any()):
            return x, res, moved
        moved += int(marg.sum())
        want = 2.0 * delta * torch.where(z < 0, -torch.ones_like(z), torch.ones_like(z))
        dead = _tnorm_dead(x64, gamma64, G)
        assert res is not None or not bool((marg & dead).any()), "beta of a channel without say of x is marginal"
        scale = (rstd.unsqueeze(2).expand(B, G, C // G, Ln).reshape(B, C, Ln) * gamma64.view(1, C, 1))
        safe = torch.where(scale != 0, scale, torch.ones_like(scale))
        x = torch.where(marg & ~dead, x64 + (want - z) / safe, x64).to(torch.float32)
        if res is not None:
            res = torch.where(marg & dead, r64 + (want - z), r64).to(torch.float32)
    raise AssertionError("conditioning did not settle")


# ------------------------------------------------------------------------------------- local attention --
def _neighbours(t, idx):
    """t (B,H,dh,N), idx (B,N,K) -> (B,H,dh,N,K): t at every point's neighbours"""
    return torch.stack([t[b][:, :, idx[b].long()] for b in range(t.shape[0])])


def local_attn_ref(qkv, idx, H, eps):
    """qkv (B,3C,N) = [q ; k ; v] per point, idx (B,N,K) -> msg (B,C,N): msg_i = sum_j a_ij v_j / (sum_j a_ij + eps),
    a_ij = <elu(q_i) + 1, elu(k_j) + 1> per head, j over the K listed neighbours of i (a neighbour listed twice counts
    twice)"""
    B, C3, N = qkv.shape
    C = C3 // 3
    Qp = _elu1(_heads(qkv[:, :C], H))
    Kn = _neighbours(_elu1(_heads(qkv[:, C:2 * C], H)), idx)
    Vn = _neighbours(_heads(qkv[:, 2 * C:], H), idx)
    a = torch.einsum("bhdn,bhdnk->bhnk", Qp, Kn)
    den = a.sum(dim=3) + eps
    return (torch.einsum("bhnk,bhdnk->bhdn", a, Vn) / den.unsqueeze(2)).reshape(B, C, N)


def local_attn_bwd_ref(qkv, idx, H, eps, g):
    """-> (dqkv (B,3C,N), edge (B,2C,N,K), scale): with da_ij = (g_i . v_j - g_i . msg_i) / z_i per head, dq_i = elu'(q_i)
    sum_j da_ij K'_j, and per EDGE d k_j += da_ij Q'_i elu'(k_j), d v_j += a_ij / z_i g_i -- edge holds these two terms,
    dqkv their sums over the edges that cite point j, added in index order (a point nobody cites gets exactly 0).
    scale = dict(dq, dk, ek): the maximum of the larger of the two terms of each -- the g . v_j part and the g . msg part of
    da -- BEFORE they are subtracted.  Where a row lists ONE distinct neighbour (K = 1, a point that is all its own
    neighbours) msg_i = v_j a / (a + eps) hardly depends on q or k: the parts cancel as dq and dk of the linear attention do
    with one key, and the scale stands in for max|dq|, max|dk|."""
    B, C3, N = qkv.shape
    C, K = C3 // 3, idx.shape[2]
    qh, kh = _heads(qkv[:, :C], H), _heads(qkv[:, C:2 * C], H)
    Qp = _elu1(qh)
    Kn = _neighbours(_elu1(kh), idx)
    Vn = _neighbours(_heads(qkv[:, 2 * C:], H), idx)
    a = torch.einsum("bhdn,bhdnk->bhnk", Qp, Kn)
    z = a.sum(dim=3) + eps                                                         # (B,H,N)
    msg = torch.einsum("bhnk,bhdnk->bhdn", a, Vn) / z.unsqueeze(2)
    gh = _heads(g, H)
    parts = (torch.einsum("bhdn,bhdnk->bhnk", gh, Vn) / z.unsqueeze(3),
             ((gh * msg).sum(dim=2) / z).unsqueeze(3).expand(B, H, N, K))         # da = parts[0] - parts[1]
    da = parts[0] - parts[1]
    dq = torch.einsum("bhnk,bhdnk->bhdn", da, Kn) * _elu1_grad(qh)
    kgrad = Qp.unsqueeze(4) * _neighbours(_elu1_grad(kh), idx)                     # (B,H,dh,N,K)
    ek = da.unsqueeze(2) * kgrad
    ev = (a / z.unsqueeze(3)).unsqueeze(2) * gh.unsqueeze(4)
    edge = torch.cat([ek.reshape(B, C, N, K), ev.reshape(B, C, N, K)], dim=1)

    def fold(e):
        out = torch.zeros(B, e.shape[1], N, dtype=qkv.dtype)
        for b in range(B):
            out[b].index_add_(1, idx[b].long().reshape(-1), e[b].reshape(e.shape[1], N * K))
        return out
    big = lambda ts: max(float(t.abs().max()) for t in ts)     # noqa: E731
    scale = dict(dq=big([torch.einsum("bhnk,bhdnk->bhdn", p, Kn) * _elu1_grad(qh) for p in parts]),
                 dk=big([fold((p.unsqueeze(2) * kgrad).reshape(B, C, N, K)) for p in parts]),
                 ek=big([p.unsqueeze(2) * kgrad for p in parts]))
    return torch.cat([dq.reshape(B, C, N), fold(edge)], dim=1), edge, scale


# ------------------------------------------------------------------------------------------- pair pool --
def _pairs(o):
    """o (2P,C,L) -> (P,C,2L): clouds p and p + P concatenated along the points"""
    P = o.shape[0] // 2
    return torch.cat([o[:P], o[P:]], dim=2)


def pool_pair_ref(o):
    """o (2P,C,L) -> (pooled (P,2C) = [max, mean] over the 2L points of pair p, arg (P,C) = the FIRST position of the
    maximum in the point-concatenated pair: an equal maximum in both halves belongs to the first)"""
    x = _pairs(o)
    arg = first_argmax(x, 2)
    mx = torch.gather(x, 2, arg.unsqueeze(2)).squeeze(2)
    return torch.cat([mx, x.mean(dim=2)], dim=1), arg


def pool_pair_bwd_ref(g, arg, L):
    """g (P,2C) -> dout (2P,C,L): the max half to position arg of the pair, the mean half / 2L to every position"""
    P, C = arg.shape
    d = (g[:, C:] / (2 * L)).unsqueeze(2).expand(P, C, 2 * L).clone()
    d.scatter_add_(2, arg.unsqueeze(2), g[:, :C].unsqueeze(2))
    return torch.cat([d[:, :, :L], d[:, :, L:]], dim=0)
