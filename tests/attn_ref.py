"""float64 restatement of the inference linear-attention block (pcr_attn_kv_f32 / pcr_attn_apply_f32), written from the
`pcr_attn_params` comment of include/pcr.h -- "M, ksum, then apply" -- and not from oracle/model_oracle.py, which
evaluates the same block the reference's way (projections, einsum attention, merge).  Plain torch on the CPU; nothing
here imports pcr_amd or the oracle.  tests/test_attn_ref_cpu.py holds the two formulations against each other.

Layouts are the launches': features (B, c, L) channel-major, coordinates (B, L, 3), output (B, cout or cfinal, Lq).
`sd` is the block's state dict (pos MLP under `pos_name`, q_proj / k_proj / v_proj / merge, mlp.0 / mlp.2, norm1 / norm2);
every tensor is taken to float64 on entry.

Every matrix product goes through ONE hook, mm(x, w) = x w^T (w (cout, cin) or a batch of them), exact float64 by
default.  `split_mm` is the operand model of the split-bf16 mode: both operands as hi = bf16(x), lo = bf16(x - hi)
(round to nearest even), y = x_hi w_hi + x_hi w_lo + x_lo w_hi accumulated in float64, the lo x lo term dropped.  The
3-input first layer of the position MLP is never split (the kernels keep it in f32 fmaf chains)."""
import torch
import torch.nn.functional as F

F64 = torch.float64
LN_EPS = 1e-5
ATTN_EPS = 1e-6


def exact_mm(x, w):
    """x (..., cin), w (cout, cin) or (B, cout, cin) -> (..., cout)"""
    return x @ w.transpose(-1, -2)


def _bf16(x):
    return x.to(torch.bfloat16).to(F64)


def _split(x):
    hi = _bf16(x)
    return hi, _bf16(x - hi)


def split_mm(x, w):
    xh, xl = _split(x)
    wh, wl = _split(w)
    return exact_mm(xh, wh) + exact_mm(xh, wl) + exact_mm(xl, wh)


def _w(sd, name):
    return sd[name].detach().to(F64)


def _tok(feat):
    """(B, c, L) -> token-major (B, L, c) float64"""
    return feat.detach().to(F64).transpose(1, 2)


def _ln(x, g, b):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + LN_EPS) * g + b


def _phi(x):
    return F.elu(x) + 1.0


def pos_encoding(sd, pos_name, xyz, mm=exact_mm):
    """pos = W2 relu(W0 xyz + b0) + b2: xyz (B, L, 3) -> (B, L, c)"""
    h = torch.relu(exact_mm(xyz.detach().to(F64), _w(sd, pos_name + ".0.weight")) + _w(sd, pos_name + ".0.bias"))
    return mm(h, _w(sd, pos_name + ".2.weight")) + _w(sd, pos_name + ".2.bias")


def kv_state(sd, pos_name, feat_k, xyz_k, nhead, k_pos, mm=exact_mm, stages=None):
    """key side of every cloud -> (M (B, d, d), ksum (B, d)):  K = elu(Wk (x + k_pos pos)) + 1,  V = Wv (x + pos) / Sk,
    KV[dd][v] = sum_s K[s][dd] V[s][v] per head,  M[o][dd] = sum_{v in head(dd)} Wm[o][v] KV[dd][v],  ksum = sum_s K"""
    x = _tok(feat_k)
    B, Sk, _ = x.shape
    pos = pos_encoding(sd, pos_name, xyz_k, mm)
    K = _phi(mm(x + pos if k_pos else x, _w(sd, "k_proj.weight")))
    V = mm(x + pos, _w(sd, "v_proj.weight")) / Sk
    Wm = _w(sd, "merge.weight")
    d = K.shape[-1]
    dh = d // nhead
    M = torch.zeros(B, d, d, dtype=F64)
    for h in range(nhead):
        hs = slice(h * dh, (h + 1) * dh)
        KV = mm(K[:, :, hs].transpose(1, 2), V[:, :, hs].transpose(1, 2))      # (B, dd, v)
        M[:, :, hs] = mm(KV, Wm[:, hs]).transpose(1, 2)                        # (B, dd, o) -> [o][dd]
    ksum = K.sum(dim=1)
    if stages is not None:
        stages.update(K=K, V=V, M=M, ksum=ksum)
    return M, ksum


def apply_block(sd, pos_name, feat_q, xyz_q, M, ksum, Sk, nhead, q_pos, residual, final=None, kv_index=None,
                q_index=None, n_out=None, pooled=False, mm=exact_mm, stages=None):
    """query side.  Virtual cloud b reads the tokens of cloud q_index[b] (default b) and the state of cloud kv_index[b]
    (default b); n_out virtual clouds (default: one per query cloud).  final = (W (cfinal, cout), b (cfinal)): the
    trailing 1x1 conv.  pooled: (B, 2, cout) = [max | sum] over the tokens instead of the block output.
    stages, when a dict, receives Q' (`Qn`), `msg` (after norm1), `ff` (feed-forward output before norm2) and `out`."""
    x = _tok(feat_q)
    xyz = None if xyz_q is None else xyz_q.detach().to(F64)
    n = n_out if n_out is not None else x.shape[0]
    qi = torch.arange(n) if q_index is None else torch.as_tensor(q_index).long()[:n]
    ki = torch.arange(n) if kv_index is None else torch.as_tensor(kv_index).long()[:n]
    x = x[qi]
    M, ksum = M[ki], ksum[ki]
    xq = x + pos_encoding(sd, pos_name, xyz[qi], mm) if q_pos else x
    Q = _phi(mm(xq, _w(sd, "q_proj.weight")))                                   # (B, L, d)
    B, L, d = Q.shape
    dh = d // nhead
    den = (Q * ksum.unsqueeze(1)).view(B, L, nhead, dh).sum(dim=-1, keepdim=True) + ATTN_EPS
    Qn = (Q.view(B, L, nhead, dh) * Sk / den).reshape(B, L, d)
    msg = _ln(mm(Qn, M), _w(sd, "norm1.weight"), _w(sd, "norm1.bias"))
    hid = torch.relu(mm(torch.cat([x, msg], dim=2), _w(sd, "mlp.0.weight")))
    ff = mm(hid, _w(sd, "mlp.2.weight"))
    out = _ln(ff, _w(sd, "norm2.weight"), _w(sd, "norm2.bias"))
    if residual:
        out = out + x
    if final is not None:
        out = mm(out, final[0].detach().to(F64)) + final[1].detach().to(F64)
    if stages is not None:
        stages.update(Q=Q, Qn=Qn, msg=msg, ff=ff, out=out)
    out = out.transpose(1, 2).contiguous()
    if pooled:
        return torch.stack([out.amax(dim=2), out.sum(dim=2)], dim=1)
    return out


def _block(sd, pos_name, feat_q, xyz_q, feat_k, xyz_k, nhead, q_pos, k_pos, residual, mm, stages, **kw):
    M, ksum = kv_state(sd, pos_name, feat_k, xyz_k, nhead, k_pos, mm=mm, stages=stages)
    return apply_block(sd, pos_name, feat_q, xyz_q, M, ksum, feat_k.shape[2], nhead, q_pos, residual, mm=mm,
                       stages=stages, **kw)


# the three blocks' flags, as the modules' plan() calls set them: position MLP, q_pos, k_pos, residual
FLAGS = {"self": ("pos_mlp", 1, 1, 1), "cross": ("pos_mlp", 0, 0, 1), "fp": ("pos_mlp2", 0, 0, 0)}


def self_attention(sd, feat, xyz, nhead=2, mm=exact_mm, stages=None, **kw):
    """Self_Attention: queries, keys and values carry the position encoding; residual"""
    return _block(sd, FLAGS["self"][0], feat, xyz, feat, xyz, nhead, *FLAGS["self"][1:], mm, stages, **kw)


def cross_attention(sd, search, search_xyz, template, template_xyz, nhead=2, mm=exact_mm, stages=None, **kw):
    """corss_attention: only the values carry the (template's) position encoding; residual on the search features"""
    return _block(sd, FLAGS["cross"][0], search, None, template, template_xyz, nhead, *FLAGS["cross"][1:], mm, stages, **kw)


def fp_sa(sd, feat1, xyz1, feat2, xyz2, nhead=2, final=None, mm=exact_mm, stages=None, **kw):
    """FP_SA: fine <- coarse, position encoding (pos_mlp2) on the values only, no residual, optional trailing conv"""
    return _block(sd, FLAGS["fp"][0], feat1, None, feat2, xyz2, nhead, *FLAGS["fp"][1:], mm, stages, final=final, **kw)
