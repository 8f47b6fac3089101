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
3-input first layer of the position MLP is never split (the kernels keep it in f32 fmaf chains).

The second half restates WHICH KERNEL a block gets (`kv_form`, `apply_form`): the dispatch rules written from
include/pcr.h and DESIGN.md 4.2, held to the library's own report (pcr_attn_launch_form) by tests/test_attn_ref_cpu.py."""
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


# ---- which kernel a block gets: the dispatch rules restated from include/pcr.h (pcr_attn_params, pcr_live,
# pcr_attn_launch_form) and DESIGN.md 4.2.  tests/test_attn_ref_cpu.py holds them to what the library itself reports. ------
PREC_F32, PREC_BF16X3 = 0, 1
MAX_DYN_LDS = 160 * 1024
# pcr_attn_launch_form's families: kernel name, positions of the bool template arguments
KERNELS = (("attn_kv_kernel", ()), ("attn_kv_kernel_o3", ()), ("attn_kv_kernel_o2", (4,)),
           ("attn_kv_stream64_kernel", (0, 1, 3)), ("attn_kv_stream32_kernel", ()), ("attn_kv_stream128_kernel", ()),
           ("attn_kv_wide_kernel", ()), ("attn_apply_kernel", ()), ("attn_apply_stream64_kernel", (0, 5)),
           ("attn_apply_stream128_kernel", ()))
(KV_TILE, KV_TILE_O3, KV_TILE_O2, KV_STREAM64, KV_STREAM32, KV_STREAM128, KV_WIDE, APPLY_TILE, APPLY_STREAM64,
 APPLY_STREAM128) = range(10)
BF_IMAGES = ("wq_bf", "wmlp0_bf", "wmlp2_bf", "wfinal_bf", "wkv_bf")
WIDE_IMAGES = ("wkv_wide", "bkv_wide", "wmerge_packed")


class Block:
    """what the dispatch reads of a pcr_attn_params block: the shape, the asked precision and WHICH optional operands it
    carries (`has`: names of the non-NULL ones among xyz_q, wfinal, bfinal, the WIDE_IMAGES, the BF_IMAGES, wmlp0_bf_xpad,
    kv_part, out, pool_out; every other pointer is taken as given)"""
    __slots__ = ("B", "Lq", "Sk", "c1", "c2", "d", "cout", "nhead", "q_pos", "residual", "cfinal", "kv_splits", "precision",
                 "has")

    def __init__(self, **kw):
        self.B, self.Lq, self.Sk, self.kv_splits, self.precision = 3, 32, 32, 0, 0
        self.q_pos = self.residual = self.cfinal = 0
        self.has = frozenset(("out",))
        for k, v in kw.items():
            setattr(self, k, v)


def images_of_plan(d, c1, c2, nhead, q_pos, cfinal):
    """the optional operands engine.AttnPlan builds for a block of this shape (its __init__), `out` included"""
    has = {"out"}
    if q_pos:
        has.add("xyz_q")
    if cfinal:
        has.update(("wfinal", "bfinal"))
    if d <= 128:
        if d % 32 == 0 and (d // nhead) % 32 == 0:
            has.add("wmerge_packed")
        if (d == 64 and c2 in (64, 128)) or (d == 32 and c2 == 32) or d == 128:
            has.add("wkv_bf")
        if d == 64 and c1 % 16:
            has.add("wmlp0_bf_xpad")
        has.update(("wq_bf", "wmlp0_bf", "wmlp2_bf"))
        if cfinal:
            has.add("wfinal_bf")
    else:
        has.update(WIDE_IMAGES)
    return frozenset(has)


def block_valid(b):
    """pcr.h: d_model in {32, 64, 96, 128} or wide (heads of 64 n <= 256 channels); c2 % 8 == 0; q_pos requires xyz_q and
    c1 == c2 == d; residual requires cout == c1; a trailing conv its weights and cout % 8 == 0; widths up to 512"""
    if b.B < 0 or min(b.Lq, b.Sk, b.c1, b.c2, b.cout, b.nhead) < 1:
        return False
    if b.d < 32 or b.d > 512 or b.d % 32 or b.d % b.nhead:
        return False
    dh = b.d // b.nhead
    if b.d > 128 and (b.d % 64 or dh % 64 or dh > 256):
        return False
    if b.c2 % 8 or b.cout > 512 or b.cfinal > 512:
        return False
    if b.q_pos and ("xyz_q" not in b.has or not b.c1 == b.c2 == b.d):
        return False
    if b.residual and b.cout != b.c1:
        return False
    if b.cfinal and ("wfinal" not in b.has or "bfinal" not in b.has or b.cout % 8):
        return False
    return True


def bf_unit(b):
    """pcr.h: precision != f32 and d <= 128 run the dense phases as split bf16 on the bf16 images -- where all of them are
    given and no layer is wider than 256"""
    return (b.precision != 0 and b.d <= 128 and max(2 * b.d, b.cout, b.cfinal) <= 256 and
            all(k in b.has for k in ("wq_bf", "wmlp0_bf", "wmlp2_bf")) and (not b.cfinal or "wfinal_bf" in b.has))


def live_ok(b):
    """pcr_attn_live_ok: d = c1 = c2 = cout = 64 without kv_splits"""
    return block_valid(b) and b.d == b.c1 == b.c2 == b.cout == 64 and b.kv_splits <= 1


def _stream64_apply_shape(b):
    """DESIGN.md 4.2, attn_apply_stream64_kernel at d = 64: (c1 = 64 | 32 | < 16 with the padded mlp[0] image) x
    (cout = 64 [+ trailing conv to 128] | cout = 128 | cout = 32 + trailing conv to 64), whole 32-token blocks"""
    plain = not b.q_pos and not b.residual
    c_in = b.c1 == 64 or (plain and (b.c1 == 32 or (b.c1 < 16 and "wmlp0_bf_xpad" in b.has)))
    c_out = ((b.cout == 64 and b.cfinal in (0, 128) and b.c1 >= 32) or
             (b.cout == 128 and not b.cfinal and not b.residual and b.c1 == 64) or
             (b.cout == 32 and b.cfinal == 64 and not b.residual and b.c1 < 16))
    return b.d == 64 and c_in and c_out and b.Lq % 32 == 0 and b.nhead in (1, 2, 4)


def pool_ok(b):
    """pcr_attn_apply_pool_ok: the wave-autonomous d = c1 = cout = 64 form without q_pos / trailing conv, bf16 unit"""
    return (block_valid(b) and _stream64_apply_shape(b) and b.c1 == 64 and b.cout == 64 and not b.cfinal and not b.q_pos
            and bf_unit(b))


def kv_tile_lds(b):
    """dynamic LDS of the tile kv kernel: [feat_k ; h] and the projection in place, (c2 + d + 3) rows of a 64-token
    (d <= 64) or 32-token tile + 4 d, or the fold buffer d (d + 1) + d if larger; + one float per thread"""
    rp = 32 * (2 if b.d <= 64 else 1) + 1
    return 4 * (max((b.c2 + b.d + 3) * rp + 4 * b.d, b.d * (b.d + 1) + b.d) + 256)


def apply_tile_lds(b):
    """dynamic LDS of the tile apply kernel: 128 / 64 / 32-token tiles for d <= 32 / <= 64 / wider"""
    T = 32 * (4 if b.d <= 32 else (2 if b.d <= 64 else 1))
    up = lambda x, m: (x + m - 1) // m * m      # noqa: E731
    rows = max(up(b.c1 + b.d, 8), 2 * b.d, up(b.cout, 32), up(b.cfinal, 32))
    return 4 * ((rows + 3 + b.nhead) * (T + 1) + 2 * (256 // T) * T + 7 * b.d + 2 * b.cout)


def apply_stream64_lds(b):
    """dynamic LDS of attn_apply_stream64_kernel: the bf16 weight images in 16-byte units (Q, mlp[0], mlp[2]) + scalars"""
    c1s, nd = (b.c1 + 15) // 16, b.d // 32
    units = (c1s + (2 * nd if b.q_pos else 0)) * nd * 128 + (c1s + 2 * nd) * nd * 256 + nd * (b.cout // 32) * 512
    return units * 16 + (448 + 256 + 64 * 8) * 4


def _form(arith, family, targs, twin, gated, splits=0, fold=0):
    """(arithmetic noted, family, template arguments, gated, effective splits, fold follows); a gated launch of a family
    without a gated twin is refused"""
    if gated and not twin:
        return None
    return (arith, family, tuple(int(x) for x in targs), int(gated), splits, fold)


def kv_form(b, gated=False):
    """the kv launch of block b (pcr_attn_kv_f32; gated: pcr_attn_kv_live_f32) -> _form, or None where it is refused"""
    if not block_valid(b) or (gated and not live_ok(b)):
        return None
    d, Sk, H = b.d, b.Sk, b.nhead
    if d > 128:                                      # wide: d / 64 workgroups per cloud, f32
        if not all(k in b.has for k in WIDE_IMAGES) or b.B > 65535:
            return None
        return _form(PREC_F32, KV_WIDE, (2 if 64 + d // H <= 256 else 3,), False, gated, 1, 0)
    if b.c2 < d or kv_tile_lds(b) > MAX_DYN_LDS:     # (the tile kernel's LDS decides whichever kernel would run)
        return None
    ns = max(b.kv_splits, 1)
    if ns > 1 and ("kv_part" not in b.has or ns > 64):
        return None
    ns = min(ns, -(-Sk // (64 if d <= 64 else 32)))  # at most one split per tile
    bf = bf_unit(b)
    bfk = bf and "wkv_bf" in b.has                   # split-bf16 projection
    whole = ns == 1 and Sk % 32 == 0                 # the wave-autonomous forms: whole clouds of whole 32-token blocks
    if whole and d == 64 and (b.c2 == 64 or (b.c2 == 128 and bfk and Sk >= 128)) and 64 % H == 0:
        wide = b.c2 == 128
        onew = bfk and not wide and Sk <= 128        # ONEW: one wave per cloud
        return _form(PREC_BF16X3 if bfk else PREC_F32, KV_STREAM64, (H >= 2, bfk, 8 if wide else 4, onew), not wide, gated, 1, 0)
    if whole and bfk and d == 32 and b.c2 == 32 and 32 % H == 0:
        return _form(PREC_BF16X3, KV_STREAM32, (), False, gated, 1, 0)
    if whole and bfk and d == 128 and b.c2 == 128 and Sk >= 256 and H in (2, 4):
        return _form(PREC_BF16X3, KV_STREAM128, (H,), False, gated, 1, 0)
    fold = int(ns > 1)                               # the tile kernels project in f32 in both units
    if d == 32:
        return _form(PREC_F32, KV_TILE, (2, 1, 2, 1), False, gated, ns, fold)
    if d == 64:
        return _form(PREC_F32, KV_TILE_O3, (2, 1, 1, 1), ns == 1, gated, ns, fold)
    if d == 128:
        return _form(PREC_F32, KV_TILE_O2, (1, 2, 1, 4, bfk and Sk >= 256), False, gated, ns, fold)
    return _form(PREC_F32, KV_TILE, (1, 2, 0, 4), False, gated, ns, fold)


def apply_form(b, gated=False):
    """the apply launch of block b (pcr_attn_apply_f32 / _live_f32; pooled where b carries pool_out) -> _form or None"""
    if not block_valid(b) or not ({"out", "pool_out"} & b.has):
        return None
    pooled = "pool_out" in b.has
    if (pooled and not pool_ok(b)) or (gated and not live_ok(b)) or b.B > 65535:
        return None
    if apply_tile_lds(b) > MAX_DYN_LDS:              # (the tile kernel's LDS decides whichever kernel would run)
        return None
    d, H, bf = b.d, b.nhead, bf_unit(b)
    arith = PREC_BF16X3 if bf else PREC_F32          # (the bf16 unit is split bf16 whatever was requested)
    if bf and b.Lq % 32 == 0:
        if d == b.c1 == b.cout == 128 and not b.cfinal and b.q_pos and b.residual and b.Lq >= 256 and H in (1, 2, 4):
            return _form(arith, APPLY_STREAM128, (H,), False, gated)
        if d == b.c1 == b.cout == 32 and not b.cfinal and H in (1, 2):
            return _form(arith, APPLY_STREAM64, (b.q_pos, 2, 0, 1, 1, 0), False, gated)
        if _stream64_apply_shape(b) and apply_stream64_lds(b) <= MAX_DYN_LDS:
            cf = 4 if b.cfinal else 0
            if pooled:
                return _form(arith, APPLY_STREAM64, (0, 4, 0, 2, 2, 1), True, gated)
            if b.cout == 128:
                return _form(arith, APPLY_STREAM64, (b.q_pos, 4, 0, 4, 2, 0), False, gated)
            if b.c1 < 16:
                return _form(arith, APPLY_STREAM64, (0, 1, 2, 1, 2, 0), False, gated)
            return _form(arith, APPLY_STREAM64, (b.q_pos, b.c1 // 16, cf, 2, 2, 0), b.c1 == 64, gated)
    wide = 2 * d > 128 or b.cout > 128 or b.cfinal > 128      # some layer has more than four 32-channel blocks
    if d <= 32:
        return _form(arith, APPLY_TILE, (4, 2 if wide else 1), False, gated)
    if d <= 64:
        return _form(arith, APPLY_TILE, (2, 2 if wide else 1), True, gated)
    widest = max(2 * d, b.cout, b.cfinal)            # rounds per wave: 8 blocks -> 2, 16 -> 4, 32 -> 8
    return _form(arith, APPLY_TILE, (1, 8 if widest > 512 else (4 if widest > 256 else 2)), False, gated)


def kernel_name(form):
    """a _form spelled as a kernel trace spells the instantiation, defaults filled in: `attn_kv_stream64_kernel<true, true,
    4, true>`; the gated twin carries GATE = true as one more argument (`attn_kv_kernel_o3_live` for the o3 tile kernel)"""
    _, family, targs, gated = form[:4]
    name, bools = KERNELS[family]
    args = [("true" if v else "false") if i in bools else str(v) for i, v in enumerate(targs)]
    if gated and family == KV_TILE_O3:
        name += "_live"
    elif gated:
        args.append("true")
    return "%s<%s>" % (name, ", ".join(args)) if args else name


def from_library(ints, apply):
    """pcr_attn_launch_form's ints -> a _form"""
    n = ints[3]
    return (ints[0], ints[1], tuple(ints[4:4 + n]), ints[2], 0 if apply else ints[10], 0 if apply else ints[11])
