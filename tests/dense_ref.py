"""The per-point dense launches (csrc/model_kernels.hip) and the EdgeConv / local-attention launches (csrc/edge_kernels.hip)
in float64 -- and the shape rules of their dispatchers (dense_launch, dense_bf_launch, pcr_dense_xpm_prec_f32,
pcr_dense_max_f32, pcr_edge_max_f32, pcr_local_attn_f32, with the Python side of the choice: engine.dense, rows.dense_gn)
restated as pure functions, so that a test can say which kernel instantiation a shape reaches without running it.
`dense_emul` is the same operation with the operands as the bf16 units see them (hi / lo split, round to nearest even),
everything after the split in float64: a correct bf16 kernel differs from it by its float32 accumulation only.
tests/test_dense_ref_cpu.py holds all of it to a second formulation, to planted faults and to the library's exported shape
queries; tests/test_gpu_dense_forms.py holds every launch form to `dense_ref` and `dense_emul`.  No import of the library."""
import zlib

import torch

F64 = torch.float64
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2}
UNIT = ("f32", "bf16x3", "bf16")
GN_EPS = 1e-5


# ---- the operations ----------------------------------------------------------------------------------------------------
def _activate(y, act, slope=0.2):
    return torch.relu(y) if act == 1 else (torch.where(y < 0, y * slope, y) if act == 2 else y)


def _affine(pre, scale, shift, act, slope=0.2):
    dt = pre.dtype
    if scale is not None:
        pre = pre * scale.to(dt).view(1, -1, 1)
    if shift is not None:
        pre = pre + shift.to(dt).view(1, -1, 1)
    return _activate(pre, act, slope)


def product(x, w, x_pm=False, dtype=F64):
    """W x per token: x (B,cin,L) (or (B,L,cin) when x_pm), w (cout,cin) or per cloud (B,cout,cin) -> (B,cout,L)"""
    x = x.to(dtype)
    if x_pm:
        x = x.transpose(1, 2)
    return torch.matmul(w.to(dtype), x)


def dense_ref(x, w, scale=None, shift=None, act=0, x_pm=False):
    """act(scale (W x) + shift), act 0 / 1 / 2 = none / ReLU / leaky 0.2: (B,cout,L) float64"""
    return _affine(product(x, w, x_pm), scale, shift, act)


def groupnorm_ref(y, gamma, beta, groups, res=None, relu=False, eps=GN_EPS, band_shift=0, res_first=False):
    """GroupNorm per token over `groups` groups of consecutive channels of y (B,C,L): biased variance, eps 1e-5, then
    + res, then ReLU.  band_shift / res_first / eps: planted faults only (the groups start band_shift channels late and
    wrap; the residual goes in ahead of the normalisation)"""
    dt = y.dtype if y.dtype in (F64, torch.float32) else F64
    y = y.to(dt)
    B, C, L = y.shape
    if res_first and res is not None:
        y = y + res.to(dt)
    if band_shift:
        y = y.roll(-band_shift, dims=1)
    g = y.reshape(B, groups, C // groups, L)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    out = ((g - mean) / torch.sqrt(var + eps)).reshape(B, C, L)
    if band_shift:
        out = out.roll(band_shift, dims=1)
    out = out * gamma.to(dt).view(1, -1, 1) + beta.to(dt).view(1, -1, 1)
    if res is not None and not res_first:
        out = out + res.to(dt)
    return torch.relu(out) if relu else out


def dense_gn_ref(x, w, gamma, beta, groups, res=None, relu=False, **fault):
    return groupnorm_ref(product(x, w), gamma, beta, groups, res, relu, **fault)


def dense_max_ref(x, w, scale, shift, act):
    """the layer's maximum over the tokens, written out[c * B + b]: (cout, B) float64"""
    return dense_ref(x, w, scale, shift, act).max(dim=2)[0].t().contiguous()


def bmm_ref(x, t):
    """PointNet's learned transform: y_b = (x_b^T T_b)^T for t (B,k,k) -- per-cloud weights W_b = T_b^T"""
    return product(x, t.transpose(1, 2))


def bmm_table(t):
    """t (B,k,k) as the STN's fc3 output hands it to pcr_pack_bmm_f32: (1, k*k, B), entry [c*k + c2][b] = T_b[c][c2]"""
    B, k, _ = t.shape
    return t.reshape(B, k * k).t().contiguous().view(1, k * k, B)


def edge_max_ref(ta, tb, idx, shift, slope=0.2, dtype=F64, drop_last=False):
    """out[b][c][i] = leaky(max_j ta[b][idx[b][i][j]][c] + tb[b][i][c] + shift[c]); ta, tb (B,N,Co) point-major, idx
    (B,N,K) -> (B,Co,N).  In float32 the kernel's order -- (m + tb) + shift, then the slope -- is kept: a maximum and two
    ordered adds are exact to reproduce.  drop_last (planted fault): the last neighbour is ignored"""
    B, N, Co = ta.shape
    li = idx.long()
    if drop_last:
        li = li[:, :, :-1]
    K = li.shape[2]
    a = ta.to(dtype)
    nb = torch.gather(a, 1, li.reshape(B, N * K, 1).expand(-1, -1, Co)).view(B, N, K, Co)
    s = nb.max(dim=2)[0] + tb.to(dtype)
    y = s + shift.to(dtype).view(1, 1, Co)
    y = torch.where(y > 0, y, y * torch.tensor(slope, dtype=dtype))
    return y.transpose(1, 2).contiguous()


def local_attn_ref(qkv, idx, nhead, eps=1e-6, dtype=F64, drop_last=False, den_eps=True):
    """local_self_attention's message (oracle/model_oracle.py: linear_attention with ONE query token per point over its K
    neighbours): Q = elu(q_i) + 1, K_j = elu(k_j) + 1, msg_i = Q . sum_j K_j (x) v_j / (Q . sum_j K_j + eps) per head.
    qkv (B,N,3C) rows [q | k | v], idx (B,N,K) -> (B,C,N)"""
    B, N, C3 = qkv.shape
    C = C3 // 3
    dh = C // nhead
    li = idx.long()
    if drop_last:
        li = li[:, :, :-1]
    K = li.shape[2]
    r = qkv.to(dtype)
    elu1 = lambda t: torch.where(t > 0, t + 1, torch.exp(t))     # noqa: E731
    Q = elu1(r[:, :, :C]).view(B, N, 1, nhead, dh)
    rows = torch.gather(r, 1, li.reshape(B, N * K, 1).expand(-1, -1, C3)).view(B, N, K, C3)
    Kf = elu1(rows[..., C:2 * C]).view(B, N, K, nhead, dh)
    V = rows[..., 2 * C:].view(B, N, K, nhead, dh)
    a = (Q * Kf).sum(dim=-1, keepdim=True)                        # (B,N,K,nhead,1)
    den = a.sum(dim=2) + (eps if den_eps else 0.0)
    num = (a * V).sum(dim=2)
    return (num / den).reshape(B, N, C).transpose(1, 2).contiguous()


# ---- the bf16 units' arithmetic ------------------------------------------------------------------------------------------
def bf_split(v):
    """(hi, lo) as float32 tensors: hi = bf16(v), lo = bf16(v - hi), both round to nearest even (bf_split8, the packer)"""
    v = v.float()
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    return hi, lo


def product_emul(x, w, ns, x_pm=False, dtype=F64, drop_lo_step=None):
    """W x as the bf16 units form it: W_hi x_hi + W_hi x_lo + W_lo x_hi (ns = 3) or W_hi x_hi (ns = 1), the sums in
    `dtype`.  drop_lo_step (planted fault): the W_hi x_lo term of that 16-channel step is left out"""
    if x_pm:
        x = x.transpose(1, 2)
    xh, xl = bf_split(x)
    wh, wl = bf_split(w)
    m = lambda a, b: torch.matmul(a.to(dtype), b.to(dtype))       # noqa: E731
    if ns == 1:
        return m(wh, xh)
    if drop_lo_step is not None:
        xl = xl.clone()
        xl[:, 16 * drop_lo_step:16 * drop_lo_step + 16] = 0
    return m(wh, xh) + m(wh, xl) + m(wl, xh)


def dense_emul(x, w, scale=None, shift=None, act=0, ns=3, x_pm=False, dtype=F64, **fault):
    return _affine(product_emul(x, w, ns, x_pm, dtype, **fault), scale, shift, act)


def dense_gn_emul(x, w, gamma, beta, groups, res=None, relu=False, ns=3, dtype=F64):
    return groupnorm_ref(product_emul(x, w, ns, False, dtype), gamma, beta, groups, res, relu)


# ---- the dispatchers' shape rules ----------------------------------------------------------------------------------------
MAX_LDS = 160 * 1024         # kMaxDynLds
CHUNK = 256                  # kChunk
PC_T = 128                   # kPcT


def ceil8(x):
    return (x + 7) & ~7


def ceil32(x):
    return (x + 31) & ~31


def prec_ok(cin, cout, L):
    """pcr_dense_prec_ok"""
    return int(cin >= 64 and cin % 64 == 0 and cout >= 32 and cout % 32 == 0 and L >= 1)


def xpm_prec_ok(cin, cout, L):
    """pcr_dense_xpm_prec_ok: the weight image must fit LDS"""
    if not (cin >= 64 and cin % 64 == 0 and 1 <= cout <= 128 and L >= 1):
        return 0
    return int((cin // 16) * ((cout + 31) // 32) * 2048 + 1024 <= 144 * 1024)


def max_ok(cin, cout, L):
    """pcr_dense_max_ok"""
    return int(cin >= 1 and cout >= 256 and cout % 256 == 0 and L >= 1 and ceil8(cin) * 65 * 4 + 2048 <= 64 * 1024)


def rw_ok(cin, cout, L):
    return 16 <= cin <= 128 and cout >= 128 and L >= 128


def _rw(cin, maxe):
    KB = ceil8(cin) // 8
    return "f32 rw<%d,%s>" % (4 if KB <= 4 else (8 if KB <= 8 else 16), "max" if maxe else "store")


def _f32(B, cin, cout, L, x_pm, gn_gs, per_cloud):
    """dense_launch"""
    if B > 65535 or min(B, cin, cout, L) < 1:
        return "refused"
    gn = "gn" if gn_gs else "plain"
    if not per_cloud and not x_pm and not gn_gs and rw_ok(cin, cout, L):
        return _rw(cin, False)
    if cin >= 2 * CHUNK and cin % CHUNK == 0 and cout % 256 == 0 and not x_pm and not per_cloud and L > 32:
        return "f32 chunk<%s>" % gn
    cinP = ceil8(cin)
    tb = 2 if (cinP * 65 * 4 <= 72 * 1024 and L > 32) else 1
    if (cinP * (32 * tb + 1) + 512) * 4 > MAX_LDS:
        return "refused"
    return "f32 tile<%d,%s>" % (tb, gn)


def _bf(B, cin, cout, L, prec, gn_gs, aligned=True):
    """dense_bf_launch"""
    if not prec_ok(cin, cout, L) or B > 65535 or B < 1:
        return "refused"
    gn = "gn" if gn_gs else "plain"
    if cin in (256, 512, 1024) and L % PC_T == 0 and aligned and cout > 128 and cin * L * 4 < 0x7FFFFFFF:
        tiles, nzw = B * (L // PC_T), (ceil32(cout) + 255) // 256
        if ((tiles + 7) // 8) * 8 * nzw > 0x7FFFFFFF:
            return "refused"
        return "%s pc<%s,%d>" % (UNIT[prec], gn, cin // 128)
    KC = 256 if cin % 256 == 0 else (128 if cin % 128 == 0 else 64)
    return "%s bf<%s,NR%d,KC%d>" % (UNIT[prec], gn, 2 if cout > 128 else 1, KC)


def _pm(B, cin, cout, L, prec):
    """pcr_dense_xpm_prec_f32"""
    if not xpm_prec_ok(cin, cout, L) or B > 65535 or B < 1 or B * ((L + 31) // 32) >= 0x7FFFFFFF:
        return "refused"
    return "%s pm<%d>" % (UNIT[prec], (cout + 31) // 32)


def has_bf_image(cin, cout):
    """engine.pack_weight_dual attaches the bf16 image (`_pcr_bf`) only where one of the bf16 launches could take it"""
    return bool(prec_ok(cin, cout, 1) or xpm_prec_ok(cin, cout, 1))


def dispatch(entry, B, cin, cout, L, prec=0, x_pm=0, gn_gs=0):
    """the instantiation a call reaches, or "refused".  entry: "dense" = engine.dense, "gn" = rows.dense_gn (gn_gs: channels
    per group), "bmm" = pcr_dense_bmm_f32, "max" = pcr_dense_max_f32; "prec" / "xpm_prec" / "f32": pcr_dense_prec_f32 /
    pcr_dense_xpm_prec_f32 / pcr_dense_f32 called directly.  prec 0 / 1 / 2 is what was asked for; the name's first word
    is the unit that runs"""
    if entry == "f32":
        return _f32(B, cin, cout, L, x_pm, 0, False)
    if entry == "prec":
        return _bf(B, cin, cout, L, prec, 0)
    if entry == "xpm_prec":
        return _pm(B, cin, cout, L, prec)
    if entry == "bmm":
        return _f32(B, cin, cout, L, 0, 0, True)
    if entry == "max":
        if not max_ok(cin, cout, L) or B > 65535 or B < 1:
            return "refused"
        return _rw(cin, True) if rw_ok(cin, cout, L) else "f32 max<>"
    bf = prec != 0 and has_bf_image(cin, cout)
    if entry == "dense":
        if bf and not x_pm and prec_ok(cin, cout, L):
            return _bf(B, cin, cout, L, prec, 0)
        if bf and x_pm and xpm_prec_ok(cin, cout, L):
            return _pm(B, cin, cout, L, prec)
        return _f32(B, cin, cout, L, x_pm, 0, False)
    assert entry == "gn" and gn_gs >= 1 and cout % gn_gs == 0 and not x_pm
    if gn_gs not in (4, 8, 16, 32):
        d = dispatch("dense", B, cin, cout, L, prec, 0, 0)
        return d if d == "refused" else d + " + groupnorm"
    if bf and prec_ok(cin, cout, L):
        return _bf(B, cin, cout, L, prec, gn_gs)
    return _f32(B, cin, cout, L, 0, gn_gs, False)


def edge_dispatch(N, Co, K, B=1):
    """pcr_edge_max_f32"""
    if min(B, N, Co, K) < 1 or Co > 256 or K > 64 or B > 65535:
        return "refused"
    if N <= 512:
        return "edge lds<%d>" % (32 if N <= 128 else 16)
    return "edge gather"


def local_dispatch(N, C, K, nhead, B=1):
    """pcr_local_attn_f32"""
    if min(B, N, C, K, nhead) < 1 or C > 64 or C % nhead or B > 65535:
        return "refused"
    dh = C // nhead
    if dh & (dh - 1):
        return "refused"
    if dh == 32 and (N * 32 * 2 + 32 * 33 + 32 * K) * 4 <= 72 * 1024:
        return "local lds<32>"
    return "local<%d>" % (dh if dh in (16, 32) else 0)


def unit_of(name):
    """the arithmetic a named instantiation runs its matrix phase in (pcr_last_launch_arith)"""
    return PREC[name.split(" ")[0]]


def kernel_name(name):
    """an instantiation as a kernel trace spells it"""
    name = name.split(" + ")[0]
    if name.startswith("local"):
        return ("local_attn_lds_kernel<%s" if " lds" in name else "local_attn_kernel<%s") % name.split("<")[1]
    unit, rest = name.split(" ", 1)
    fam, _, args = rest.partition("<")
    a = args.rstrip(">").split(",") if args.rstrip(">") else []
    if unit == "edge":
        return "edge_max_kernel(" if fam == "gather" else "edge_max_lds_kernel<%s>" % a[0]
    gn = "true" if a and a[0] == "gn" else "false"
    ns = "3" if unit == "bf16x3" else "1"
    if fam == "rw":
        return "dense_rw_kernel<%s, %s>" % (a[0], "true" if a[1] == "max" else "false")
    if fam == "tile":
        return "dense_kernel<%s, %s, false>" % (a[0], "true" if a[1] == "gn" else "false")
    if fam == "chunk":
        return "dense_kernel<2, %s, true>" % gn
    if fam == "max":
        return "dense_max_kernel("
    if fam == "bf":
        return "dense_bf_kernel<%s, %s, %s>" % (gn, ns, a[1][2:])
    if fam == "pc":
        return "dense_bf_pc_kernel<%s, %s, %s>" % (gn, ns, a[1])
    assert fam == "pm", name
    return "dense_pm_stream_kernel<%s, %s>" % (a[0], "true" if unit == "bf16x3" else "false")


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def marked_tokens(L):
    """the tokens a max form must not lose: the first, the last, and one next to a 64-token tile boundary"""
    return sorted({0, L - 1, 63 if L > 63 else L // 2, 64 if L > 64 else L // 2})


def dense_inputs(entry, B, cin, cout, L, x_pm, act, groups, res):
    """dict of CPU float32 tensors for one dense row, seeded by the shape.  Weights of one scale over all of cin (every
    k-block carries comparable weight); pre-activation values straddle zero; affine: scale and shift with an activation,
    the shift alone or nothing without (L even / odd); max rows: the marked tokens are three times a typical token's length, so each
    owns channels' maxima; GN rows: token 1 of every cloud is scaled so that W x is about 3e-3 -- a variance of 1e-5, where eps
    decides -- and the residual is drawn apart from everything else"""
    g = _gen(entry, B, cin, cout, L, x_pm, act, groups, res)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    d = {"w": w}
    if entry == "bmm":
        d["t"] = torch.randn(B, cin, cout, generator=g) / cin ** 0.5
        d["w"] = d["t"].transpose(1, 2).contiguous()
    if entry == "max":
        for t in marked_tokens(L):          # (three times a typical token's length, each in a direction of its own)
            x[:, :, t] *= 3.0 * cin ** 0.5 / x[:, :, t].norm(dim=1, keepdim=True)
    if entry == "gn":
        # (channel 0 is a constant that the weights hand to the couts with alternating sign: no group of a token is then
        # nearly constant, where 1 / sqrt(var) would multiply the error of ANY arithmetic -- the float64 restatement of the
        # split operands included -- by ten and more; 4 752 groups of four N(0,1) values reach a variance of 0.005)
        x[:, 0, :] = (1 - 2 * (torch.arange(L) % 2)).float()       # (the sign by the token, so that no cout is cut by every ReLU)
        w[:, 0] = 4.0 * (1 - 2 * (torch.arange(cout) % 2)).float()
        x[:, :, min(1, L - 1)] *= 3e-3
        d["gamma"] = torch.rand(cout, generator=g) + 0.5
        d["beta"] = torch.randn(cout, generator=g) * 0.5
        d["res"] = torch.randn(B, cout, L, generator=g) if res else None
    elif entry != "bmm":
        kind = "both" if act else ("shift" if L % 2 == 0 else "none")
        d["scale"] = torch.rand(cout, generator=g) + 0.5 if kind == "both" else None
        d["shift"] = torch.randn(cout, generator=g) * 0.5 if kind != "none" else None
    d["x"] = x.transpose(1, 2).contiguous() if x_pm else x           # (B,L,cin) storage when point-major
    return d


def edge_inputs(B, N, Co, K):
    """ta, tb (B,N,Co), idx (B,N,K) with N - 1 among the indices, shift (Co): every point's FIRST neighbour owns the maximum
    of channel i % Co and its LAST neighbour that of channel (i + 1) % Co (K >= 2; with one channel the even points' first
    and the odd points' last neighbour own it)"""
    g = _gen("edge", B, N, Co, K)
    ta = torch.randn(B, N, Co, generator=g)
    tb = torch.randn(B, N, Co, generator=g)
    shift = torch.randn(Co, generator=g) * 0.5
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32)
    idx[:, 0, K - 1] = N - 1
    idx[:, N - 1, 0] = N - 1
    # reorder each point's list -- a maximum does not care -- so that the first / last neighbour owns a channel (a point
    # whose first neighbour owns both channels keeps its order)
    pts = torch.arange(N)
    for b in range(B):
        for which, ch in ((0, pts % Co), (K - 1, (pts + 1) % Co)):
            if K < 2 or (Co < 2 and which):
                continue
            nb = ta[b][idx[b].long()]                               # (N,K,Co)
            win = nb[pts, :, ch].argmax(dim=1)                      # (N,): position of the channel's maximum
            if which:
                win = torch.where(win == 0, torch.full_like(win, K - 1), win)
            to = torch.full_like(win, which)
            if Co < 2:                                              # (one channel: the odd points' LAST neighbour owns it)
                to = torch.where(pts % 2 == 1, torch.full_like(win, K - 1), to)
            a, c = idx[b, pts, win].clone(), idx[b, pts, to].clone()
            idx[b, pts, win], idx[b, pts, to] = c, a
    # the values straddle zero ahead of the slope: the shift takes out what a maximum over K draws adds on average
    nb = ta[torch.arange(B).view(B, 1, 1), idx.long()]                  # (B,N,K,Co)
    shift = shift - (nb.amax(dim=2) + tb).mean(dim=(0, 1))
    return ta, tb, idx.contiguous(), shift.contiguous()


def local_inputs(B, N, C, K):
    """qkv (B,N,3C), idx (B,N,K) with N - 1 among the indices.  Point 2 of every cloud has q = -16 throughout, so that
    its Q = exp(q) is 1e-7 and its denominator is of the order of eps = 1e-6: there eps decides"""
    g = _gen("local", B, N, C, K)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    qkv[:, min(2, N - 1), :C] = -16.0
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32)
    idx[:, 0, K - 1] = N - 1
    return qkv, idx.contiguous()


# ---- a row of tests/test_gpu_dense_forms.py --------------------------------------------------------------------------------
def dense_row_eval(row, d, kind="ref", **fault):
    """a dense row's result from its inputs `d` (dense_inputs).  kind: "ref" float64 restatement; "y32" the same in torch
    float32; "emul" / "emul32": the unit's emulated arithmetic, sums in float64 / float32.  The unit is the one the row's
    instantiation names.  (B,cout,L), or (cout,B) for a max row"""
    entry, prec, B, cin, cout, L, x_pm, act, groups, res, name = row
    ns = {0: 0, 1: 3, 2: 1}[unit_of(name)]
    dtype = torch.float32 if kind in ("y32", "emul32") else F64
    lo = {k: fault.pop(k) for k in ("drop_lo_step",) if k in fault}
    if kind in ("emul", "emul32"):
        assert ns, "an f32 row has no emulated arithmetic"
        pre = product_emul(d["x"], d["w"], ns, bool(x_pm), dtype, **lo)
    else:
        pre = product(d["x"], d["w"], bool(x_pm), dtype)
    if "drop_k" in fault:           # planted fault: the channels from drop_k on are left out of the contraction
        k0 = fault.pop("drop_k")
        x = d["x"].transpose(1, 2) if x_pm else d["x"]
        pre = pre - torch.matmul(d["w"].to(dtype)[..., k0:], x.to(dtype)[:, k0:])
    if entry == "gn":
        return groupnorm_ref(pre, d["gamma"], d["beta"], groups, d["res"], bool(act), **fault)
    if entry == "bmm":
        return pre
    out = _affine(pre, d["scale"], d["shift"], act, **fault)
    return out.max(dim=2)[0].t().contiguous() if entry == "max" else out


def rel_err(got, want):
    return float((got.double() - want.double()).abs().max()) / float(want.double().abs().max())
