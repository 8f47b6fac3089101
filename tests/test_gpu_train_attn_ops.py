"""GPU: the Point-Transformer training ops (pcr_amd.train_ops: the linear-attention core in its launch and Function forms,
TNorm, LocalAttn, PoolPair; csrc/train_attn_kernels.hip, csrc/train_local_kernels.hip) one by one against the float64
references of tests/train_attn_ref.py -- forward value, every gradient, every saved record (A, ks, mean, rstd, arg) -- at
the shapes where their kernels change plan, and bit-reproducibility of all of it (every case runs twice).

Bounds (`_rel` = max|a - b| / max|b|): selections, arg, maxima and routed copies exact; pooling means and their gradients
1e-6; linear attention, token norm and local attention, values and gradients, 2e-5 (the bounds test_gpu_train_ops.py
holds the same ops to).  The rows marked `yard` (head width 128, the stressed token norm) had never been measured on the
device: they are held to max(2e-5, 8 y32), y32 = the error of a float32 CPU evaluation of the same formula
(train_attn_ref on float32 tensors) against the float64 reference, tensor by tensor, computed here on the CPU -- never a
figure read off the kernel.  Quantities that are zero in exact arithmetic are held absolutely, against the scale of the
terms that cancel: dq and dk of the linear attention with one key and of the local attention with one distinct neighbour
(train_attn_ref), dx / dgamma of a one-channel group (the kernel's go gamma - go gamma is a fused multiply-add against a
rounded product: a rounding of the term times rstd = eps^-1/2, not 0).  dk / dv of a point no neighbour list cites are
exactly 0.

The case tables are plain data, shared with test_train_attn_ref_cpu.py, which builds every input without a device, shows
each token-norm input conditioned to zero marginal decisions within the moved-share cap, and prints every yardstick."""
import functools
import json

import pytest
import torch

import train_attn_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
ATTN_EPS = 1e-6            # LinearAttention's eps
NORM_EPS = 1e-5            # nn.LayerNorm / nn.GroupNorm default
BOUND = 2e-5
MEAN_BOUND = 1e-6
YARD = 8.0                 # margin on a float32-CPU yardstick (test_gpu_dense_forms.py)
MOVED_CAP = 0.005          # conditioning may move at most this share of a tensor
SENTINEL = 98765.0

# ---------------------------------------------------------------------------------------------- cases --
# LinAttn (B, d, H, Lq, Sk).  MFMA forms (dh = 32: one 32 x 32 tile of A, wave 0 only; dh = 64: four tiles, one per wave),
# 64-token chunks: a chunk of nl <= 32 tokens runs KT = 32 and skips its second n-tile, 33 .. 64 run KT = 64 over zero
# padding; 65 = a full chunk + a tail of 1, 97 = + a tail of 33, 130 = two full chunks + a tail of 2.
_MFMA_LS = [(1, 1),        # one query, one key: KT = 32 both passes, dq = 0 in exact arithmetic at eps = 0
            (32, 2),       # nl = 32: the last size that skips the second n-tile; tail of 2 keys
            (33, 31),      # nl = 33: the first size with KT = 64; ns = 31 < 32
            (64, 32),      # one full query chunk; ns = 32: KT = 32 exactly full
            (65, 33),      # full chunk + 1-token tail (KT 64 then 32: stale second-tile columns); ns = 33: KT = 64
            (130, 64),     # two full chunks + tail of 2; one full key chunk
            (1, 65),       # key chunk + 1-key tail (second chunk KT = 32)
            (32, 97),      # key chunk + 33-key tail (second chunk KT = 64)
            (33, 1),       # one key under 33 queries: dq = 0 again, KT = 64 in pass 1
            (64, 33),
            (65, 65),      # both tails of 1
            (130, 97)]     # both multi-chunk with tails 2 and 33
LIN_CASES = [(2, 64, 2, lq, sk) for lq, sk in _MFMA_LS]                     # linattn_*_mfma_kernel<32>
LIN_CASES += [(2, 128, 2, lq, sk) for lq, sk in _MFMA_LS]                   # linattn_*_mfma_kernel<64>
LIN_CASES += [(2, 32, 2, 65, 33),      # linattn_*_kernel<16, 64> (scalar, 64-token chunks): chunk + tail of 1, 33 keys
              (3, 16, 1, 1, 2),        # <16, 64>: one head, one query, two keys, three clouds
              (2, 32, 2, 64, 64)]      # <16, 64>: exactly one full chunk each way
LIN_CASES += [(2, 256, 2, 1, 17),      # linattn_*_kernel<128, 16> (scalar, 16-token chunks, ~156 KiB LDS in the backward)
              (2, 256, 2, 15, 33),     # <128, 16>: 15 < chunk; two key chunks + tail of 1
              (2, 256, 2, 16, 16),     # <128, 16>: exactly one chunk each way
              (2, 256, 2, 17, 1),      # <128, 16>: chunk + tail of 1; one key
              (2, 256, 2, 33, 15),     # <128, 16>: two chunks + tail of 1
              (1, 128, 1, 1, 1),       # <128, 16> with H = 1: one query, one key
              (2, 128, 1, 16, 33),
              (2, 128, 1, 17, 16),
              (1, 128, 1, 33, 17),
              (2, 128, 1, 15, 15)]
# kv_roll (B = 3, both signs, Lq = Sk so that the fused qkv form applies): one row per kernel form
ROLL_CASES = [(3, 64, 2, 33, 33), (3, 128, 2, 65, 65), (3, 32, 2, 17, 17), (3, 128, 1, 17, 17)]


def lin_yard(case):
    """head width 128 was never measured on the device: max(BOUND, YARD y32)"""
    return case[1] // case[2] == 128


# TNorm (B, C, L, G, res, relu, stress).  Plans (pcr_tnorm_*_f32): a group of 32 / 64 / 128 / 256 channels runs the
# four-wave kernel tnorm_*4_kernel<NC = 8 / 16 / 32 / 64>, every other group size the generic one-thread-per-token kernel.
# A block is 64 flat tokens b L + t: B L = 63 / 64 / 65 are one partial block, one full, one full + 1 token.
TN_CASES = [
    (1, 32, 63, 1, False, False, False),    # tnorm_*4_kernel<8>; B L = 63
    (2, 64, 32, 2, True, True, False),      # <8> with G = 2 (four-wave, G > 1); B L = 64
    (1, 64, 65, 1, True, False, False),     # <16>; B L = 65
    (5, 64, 13, 1, False, True, False),     # <16>; B L = 65 over five clouds
    (3, 128, 50, 1, False, False, False),   # <32>; a wave straddles two clouds, last block partial (150 = 2 x 64 + 22)
    (3, 128, 50, 1, True, False, False),    # <32>; res x relu, the other three
    (3, 128, 50, 1, False, True, False),
    (3, 128, 50, 1, True, True, False),
    (1, 256, 64, 1, True, True, False),     # <64>; B L = 64
    (70, 256, 1, 1, False, False, False),   # <64>; L = 1, every token its own cloud
    (1, 96, 63, 6, False, True, False),     # generic, group of 16 (divisible by 4, NC = 4 not instantiated)
    (3, 36, 50, 1, False, False, False),    # generic, group of 36 (divisible by 4, NC = 9 not instantiated); straddle
    (3, 36, 50, 1, True, False, False),     # generic; res x relu, the other three
    (3, 36, 50, 1, False, True, False),
    (3, 36, 50, 1, True, True, False),
    (5, 12, 13, 2, True, True, False),      # generic, group of 6 (not divisible by 4); B L = 65
    (70, 12, 1, 2, False, False, False),    # generic, group of 6; L = 1
    (70, 4, 1, 4, True, True, False),       # generic, group of ONE: rstd = eps^-1/2, z = beta + res, dx = dgamma = 0
    (2, 4, 32, 4, False, False, False),     # generic, group of one, no residual, no ReLU
    (1, 32, 65, 1, True, True, True),       # stressed (token mean = 10 sigma), one per plan: <8>
    (3, 64, 50, 1, False, True, True),      # stressed <16>
    (1, 128, 63, 1, True, False, True),     # stressed <32>
    (2, 256, 32, 1, False, True, True),     # stressed <64>
    (3, 72, 50, 2, True, True, True),       # stressed generic (group of 36)
]

# LocalAttn (B, C, N, K, H) x neighbour variant.  One wave per point, lane = channel: C = 64 has no dead lane, C = 48 / 32 /
# 8 do; four points per workgroup, so N = 9 / 33 / 50 leave a partial last workgroup; dh = 32, 16, 1, 8, 32.
LA_SHAPES = [(2, 64, 9, 4, 2), (2, 48, 33, 33, 3), (1, 8, 5, 1, 8), (2, 32, 50, 7, 4), (3, 64, 128, 48, 2)]
# perm: K distinct random neighbours; repeat: the second entry of every row repeats the first (K >= 2); self: every row
# is its own point K times; hub: every row cites points 0 .. K-1, so the points K .. N-1 are cited by nobody
LA_CASES = [(s, v) for s in LA_SHAPES for v in ("perm", "repeat", "self", "hub") if not (v == "repeat" and s[3] < 2)]
LA_EDGE_CASE = ((2, 32, 50, 7, 4), "repeat")          # the per-edge buffer itself against the reference's terms

# PoolPair (P, C, L): a wave per channel strides the 2 L positions by 64 -- 2 L < 64 (L = 1, 31) leaves idle lanes, L = 32
# fills the wave once, 33 .. 300 stride; four waves share the channels (C = 1, 5: idle / uneven waves).  Every (p, c) row
# plants one tie pattern (make_pool_input).
PP_CASES = [(5 if C == 1 else 2, C, Ln) for C in (1, 5, 64) for Ln in (1, 31, 32, 33, 64, 65, 300)]


# --------------------------------------------------------------------------------------------- inputs --
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def make_lin_input(case):
    """float32 CPU tensors of one LinAttn case: q (B,d,Lq), k, v (B,d,Sk), go (B,d,Lq)"""
    B, d, H, Lq, Sk = case
    g = _gen(*case)
    return dict(q=torch.randn(B, d, Lq, generator=g), k=torch.randn(B, d, Sk, generator=g),
                v=torch.randn(B, d, Sk, generator=g), go=torch.randn(B, d, Lq, generator=g))


@functools.lru_cache(maxsize=None)
def lin_want(case, kv_roll=0):
    """the float64 reference of one case, computed once: dict(out, A, ks, dq, dk, dv, scale = the maximum of the larger
    of the two cancelling terms of dq and of dk) plus y32 = dict of the float32 evaluation's errors when the case is held to
    a yardstick"""
    B, d, H, Lq, Sk = case
    inp = make_lin_input(case)
    q, k, v, go = (inp[n].to(F64) for n in ("q", "k", "v", "go"))
    out, A, ks = R.linattn_ref(q, k, v, H, ATTN_EPS, kv_roll)
    dq, dk, dv, (t1, t2), (u1, u2) = R.linattn_bwd_ref(q, k, v, H, ATTN_EPS, go, kv_roll)
    want = dict(out=out, A=A, ks=ks, dq=dq, dk=dk, dv=dv,
                scale=dict(dq=max(float(t1.abs().max()), float(t2.abs().max())),
                           dk=max(float(u1.abs().max()), float(u2.abs().max()))))
    if lin_yard(case):
        o32, A32, ks32 = R.linattn_ref(inp["q"], inp["k"], inp["v"], H, ATTN_EPS, kv_roll)
        g32 = R.linattn_bwd_ref(inp["q"], inp["k"], inp["v"], H, ATTN_EPS, inp["go"], kv_roll)
        want["y32"] = {n: _rel(a.to(F64), want[n]) for n, a in zip(("out", "A", "ks", "dq", "dk", "dv"),
                                                                   (o32, A32, ks32) + tuple(g32[:3]))}
        if Sk == 1:        # (dq and dk are cancellations: their yardsticks are on the scale of the terms too)
            want["y32"]["dq"] = float((g32[0].to(F64) - dq).abs().max()) / want["scale"]["dq"]
            want["y32"]["dk"] = float((g32[1].to(F64) - dk).abs().max()) / want["scale"]["dk"]
    return want


def lin_bound(case, want, name):
    """project bound, or the larger of it and YARD x the float32-CPU yardstick of this tensor"""
    return max(BOUND, YARD * want["y32"][name]) if "y32" in want else BOUND


def _affine(C, g):
    """gamma = 1 + 0.3 N(0,1) with channel 0 negative and channel 1 exactly zero (z = beta there, kept clear of zero);
    beta = 0.1 N(0,1) -- test_gpu_train_pointwise_ops._affine"""
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    gamma[0] = -gamma[0].abs() - 0.1
    gamma[1] = 0.0
    beta[1] = -0.25
    return gamma, beta


@functools.lru_cache(maxsize=None)
def make_tn_input(case):
    """float32 CPU tensors of one TNorm case: x (conditioned when there is a ReLU), gamma, beta, res | None, go, and the
    number of elements conditioning moved"""
    B, C, Ln, G, res, relu, stress = case
    g = _gen(*case)
    x = torch.randn(B, C, Ln, generator=g) * (0.5 + torch.rand(1, C, 1, generator=g))
    if stress:      # every token 10 of its own standard deviations off zero, either way
        side = torch.where(torch.rand(B, 1, Ln, generator=g) < 0.5, -1.0, 1.0)
        x = x + 10.0 * x.std(dim=1, keepdim=True) * side
    gamma, beta = _affine(C, g)
    r = torch.randn(B, C, Ln, generator=g) if res else None
    moved = 0
    if relu:
        x, r, moved = R.condition_tnorm(x, gamma, beta, r, G, NORM_EPS)
    return dict(x=x, gamma=gamma, beta=beta, res=r, go=torch.randn(B, C, Ln, generator=g), moved=moved)


def _tn_eval(inp, case, dtype):
    B, C, Ln, G, res, relu, stress = case
    x, gamma, beta, go = (inp[n].to(dtype) for n in ("x", "gamma", "beta", "go"))
    r = inp["res"].to(dtype) if res else None
    y, mean, rstd, _ = R.tnorm_ref(x, gamma, beta, r, G, NORM_EPS, relu)
    dx, dgamma, dbeta, dres = R.tnorm_bwd_ref(x, gamma, beta, r, G, NORM_EPS, relu, go)
    out = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if res:
        out["dres"] = dres
    return out


@functools.lru_cache(maxsize=None)
def tn_want(case):
    """the float64 reference of one TNorm case (dict by tensor name), with y32 for the stressed rows"""
    inp = make_tn_input(case)
    want = _tn_eval(inp, case, F64)
    if case[6]:
        want["y32"] = {n: _rel(a.to(F64), want[n]) for n, a in _tn_eval(inp, case, torch.float32).items()}
    B, C, Ln, G, res, relu, stress = case
    if C == G:
        # a group of ONE channel: x - mean = 0, so dx = rstd (go gamma - go gamma) and dgamma = sum go (x - mean) rstd are
        # zero in exact arithmetic; the scale of what cancels stands in for max|dx|, max|dgamma|
        go = inp["go"].to(F64) * (want["y"] > 0) if relu else inp["go"].to(F64)
        rstd = want["rstd"].reshape(B, C, Ln)
        want["scale"] = dict(dx=float((rstd * go * inp["gamma"].to(F64).view(1, C, 1)).abs().max()),
                             dgamma=float((go * inp["x"].to(F64) * rstd).abs().sum(dim=(0, 2)).max()))
    return want


def tn_bound(want, name):
    return max(BOUND, YARD * want["y32"][name]) if "y32" in want else BOUND


@functools.lru_cache(maxsize=None)
def make_la_input(shape, variant):
    """float32 / int32 CPU tensors of one LocalAttn case: qkv (B,3C,N), idx (B,N,K), go (B,C,N)"""
    B, C, N, K, H = shape
    g = _gen(*shape, len(variant))
    qkv = torch.randn(B, 3 * C, N, generator=g)
    go = torch.randn(B, C, N, generator=g)
    if variant == "self":
        idx = torch.arange(N).view(1, N, 1).expand(B, N, K)
    elif variant == "hub":
        idx = torch.arange(K).view(1, 1, K).expand(B, N, K)
    else:
        idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(N)]) for _ in range(B)])
        if variant == "repeat":
            idx[:, :, 1] = idx[:, :, 0]
    return dict(qkv=qkv, idx=idx.to(torch.int32).contiguous(), go=go)


@functools.lru_cache(maxsize=None)
def la_want(shape, variant):
    inp = make_la_input(shape, variant)
    H = shape[4]
    qkv, go = inp["qkv"].to(F64), inp["go"].to(F64)
    dqkv, edge, scale = R.local_attn_bwd_ref(qkv, inp["idx"], H, ATTN_EPS, go)
    return dict(msg=R.local_attn_ref(qkv, inp["idx"], H, ATTN_EPS), dqkv=dqkv, edge=edge, scale=scale)


def la_one_neighbour(shape, variant):
    """every row lists ONE distinct neighbour (K = 1, `self`): msg_i = v_j a / (a + eps), so dq and dk are zero in exact
    arithmetic at eps = 0 and eps / (a + eps) of their cancelling terms otherwise: their ERROR is held absolutely, on the
    scale of those terms (train_attn_ref)"""
    idx = make_la_input(shape, variant)["idx"]
    return bool((idx == idx[:, :, :1]).all())


def la_uncited(shape, variant):
    """mask (B,N) of the points no neighbour list cites"""
    B, C, N, K, H = shape
    idx = make_la_input(shape, variant)["idx"].long()
    cited = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        cited[b, idx[b].reshape(-1)] = True
    return ~cited


@functools.lru_cache(maxsize=None)
def make_pool_input(case):
    """o (2P,C,L) float32 with one exact-tie pattern planted per (pair, channel) row, kind = row % 5 -- 0: as drawn; 1: the
    maximum in BOTH halves (the first half's position wins); 2: the maximum at L - 1 and at L (the last point of the first
    cloud and the first of the second); 3: a constant channel (arg = 0); 4: the maximum in the second half only, twice where
    L > 1 (its first position wins) -- and go (P,2C)"""
    P, C, Ln = case
    g = _gen(*case, 19)
    x = torch.randn(P * C, 2 * Ln, generator=g)
    kind = torch.arange(P * C) % 5
    top = x.abs().amax(dim=1) + 1.0
    a, b = Ln // 3, Ln + (2 * Ln) // 3          # one position in each half
    for r in range(P * C):
        if kind[r] == 1:
            x[r, a] = x[r, b] = top[r]
        elif kind[r] == 2:
            x[r, Ln - 1] = x[r, Ln] = top[r]
        elif kind[r] == 3:
            x[r] = float(x[r, 0])
        elif kind[r] == 4:
            x[r, b] = x[r, 2 * Ln - 1] = top[r]
    x = x.reshape(P, C, 2 * Ln)
    o = torch.cat([x[:, :, :Ln], x[:, :, Ln:]], dim=0).contiguous()
    return dict(o=o, go=torch.randn(P, 2 * C, generator=g), kind=kind.reshape(P, C), a=a, b=b)


def pool_planted_arg(case):
    """the argument every planted row must select, -1 where the row is as drawn"""
    P, C, Ln = case
    inp = make_pool_input(case)
    want = torch.full((P, C), -1, dtype=torch.long)
    want[inp["kind"] == 1] = inp["a"]
    want[inp["kind"] == 2] = Ln - 1
    want[inp["kind"] == 3] = 0
    want[inp["kind"] == 4] = inp["b"]
    return want


# -------------------------------------------------------------------------------------------- helpers --
def _rel(a, b):
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def _vs(got, want):
    """_rel of a device float32 tensor against its float64 reference"""
    return _rel(got.detach().cpu().to(F64), want.detach())


def _report(op, case, worst, bound=None):
    print(json.dumps(dict(op=op, case=str(case), worst=worst, bound=bound)))


def _same(run_a, run_b):
    for a, b in zip(run_a, run_b):
        assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------- LinAttn --
_ROWS = lambda d: ((1, 1 + d), (2 + d, 2 + 2 * d), (3 + 2 * d, 3 + 3 * d))     # noqa: E731  [s q s k s v s]: 3 d + 4 rows


def _guarded(B, d, Lq, Sk, blocks=None):
    """(buffers, [q, k, v] channel slices): (B, 3 d + 4, L) buffers full of SENTINEL with the three blocks (None: left as
    sentinel, to be written by a launch) at rows [s q s k s v s]; one buffer when Lq = Sk, else one of each length, the
    q block in the first and the k / v blocks in the second"""
    bufs = [torch.full((B, 3 * d + 4, Ln), SENTINEL) for Ln in ((Lq,) if Lq == Sk else (Lq, Sk))]
    if blocks is not None:
        for buf, (lo, hi), blk in zip((bufs[0], bufs[-1], bufs[-1]), _ROWS(d), blocks):
            buf[:, lo:hi] = blk
    bufs = [b.cuda() for b in bufs]
    return bufs, [buf[:, lo:hi] for buf, (lo, hi) in zip((bufs[0], bufs[-1], bufs[-1]), _ROWS(d))]


def _guards_intact(bufs, d, Lq, Sk):
    """everything outside the blocks a launch may write still holds the sentinel"""
    for n, buf in enumerate(bufs):
        keep = torch.ones(buf.shape[1], dtype=torch.bool)
        for i, (lo, hi) in enumerate(_ROWS(d)):
            if len(bufs) == 1 or (i == 0) == (n == 0):
                keep[lo:hi] = False
        assert int(keep.sum()) >= 4
        assert bool((buf.cpu()[:, keep] == SENTINEL).all())


def _lin_launch(case, kv_roll, records=None):
    """one forward + backward through train_ops._linattn_fwd / _linattn_bwd on guarded buffers -> [out, A, ks, dq, dk, dv];
    records = (A, ks): the backward reads THESE (the forward is not launched: out, A, ks are returned as given)"""
    from pcr_amd import train_ops as TO
    B, d, H, Lq, Sk = case
    inp = make_lin_input(case)
    src, (q, k, v) = _guarded(B, d, Lq, Sk, (inp["q"], inp["k"], inp["v"]))
    before = [s.clone() for s in src]
    if records is None:
        out, A, ks = TO._linattn_fwd(q, k, v, H, ATTN_EPS, kv_roll)
    else:
        out, (A, ks) = None, records
    dst, (dq, dk, dv) = _guarded(B, d, Lq, Sk)
    TO._linattn_bwd(q, k, v, A, ks, inp["go"].cuda(), dq, dk, dv, H, ATTN_EPS, kv_roll)
    torch.cuda.synchronize()
    _same(src, before)                                    # the operand buffers, spare rows included, are only read
    _guards_intact(dst, d, Lq, Sk)
    return [t if t is None else t.clone() for t in (out, A, ks, dq, dk, dv)]


def _lin_check(case, got, want, names, tag):
    """every named tensor within its bound; dq and dk with ONE key absolutely (max|dq| and max|dq - reference| against the
    larger of the two cancelling terms the reference returns): both are zero in exact arithmetic at eps = 0"""
    B, d, H, Lq, Sk = case
    worst, bounds = {}, {}
    for n in names:
        bounds[n] = lin_bound(case, want, n)
        if n in ("dq", "dk") and Sk == 1:
            ours = got[n].cpu().to(F64)
            worst[n] = max(float(ours.abs().max()), float((ours - want[n]).abs().max())) / want["scale"][n]
        else:
            worst[n] = _vs(got[n], want[n])
    _report(tag, case, worst, bounds)
    for n in names:
        assert worst[n] < bounds[n], (tag, case, n, worst[n], bounds[n])


_LIN_NAMES = ("out", "A", "ks", "dq", "dk", "dv")


@pytest.mark.parametrize("case", LIN_CASES)
def test_linattn_launches_match_float64(case):
    want = lin_want(case)
    runs = [_lin_launch(case, 0) for _ in range(2)]
    _same(*runs)
    _lin_check(case, dict(zip(_LIN_NAMES, runs[0])), want, _LIN_NAMES, "linattn")


@pytest.mark.parametrize("case", LIN_CASES)
def test_linattn_backward_on_given_records(case):
    """A and ks are the float64 reference's, rounded once: the backward launch alone, without the forward's error"""
    want = lin_want(case)
    rec = (want["A"].to(torch.float32).cuda(), want["ks"].to(torch.float32).cuda())
    runs = [_lin_launch(case, 0, rec)[3:] for _ in range(2)]
    _same(*runs)
    _lin_check(case, dict(zip(_LIN_NAMES[3:], runs[0])), want, _LIN_NAMES[3:], "linattn given")


def _fn_run(fn, leaves, go):
    out = fn(*leaves)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, go))


@pytest.mark.parametrize("case", LIN_CASES)
def test_linattn_functions_match_float64_and_each_other(case):
    """LinAttn on separate tensors against float64; LinAttnKV (k | v one tensor) and, where Lq = Sk, LinAttnQKV (one fused
    projection) bit-equal to it"""
    from pcr_amd import train_ops as TO
    B, d, H, Lq, Sk = case
    inp, want = make_lin_input(case), lin_want(case)
    go = inp["go"].cuda()
    leaf = lambda t: t.cuda().requires_grad_(True)     # noqa: E731
    runs = [_fn_run(lambda q, k, v: TO.LinAttn.apply(q, k, v, H, ATTN_EPS), [leaf(inp[n]) for n in "qkv"], go)
            for _ in range(2)]
    _same(*runs)
    _lin_check(case, dict(zip(("out", "dq", "dk", "dv"), runs[0])), want, ("out", "dq", "dk", "dv"), "LinAttn")
    out, dq, dk, dv = runs[0]
    kv = _fn_run(lambda q, t: TO.LinAttnKV.apply(q, t, H, ATTN_EPS),
                 [leaf(inp["q"]), leaf(torch.cat([inp["k"], inp["v"]], 1))], go)
    _same(kv, [out, dq, torch.cat([dk, dv], dim=1)])
    if Lq == Sk:
        one = _fn_run(lambda t: TO.LinAttnQKV.apply(t, H, ATTN_EPS), [leaf(torch.cat([inp["q"], inp["k"], inp["v"]], 1))], go)
        _same(one, [out, torch.cat([dq, dk, dv], dim=1)])


# eps = 0: a padding token of a partial chunk has Q' = 0, so 1 / (Q'.ks + eps) = 1 / 0 there; one case per kernel form with
# a partial query chunk (the MFMA forms also with a full chunk before a 16-token tail)
EPS0_CASES = [(2, 64, 2, 33, 33), (2, 64, 2, 80, 80), (2, 128, 2, 33, 33), (2, 128, 2, 80, 80), (2, 32, 2, 65, 33),
              (2, 256, 2, 17, 17)]


@pytest.mark.parametrize("case", EPS0_CASES)
def test_linattn_at_eps_zero_is_finite_and_matches_float64(case):
    """the padding tokens are inert: no inf 0 reaches dq, dk or dv"""
    from pcr_amd import train_ops as TO
    B, d, H, Lq, Sk = case
    inp = make_lin_input(case)
    q, k, v, go = (inp[n].to(F64) for n in ("q", "k", "v", "go"))
    want = dict(zip(("out", "dq", "dk", "dv"), (R.linattn_ref(q, k, v, H, 0.0)[0],) + R.linattn_bwd_ref(q, k, v, H, 0.0, go)[:3]))
    f32 = (R.linattn_ref(inp["q"], inp["k"], inp["v"], H, 0.0)[0],) + R.linattn_bwd_ref(inp["q"], inp["k"], inp["v"], H, 0.0,
                                                                                     inp["go"])[:3]
    bounds = {n: max(BOUND, YARD * _rel(a.to(F64), want[n])) for n, a in zip(want, f32)}
    got = _fn_run(lambda a, b, c: TO.LinAttn.apply(a, b, c, H, 0.0), [inp[n].cuda().requires_grad_(True) for n in "qkv"],
                  inp["go"].cuda())
    worst = {n: _vs(t, want[n]) for n, t in zip(want, got)}
    _report("LinAttn eps 0", case, worst, bounds)
    for n, t in zip(want, got):
        assert bool(torch.isfinite(t).all()), (case, n)
        assert worst[n] < bounds[n], (case, n, worst[n], bounds[n])


@pytest.mark.parametrize("kv_roll", [1, -1])
@pytest.mark.parametrize("case", ROLL_CASES)
def test_linattn_kv_roll_matches_float64(case, kv_roll):
    """query cloud b against cloud (b + kv_roll) mod 3: the launches on guarded buffers and LinAttnQKV, both against the
    float64 reference of the rolled problem (dk / dv land on the clouds they were read from)"""
    from pcr_amd import train_ops as TO
    B, d, H, Lq, Sk = case
    inp, want = make_lin_input(case), lin_want(case, kv_roll)
    assert not torch.equal(want["out"], lin_want(case)["out"])
    runs = [_lin_launch(case, kv_roll) for _ in range(2)]
    _same(*runs)
    _lin_check(case, dict(zip(_LIN_NAMES, runs[0])), want, _LIN_NAMES, "linattn roll %d" % kv_roll)
    qkv = torch.cat([inp["q"], inp["k"], inp["v"]], dim=1).cuda().requires_grad_(True)
    one = _fn_run(lambda t: TO.LinAttnQKV.apply(t, H, ATTN_EPS, kv_roll), [qkv], inp["go"].cuda())
    _same(one, [runs[0][0], torch.cat(runs[0][3:], dim=1)])


# ---------------------------------------------------------------------------------------------- TNorm --
def _tn_run(case):
    from pcr_amd import train_ops as TO
    B, C, Ln, G, res, relu, stress = case
    inp = make_tn_input(case)
    leaves = [inp[n].cuda().requires_grad_(True) for n in ("x", "gamma", "beta") + (("res",) if res else ())]
    y = TO.TNorm.apply(leaves[0], leaves[1], leaves[2], leaves[3] if res else None, G, NORM_EPS, relu)
    mean, rstd = y.grad_fn.saved_tensors[2:4]
    assert tuple(mean.shape) == tuple(rstd.shape) == (B, G, Ln)
    grads = torch.autograd.grad(y, leaves, inp["go"].cuda())
    names = ["y", "mean", "rstd", "dx", "dgamma", "dbeta"] + (["dres"] if res else [])
    return dict(zip(names, [y.detach(), mean.clone(), rstd.clone()] + list(grads)))


@pytest.mark.parametrize("case", TN_CASES)
def test_tnorm_matches_float64(case):
    B, C, Ln, G, res, relu, stress = case
    inp, want = make_tn_input(case), tn_want(case)
    if relu:
        assert R.tnorm_marginals(inp["x"], inp["gamma"], inp["beta"], inp["res"], G, NORM_EPS) == 0
        assert inp["moved"] <= MOVED_CAP * inp["x"].numel()
    runs = [_tn_run(case) for _ in range(2)]
    _same(runs[0].values(), runs[1].values())
    got = runs[0]
    worst, bounds = {}, {}
    for n in got:
        bounds[n] = tn_bound(want, n)
        if C == G and n in ("dx", "dgamma"):
            # a group of one channel: both are zero in exact arithmetic (and exactly in the reference): held absolutely
            assert float(want[n].abs().max()) == 0.0
            worst[n] = float(got[n].abs().max()) / want["scale"][n]
            continue
        worst[n] = _vs(got[n], want[n])
    _report("tnorm", case, worst, bounds)
    for n in worst:
        assert worst[n] < bounds[n], (case, n, worst[n], bounds[n])
    if relu:
        assert torch.equal(got["y"].cpu() > 0, want["y"] > 0)            # no decision differs from the reference's


# ------------------------------------------------------------------------------------------ LocalAttn --
def _la_run(shape, variant):
    from pcr_amd import train_ops as TO
    inp = make_la_input(shape, variant)
    qkv = inp["qkv"].cuda().requires_grad_(True)
    msg = TO.LocalAttn.apply(qkv, inp["idx"].cuda(), shape[4], ATTN_EPS)
    return [msg.detach(), torch.autograd.grad(msg, qkv, inp["go"].cuda())[0]]


@pytest.mark.parametrize("shape,variant", LA_CASES)
def test_local_attn_matches_float64(shape, variant):
    B, C, N, K, H = shape
    want = la_want(shape, variant)
    runs = [_la_run(shape, variant) for _ in range(2)]
    _same(*runs)
    msg, dqkv = runs[0]
    worst = dict(msg=_vs(msg, want["msg"]), dq=_vs(dqkv[:, :C], want["dqkv"][:, :C]),
                 dk=_vs(dqkv[:, C:2 * C], want["dqkv"][:, C:2 * C]), dv=_vs(dqkv[:, 2 * C:], want["dqkv"][:, 2 * C:]))
    if la_one_neighbour(shape, variant):
        for n, rows in (("dq", slice(0, C)), ("dk", slice(C, 2 * C))):
            ours, ref = dqkv[:, rows].cpu().to(F64), want["dqkv"][:, rows]
            worst[n] = float((ours - ref).abs().max()) / want["scale"][n]
    _report("local_attn", (shape, variant), worst, BOUND)
    assert max(worst.values()) < BOUND, (shape, variant, worst)
    idle = la_uncited(shape, variant)
    if variant == "hub" and K < N:
        assert int(idle.sum()) == B * (N - K)
    dkv = dqkv[:, C:].cpu().permute(0, 2, 1)                              # (B,N,2C)
    assert bool((dkv[idle] == 0).all()) and bool((want["dqkv"][:, C:].permute(0, 2, 1)[idle] == 0).all())


def test_local_attn_edge_buffer_matches_float64():
    """the per-edge gradients of pcr_local_attn_train_bwd_f32 themselves, before the grouping backward folds them"""
    from pcr_amd import _lib as L
    shape, variant = LA_EDGE_CASE
    B, C, N, K, H = shape
    inp, want = make_la_input(shape, variant), la_want(shape, variant)
    qkv, idx, go = inp["qkv"].cuda(), inp["idx"].cuda(), inp["go"].cuda()
    runs = []
    for _ in range(2):
        dq = torch.full((B, 3 * C, N), SENTINEL, device="cuda")
        edge = torch.full((B, 2 * C, N, K), SENTINEL, device="cuda")
        L.run.pcr_local_attn_train_bwd_f32(qkv, idx, go, dq, 3 * C * N, edge, B, N, C, K, H, ATTN_EPS, L.stream_ptr())
        torch.cuda.synchronize()
        runs.append([dq, edge])
    _same(*runs)
    dq, edge = runs[0]
    assert bool((dq[:, C:] == SENTINEL).all())                            # only the q rows of the (B,3C,N) gradient
    worst = dict(dq=_vs(dq[:, :C], want["dqkv"][:, :C]), ek=_vs(edge[:, :C], want["edge"][:, :C]),
                 ev=_vs(edge[:, C:], want["edge"][:, C:]))
    _report("local_attn edge", (shape, variant), worst, BOUND)
    assert max(worst.values()) < BOUND, worst


# ------------------------------------------------------------------------------------------- PoolPair --
def _pp_run(case):
    from pcr_amd import train_ops as TO
    inp = make_pool_input(case)
    o = inp["o"].cuda().requires_grad_(True)
    pooled = TO.PoolPair.apply(o)
    arg, = pooled.grad_fn.saved_tensors
    return [pooled.detach(), arg.clone(), torch.autograd.grad(pooled, o, inp["go"].cuda())[0]]


@pytest.mark.parametrize("case", PP_CASES)
def test_pool_pair_matches_float64(case):
    P, C, Ln = case
    inp = make_pool_input(case)
    o64, go64 = inp["o"].to(F64), inp["go"].to(F64)
    want, warg = R.pool_pair_ref(o64)
    wd = R.pool_pair_bwd_ref(go64, warg, Ln)
    runs = [_pp_run(case) for _ in range(2)]
    _same(*runs)
    pooled, arg, dout = (t.cpu() for t in runs[0])
    assert torch.equal(arg.long(), warg)
    planted = pool_planted_arg(case)                                      # and both take the planted ties as stated
    assert torch.equal(arg.long()[planted >= 0], planted[planted >= 0])
    assert torch.equal(pooled[:, :C].to(F64), want[:, :C])                # maxima are copies
    routed = torch.zeros(P, C, 2 * Ln, dtype=torch.bool).scatter_(2, warg.unsqueeze(2), True)
    routed = torch.cat([routed[:, :, :Ln], routed[:, :, Ln:]], dim=0)
    mean_only = R.pool_pair_bwd_ref(torch.cat([torch.zeros(P, C, dtype=F64), go64[:, C:]], dim=1), warg, Ln)
    worst = dict(mean=_vs(pooled[:, C:], want[:, C:]), dmean=_vs(dout[~routed], mean_only[~routed]), dout=_vs(dout, wd))
    _report("pool_pair", case, worst, MEAN_BOUND)
    assert max(worst.values()) < MEAN_BOUND, (case, worst)
