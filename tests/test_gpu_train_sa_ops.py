"""GPU: the launches of the grouped-MLP training path (pcr_amd.train_ops.SaEdgeTrain / dense and what they call:
pcr_sa_l1_*, pcr_tdense_*, pcr_sa_pool_*, pcr_bn_*_finalize), one by one against the float64 references of
tests/train_ref.py, at the shapes where their dispatch changes kernel or plan (the backward's by the rule its dispatch
applies, LDS gate included, not by width alone), and bit-reproducibility of all of it (no float atomics anywhere).

Bounds (`_rel` = max|a - b| / max|b| against float64), all the project's own: selections, indices, routed copies and
zeros exact; single-rounding results (pooled, the finalize outputs) 1e-6 (MEAN_BOUND); matrix products and their sums
1e-5 (test_gpu_train_stream.py); the split-bf16 128 x 128 backward 3e-5 (the grad_floor fixture); BatchNorm
compositions, the stressed ones included, 2e-5 (BN_BOUND).  Inputs are conditioned (train_ref) so that the float64
reference takes no marginal ReLU / max-pool decision; every test asserts that on the CPU before it launches.  The case
tables and input builders are shared with test_train_ref_cpu.py, which shows without a device that every input
conditions to zero marginal decisions by moving at most 0.1 % of its elements."""
import json
import math
import zlib

import pytest
import torch

import train_ref as R
from pcr_amd import _lib as L
from test_gpu_train_pointwise_ops import BN_BOUND, EPS, MEAN_BOUND, _planted, _rel, _vs

pytestmark = pytest.mark.gpu

F64 = torch.float64
PROD_BOUND = 1e-5
BF_BOUND = 3e-5
TILE, STREAM = 1 << 30, 0          # pcr_set_stream_min_blocks: every launch on the tile kernels / on the streaming ones
MOVE_CAP = 1e-3                    # conditioning may move this fraction of a case's elements, no more

# ---------------------------------------------------------------------------------------------- cases --
# layer 1 (B, N, S, K, c1); channel chunk = min(c1, 32 halved while chunk N 4 > 32 KiB) rounded down to a power of two:
# S = N; four chunks; chunk 16 with four live channels in the second, L = 740 (a 36-row tail tile); one live channel in
# chunk two, L = 35 < 64; chunk 16; chunk 8; chunk 4; K = 1; K > the 64-row tile; K = the tile
L1_SHAPES = [(3, 128, 128, 32, 32), (2, 64, 32, 48, 128), (3, 100, 37, 20, 20), (2, 50, 7, 5, 33), (2, 300, 150, 16, 64),
             (1, 600, 64, 16, 24), (1, 1100, 32, 8, 6), (2, 64, 64, 1, 32), (2, 40, 8, 96, 16), (2, 48, 6, 64, 16)]
# (shape, index set, with tables): "hot" = every row gathers point N - 1 (one owner takes all L rows), "repeat" = a
# neighbour listed twice within a centre, "knn" = engine.knn_prefix of the cloud
L1_CASES = [(s, "random", True) for s in L1_SHAPES] + [(L1_SHAPES[0], "random", False), (L1_SHAPES[3], "random", False),
                                                        (L1_SHAPES[2], "hot", True), (L1_SHAPES[8], "hot", True),
                                                        (L1_SHAPES[3], "repeat", True), (L1_SHAPES[1], "repeat", True),
                                                        (L1_SHAPES[0], "knn", True)]
# train-dense forward, tile kernels (B, cin1, cin2, cout, L): one instantiation per ceil32(cout) / 32 in {1, 2, 3-4, 5-8,
# 9-12} times one per input-prefetch depth (cin <= 32, <= 64, <= 128, above)
FWD_SHAPES = [(3, 32, 0, 32, 100), (2, 64, 0, 64, 77), (2, 128, 0, 128, 64), (2, 20, 13, 96, 33), (1, 131, 0, 160, 130),
              (2, 64, 64, 256, 65), (1, 288, 0, 384, 40), (5, 7, 0, 5, 1), (800, 16, 0, 32, 8)]
FWD_FLAGS = ("plain", "bn", "res", "relu", "res_relu")       # "bn": isc / ish / in_relu + bias + stats
FWD_CASES = [(s, f) for s in FWD_SHAPES for f in FWD_FLAGS]
# train-dense backward, tile kernels (B, cin1, cin2, cout, L), by the dispatch of pcr_tdense_bwd_f32 (LDS of a launch =
# ((max(coutP, cinP) + cinP) 65 + 3 cout + 3 cin1) 4 bytes; the narrow kernels p1 / o3 / o4 take at most four 32 x 32 dW
# tiles and 40 KiB): p1 (32 x 32); o3 (cin 33-64, cout <= 64); o3 ragged; 32 -> 128 (43,520 B: past the 40 KiB gate, the
# generic kernel at one input block); 128 x 128 (split bf16 under "bf16x3"); generic at 1, 3, 5 and 8 input blocks, the
# last with grid.z = 4; x2; many clouds; then o4 (cin <= 32, cout 33-96: the 32 -> 64 layer of SaEdgeTrain), generic at 2
# input blocks (cin 33-64, cout >= 96: its 64 -> 128 layer), generic at 9 input blocks (cin 257-288, 156,288 B: a corner
# the LDS rule still admits)
BWD_SHAPES = [(3, 32, 0, 32, 96), (2, 64, 0, 64, 77), (2, 48, 0, 40, 50), (2, 32, 0, 128, 64), (2, 128, 0, 128, 64),
              (2, 24, 0, 160, 33), (1, 96, 0, 96, 70), (1, 131, 0, 32, 130), (1, 256, 0, 256, 40), (2, 3, 64, 128, 77),
              (800, 32, 0, 32, 8), (2, 32, 0, 64, 64), (2, 64, 0, 128, 64), (1, 288, 0, 256, 40)]
SQUARE128 = (2, 128, 0, 128, 64)
BWD_CASES = [(s, m, "f32") for s in BWD_SHAPES for m in range(4)] + [(SQUARE128, m, "bf16x3") for m in range(4)]
POOL_KS = (1, 5, 32)
# the shapes test_gpu_train_stream.py runs through the wave-autonomous kernels: forward (B, cin, cout, L), backward
# (B, c, S, K, mode)
STREAM_FWD = [(3, 32, 32, 4096), (5, 32, 32, 96), (2, 64, 64, 3072), (7, 64, 64, 32), (3, 32, 64, 160), (3, 64, 32, 640),
              (130, 32, 32, 64), (2, 128, 128, 1536), (37, 128, 128, 32)]
STREAM_BWD = [(3, 32, 128, 32, 1), (3, 32, 128, 32, 3), (2, 32, 64, 48, 3), (5, 32, 3, 32, 1), (130, 32, 2, 16, 3),
              (4, 32, 40, 20, 3), (3, 64, 64, 48, 1), (2, 64, 64, 48, 3), (9, 64, 1, 32, 3), (70, 64, 2, 16, 1)]
# train_ops.dense (cout, cin) at L = 40, B = 1: the corner the backward's LDS rule refuses (dense() tiles it), the chunked
# path, and the last shapes the rule admits (one launch each, about 156 KB of LDS)
ENVELOPE = [(384, 224), (384, 256), (384, 288), (352, 288), (320, 288), (385, 64), (64, 289), (256, 288), (288, 256),
            (384, 192)]
ADMITTED = ENVELOPE[-3:]
# pooling (B, C, S, K): both staging paths (K % 4), every count of centres per tile from 192 down to 1, a tail tile, S
# below one tile, a channel block with one live channel
POOL_CASES = [(3, 32, 128, 32), (2, 33, 7, 5), (2, 7, 300, 1), (2, 64, 5, 48), (1, 32, 3, 96), (2, 32, 2, 100), (1, 40, 2, 192)]
FUSED = [(3, 32, 128, 32), (1, 32, 3, 96)]          # ... of which pcr_tdense_fwd_pooled takes these through the streaming launch
UNFUSED = [c for c in POOL_CASES if c not in FUSED]
FIN_CASES = [(n, C) for n in (1, 31, 33, 70, 1100) for C in (7, 32, 33, 256)]
# compositions: (lower launch, stress).  Stress = channel mean at 10 standard deviations (EDGE_CASES "stress"), injected
# through the bias, or through a part of the layer no launch could know in advance: a rank-one component a u^T of W (dense) /
# the centre half of the table (layer 1)
COMP_CASES = [(low, s) for low in ("l1", "tile", "stream") for s in ("none", "bias", "rank1")]
COMP_DENSE = (4, 64, 64, 256)      # (B, c0, c1, L)
COMP_L1 = (4, 128, 4, 32, 32)      # (B, N, S, K, c1): S K = N, the neighbour lists a permutation of the cloud
COMP_C2 = 64
STRESS = 10.0
# (table, case) -> seed offset, where the plain seed conditions more than MOVE_CAP of the case
SALT = {("bwd", (2, 3, 64, 128, 77), 2, 0): 1, ("bwd", (2, 3, 64, 128, 77), 3, 1): 1}


def _gen(tag, *key):
    flat = []
    for v in key:
        flat += list(v) if isinstance(v, tuple) else [v]
    flat = [zlib.crc32(v.encode()) if isinstance(v, str) else int(v) for v in [tag] + flat]     # (a stable hash of the names)
    salt = SALT.get((tag,) + tuple(key), 0)
    return torch.Generator().manual_seed((sum((i + 1) * 7919 * v for i, v in enumerate(flat)) + salt) % (2 ** 31))


def _pos(n, g):
    return torch.rand(n, generator=g) + 0.5


# --------------------------------------------------------------------------------------------- inputs --
def make_l1_input(shape, variant, with_tab, knn=None):
    """float32 CPU tensors of one layer-1 case; knn(xyz, S, K) -> (B,S,K) int32 serves the "knn" variant"""
    B, N, S, K, c1 = shape
    g = _gen("l1", shape, variant, with_tab)
    xyz = torch.randn(B, N, 3, generator=g)
    if variant == "knn":
        idx = knn(xyz, S, K)
    elif variant == "hot":
        idx = torch.full((B, S, K), N - 1, dtype=torch.int32)
    else:
        idx = torch.randint(0, N, (B, S, K), generator=g, dtype=torch.int32)
        if variant == "repeat":
            idx[:, :, K // 2:2 * (K // 2)] = idx[:, :, :K // 2]
    Ln = S * K
    return dict(xyz=xyz, idx=idx.contiguous(), tab=torch.randn(B, 2 * c1, N, generator=g) if with_tab else None,
                wa=torch.randn(c1, 3, generator=g), bias=torch.randn(c1, generator=g),
                g=torch.randn(B, c1, Ln, generator=g), y=torch.randn(B, c1, Ln, generator=g),
                ka=_pos(c1, g), kb=torch.randn(c1, generator=g) * 0.05, kc=torch.randn(c1, generator=g) * 0.05)


def fwd_ref(inp, with_pre=False):
    d = lambda t: None if t is None else t.to(F64)
    return R.tdense_ref(d(inp["x"]), d(inp["x2"]), d(inp["W"]), d(inp["bias"]), d(inp["isc"]), d(inp["ish"]), inp["in_relu"],
                        d(inp["res"]), inp["out_relu"], with_pre=with_pre)


def fwd_marginals(inp):
    n = R.relu_arg_marginals(inp["x"], inp["isc"], inp["ish"]) if inp["in_relu"] else 0
    return n + (R.value_marginals(fwd_ref(inp, True)[1] + (0 if inp["res"] is None else inp["res"].to(F64)))
                if inp["out_relu"] else 0)


def make_fwd_input(shape, flags):
    """float32 CPU tensors of one forward case, conditioned: `moved` ReLU arguments out of `total`"""
    B, cin1, cin2, cout, Ln = shape
    g = _gen("fwd", shape, flags)
    inp = dict(x=torch.randn(B, cin1, Ln, generator=g), x2=torch.randn(B, cin2, Ln, generator=g) if cin2 else None,
               W=torch.randn(cout, cin1 + cin2, generator=g) / math.sqrt(cin1 + cin2), bias=None, isc=None, ish=None,
               in_relu=False, res=None, out_relu=flags in ("relu", "res_relu"), stats=False, moved=0)
    inp["total"] = B * cin1 * Ln
    if flags == "bn":
        inp.update(bias=torch.randn(cout, generator=g), isc=_pos(cin1, g), ish=torch.randn(cin1, generator=g) * 0.3,
                   in_relu=True, stats=cout <= 256)                 # (the launch takes statistics up to cout = 256)
        inp["x"], inp["moved"] = R.condition_relu_args(inp["x"], inp["isc"], inp["ish"])
    if flags in ("res", "res_relu"):
        inp["res"] = torch.randn(B, cout, Ln, generator=g)
    if inp["out_relu"]:
        inp["total"] = B * cout * Ln

        def y_of(x, res):
            return fwd_ref(dict(inp, x=x, res=res, out_relu=False))
        inp["x"], inp["res"], inp["moved"] = R.condition_out_relu(y_of, inp["res"], inp["x"], inp["W"])
    return inp


def bwd_ks(shape):
    """the K of dy_mode 3 that divide L"""
    return [K for K in POOL_KS if shape[4] % K == 0]


def make_bwd_input(shape, mode, K=0):
    """float32 CPU tensors of one backward case (mode 3: S K = L); x conditioned for the input ReLU"""
    B, cin1, cin2, cout, Ln = shape
    g = _gen("bwd", shape, mode, K)
    inp = dict(x=torch.randn(B, cin1, Ln, generator=g), x2=torch.randn(B, cin2, Ln, generator=g) if cin2 else None,
               W=torch.randn(cout, cin1 + cin2, generator=g) / math.sqrt(cin1 + cin2),
               y=torch.randn(B, cout, Ln, generator=g), isc=_pos(cin1, g), ish=torch.randn(cin1, generator=g) * 0.3,
               k=dict(ka=_pos(cout, g), kb=torch.randn(cout, generator=g) * 0.05, kc=torch.randn(cout, generator=g) * 0.05),
               argmax=None, pooled=None, K=K, S=Ln // K if K else 0, total=B * cin1 * Ln)
    if mode == 2:
        inp["y"] = torch.relu(inp["y"])          # the layer stored after its ReLU: exact zeros, y > 0 is decided on float32
    if mode == 3:
        S = Ln // K
        inp.update(g=torch.randn(B, cout, S, generator=g), pooled=torch.randn(B, cout, S, generator=g),
                   argmax=torch.randint(0, K, (B, cout, S), generator=g, dtype=torch.int32))
    else:
        inp["g"] = torch.randn(B, cout, Ln, generator=g)
    inp["x"], inp["moved"] = R.condition_relu_args(inp["x"], inp["isc"], inp["ish"])
    return inp


def make_pool_input(shape):
    """float32 CPU tensors of one pooling case: rows planted as `_planted` does (on the winning side of each channel's
    scale), scale negative on channel 0 and exactly zero on channel 1, conditioned"""
    B, C, S, K = shape
    g = _gen("pool", shape)
    scale = _pos(C, g) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    shift = (0.05 + 0.15 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    scale[0] = -scale[0].abs()
    scale[1] = 0.0
    side = torch.where(scale < 0, -1.0, 1.0).view(1, C, 1, 1)
    v = _planted(B * C * S, K, g).view(B, C, S, K) * side
    y0 = v.reshape(B, C, S * K).contiguous()
    y, _ = R.condition_pool(y0, scale, shift, K)
    return dict(y=y, scale=scale, shift=shift, gp=torch.randn(B, C, S, generator=g), moved=int((y != y0).sum()),
                total=y.numel())


def _ratio(y):
    return y.mean(dim=(0, 2)).abs() / y.std(dim=(0, 2))


def _affine(C, g):
    """gamma = 1 + 0.3 N(0,1), channel 0 negative; beta = 0.1 N(0,1)"""
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    gamma[0] = -gamma[0].abs() - 0.1
    return gamma, 0.1 * torch.randn(C, generator=g)


def comp_lower_ref(inp, leaves=None):
    """float64 output y1 (B,c1,L) of a composition's lower launch from its float32 inputs (or from the given leaves)"""
    d = leaves or {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
    if inp["low"] == "l1":
        return R.sa_l1_ref(d["xyz"], inp["idx"], d["tab"], d["wa"], d["bias"])
    z0 = d["z0"] if "z0" in d else R._ch(d["isc"]) * d["x"] + R._ch(d["ish"])
    return torch.einsum("oc,bcl->bol", d["W"], torch.relu(z0)) + R._ch(d["bias"])


def make_comp_input(low, stress):
    """float32 CPU tensors of one composition case.  The lower launch's output y1 is normalised (gamma, beta), passed
    through a ReLU and multiplied by W2; its inputs are conditioned THROUGH the launch so that no BatchNorm output lies
    within delta of zero: layer 1 through the neighbour half of the table (the lists are a permutation: one table entry
    per row), the dense layer through the token's column of x along the row of W (open channels only).  The dense
    layer's own input ReLU arguments isc x + ish start well clear of zero (|x| >= 0.5) and are checked again afterwards."""
    g = _gen("comp", low, stress)
    if low == "l1":
        B, N, S, K, c1 = COMP_L1
        Ln = S * K
        inp = dict(low=low, xyz=torch.randn(B, N, 3, generator=g),
                   idx=torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).view(B, S, K).to(torch.int32),
                   tab=torch.randn(B, 2 * c1, N, generator=g), wa=torch.randn(c1, 3, generator=g),
                   bias=torch.randn(c1, generator=g))
    else:
        B, c0, c1, Ln = COMP_DENSE
        mag = torch.randn(B, c0, Ln, generator=g).abs() + 0.5
        x = mag + 3.0 if stress == "rank1" else mag * torch.where(torch.rand(B, c0, Ln, generator=g) < 0.5, -1.0, 1.0)
        inp = dict(low=low, x=x, W=torch.randn(c1, c0, generator=g) / math.sqrt(c0), bias=torch.randn(c1, generator=g),
                   isc=_pos(c0, g), ish=0.1 * torch.randn(c0, generator=g))
        inp["x"], _ = R.condition_relu_args(inp["x"], inp["isc"], inp["ish"])
    inp["gamma"], inp["beta"] = _affine(c1, g)
    inp["W2"] = torch.randn(COMP_C2, c1, generator=g) / math.sqrt(c1)
    inp["dy2"] = torch.randn(B, COMP_C2, Ln, generator=g)
    y = comp_lower_ref(inp)
    sd = y.std(dim=(0, 2))
    if stress == "bias":
        inp["bias"] = (inp["bias"].to(F64) + STRESS * sd - y.mean(dim=(0, 2))).to(torch.float32)
    elif stress == "rank1" and low == "l1":
        inp["tab"][:, c1:] += (STRESS * sd - y.mean(dim=(0, 2))).to(torch.float32).view(1, c1, 1)
    elif stress == "rank1":
        # W + a u^T, u = 1 / c0: the common mode t = mean_c f(x) joins output channel o with weight a[o], the root of
        # (m + a mt)^2 = STRESS^2 (v + 2 a cov + a^2 vt) with the smaller |a| and a positive mean
        t = torch.relu(R._ch(inp["isc"].to(F64)) * inp["x"].to(F64) + R._ch(inp["ish"].to(F64))).mean(dim=1, keepdim=True)
        m, v, mt, vt = y.mean(dim=(0, 2)), y.var(dim=(0, 2)), float(t.mean()), float(t.var())
        cov = ((y - R._ch(m)) * (t - mt)).sum(dim=(0, 2)) / (y.shape[0] * y.shape[2] - 1)
        qa, qb, qc = mt * mt - STRESS ** 2 * vt, 2 * m * mt - 2 * STRESS ** 2 * cov, m * m - STRESS ** 2 * v
        disc = torch.sqrt(qb * qb - 4 * qa * qc)
        roots = torch.stack([(-qb + disc) / (2 * qa), (-qb - disc) / (2 * qa)])
        roots = torch.where(m + roots * mt > 0, roots, torch.full_like(roots, float("inf")))
        a = roots.gather(0, roots.abs().argmin(dim=0, keepdim=True))[0]
        inp["W"] = (inp["W"].to(F64) + a.view(-1, 1) / c0).to(torch.float32)
    base = {k: v.clone() for k, v in inp.items() if torch.is_tensor(v)}

    def push(dy):
        if low == "l1":
            li = inp["idx"].long().view(B, 1, Ln).expand(B, c1, Ln)
            t = inp["tab"].to(F64)
            t[:, :c1] = t[:, :c1].scatter_add(2, li, dy)
            inp["tab"] = t.to(torch.float32)
        else:
            z0 = R._ch(inp["isc"].to(F64)) * inp["x"].to(F64) + R._ch(inp["ish"].to(F64))
            m = (z0 > 0).to(F64)
            J = inp["W"].to(F64) * inp["isc"].to(F64).view(1, -1)
            n2 = torch.einsum("oc,bcl->bol", J * J, m)
            inp["x"] = (inp["x"].to(F64) + m * torch.einsum("oc,bol->bcl", J, dy / n2)).to(torch.float32)
    inp["moved"] = R.condition_bn_through(lambda: comp_lower_ref(inp), push, inp["gamma"], inp["beta"], EPS)
    key = "tab" if low == "l1" else "x"
    inp["changed"], inp["total"] = int((inp[key] != base[key]).sum()), y.numel()
    return inp


def comp_marginals(inp):
    n = _bn_marginals(comp_lower_ref(inp), inp["gamma"], inp["beta"])
    if inp["low"] != "l1":
        n += R.relu_arg_marginals(inp["x"], inp["isc"], inp["ish"])
    return n


def _bn_marginals(y64, gamma, beta):
    z = R._bn(y64, gamma.to(F64), beta.to(F64), EPS, (0, 2))[0]
    return int((z.abs() < R.REL_DELTA * z.abs().max()).sum())


# -------------------------------------------------------------------------------------------- helpers --
class _policy:
    """pcr_set_stream_min_blocks for the duration of a with-block"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = L.load().pcr_set_stream_min_blocks(self.n)

    def __exit__(self, *a):
        L.load().pcr_set_stream_min_blocks(self.old)


def _cu(t):
    return None if t is None else t.cuda()


def _d(t):
    return None if t is None else t.to(F64)


def _report(op, case, worst):
    print(json.dumps(dict(op=op, case=str(case), worst=worst)))
    assert all(math.isfinite(v) for v in worst.values()), worst          # (max() and < both let a NaN through)


def _keep(worst, key, val):
    """the larger of worst[key] and val; a NaN or an infinity fails here (max(0.0, nan) is 0.0)"""
    assert math.isfinite(val), (key, val)
    worst[key] = max(worst.get(key, 0.0), val)


def _rows_vs(worst, name, got, want):
    """a (2, C) record of sums, each row under its own norm (the second row is a sum of products: sqrt(R) or more larger)"""
    worst[name + "_1"], worst[name + "_2"] = _vs(got[0], want[0]), _vs(got[1], want[1])


def _same(a, b):
    """two runs' results (lists / dicts of tensors or None) bit for bit"""
    if isinstance(a, dict):
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(b)]
    for s, t in zip(a, b):
        assert (s is None and t is None) or torch.equal(s, t)


def _sums(part, C):
    """partial records (nparts, 2, CP) -> (2, C)"""
    return part.sum(0)[:, :C]


def _zeros_like_part(n, C):
    return torch.zeros(n, 2, L._c32(C), device="cuda")


# -------------------------------------------------------------------------------------------- layer 1 --
def _device_knn(xyz, S, K):
    from pcr_amd import engine
    return engine.knn_prefix(xyz.cuda().contiguous(), S, K).cpu()


def _l1_launch(inp, shape):
    from pcr_amd import train_ops as TO
    B, N, S, K, c1 = shape
    Ln = S * K
    xyz, idx, tab = inp["xyz"].cuda(), inp["idx"].cuda(), _cu(inp["tab"])
    y = torch.empty(B, c1, Ln, device="cuda")
    st = _zeros_like_part(B, c1)
    L.run.pcr_sa_l1_fwd_f32(xyz, idx, tab, inp["wa"].cuda(), inp["bias"].cuda(), y, st, B, N, S, K, c1, L.stream_ptr())
    dtab = torch.empty(B, 2 * c1, N, device="cuda") if tab is not None else None
    dwa_p = torch.empty(B, c1, 4, device="cuda")
    L.run.pcr_sa_l1_bwd_f32(xyz, idx, inp["g"].cuda(), inp["y"].cuda(), inp["ka"].cuda(), inp["kb"].cuda(), inp["kc"].cuda(),
                            dtab, dwa_p, B, N, S, K, c1, L.stream_ptr())
    return [y, st, dtab, TO.reduce_parts(dwa_p, B, c1 * 4, c1, 4, 4)]


def _l1_want(inp, with_tab):
    """-> (y, [dwa, dbias(, dtab)]) in float64"""
    leaves = [t.to(F64).requires_grad_(True) for t in (inp["wa"], inp["bias"])] + \
             ([inp["tab"].to(F64).requires_grad_(True)] if with_tab else [])
    y64 = R.sa_l1_ref(inp["xyz"].to(F64), inp["idx"], leaves[2] if with_tab else None, leaves[0], leaves[1])
    k = {n: inp[n].to(F64) for n in ("ka", "kb", "kc")}
    dy = R.tdense_dy(1, inp["g"].to(F64), inp["y"].to(F64), k)
    return y64.detach(), torch.autograd.grad(y64, leaves, dy)


@pytest.mark.parametrize("shape,variant,with_tab", L1_CASES)
def test_sa_l1_matches_float64(shape, variant, with_tab):
    """y, the summed statistics, dtab (both halves, the centre half exactly zero beyond S), dwa and dbias within 1e-5.  The
    launches are linear: nothing to condition.  Observed worst _rel on the MI355X: y 1.2e-7, sums of y 1.2e-7, of y^2 1.0e-7
    (each row of the record under its own norm), dwa 5.0e-7, dbias 2.4e-7, dtab neighbour half 5.0e-7, centre half 2.5e-7."""
    B, N, S, K, c1 = shape
    inp = make_l1_input(shape, variant, with_tab, _device_knn)
    idx = inp["idx"]
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < N
    if variant == "repeat":
        assert K >= 2 and bool((idx[:, :, 0] == idx[:, :, K // 2]).all())
    runs = [_l1_launch(inp, shape) for _ in range(2)]
    _same(*runs)
    y, st, dtab, dwa4 = runs[0]
    y64, grads = _l1_want(inp, with_tab)
    worst = dict(y=_vs(y, y64), dwa=_vs(dwa4[:, :3], grads[0]), dbias=_vs(dwa4[:, 3], grads[1]))
    _rows_vs(worst, "stats", _sums(st, c1), R.stats_ref(y64))
    if with_tab:
        assert bool((grads[2][:, c1:, S:] == 0).all())
        assert bool((dtab[:, c1:, S:] == 0).all())
        worst["dtab_p"] = _vs(dtab[:, :c1], grads[2][:, :c1])
        worst["dtab_q"] = _vs(dtab[:, c1:], grads[2][:, c1:])
    _report("sa_l1", (shape, variant, with_tab), worst)
    assert max(worst.values()) < PROD_BOUND, worst


# -------------------------------------------------------------------------------- train-dense forward --
def _fwd_launch(inp, cout, policy):
    from pcr_amd import train_ops as TO
    with _policy(policy):
        y, st = TO.tdense_fwd(inp["x"].cuda(), TO.pack_dev(inp["W"].cuda()), cout, x2=_cu(inp["x2"]), isc=_cu(inp["isc"]),
                              ish=_cu(inp["ish"]), in_relu=inp["in_relu"], bias=_cu(inp["bias"]), res=_cu(inp["res"]),
                              out_relu=inp["out_relu"], want_stats=inp["stats"])
    return [y, st]


def _check_fwd(inp, cout, policy, tag, case):
    assert fwd_marginals(inp) == 0
    runs = [_fwd_launch(inp, cout, policy) for _ in range(2)]
    _same(*runs)
    y64, pre64 = fwd_ref(inp, with_pre=True)
    worst = dict(y=_vs(runs[0][0], y64))
    if inp["stats"]:
        _rows_vs(worst, "stats", _sums(runs[0][1], cout), R.stats_ref(pre64))
        if policy == STREAM:          # the wave-autonomous kernel took the launch: its grid is not the tile kernels'
            assert runs[0][1].shape[0] != L.load().pcr_train_groups(inp["x"].shape[0], inp["x"].shape[2])
    _report(tag, case, worst)
    assert max(worst.values()) < PROD_BOUND, worst


@pytest.mark.parametrize("shape,flags", FWD_CASES)
def test_tdense_fwd_tile_matches_float64(shape, flags):
    """y and the summed statistics within 1e-5 on the tile kernels, per flag set the header allows.  Observed worst _rel on
    the MI355X: y 6.0e-7 (the widest launch), sums of y 1.1e-7, of y^2 9.8e-8."""
    _check_fwd(make_fwd_input(shape, flags), shape[3], TILE, "tdense_fwd", (shape, flags))


@pytest.mark.parametrize("B,cin,cout,Ln", STREAM_FWD)
def test_tdense_fwd_stream_matches_float64(B, cin, cout, Ln):
    """the same reference on the wave-autonomous kernels, at the shapes test_gpu_train_stream.py lists; the row count of the
    statistics record shows that the streaming kernel took the launch.  Observed worst _rel on the MI355X: y 4.6e-7, sums of
    y 1.2e-7, of y^2 1.1e-7."""
    shape = (B, cin, 0, cout, Ln)
    _check_fwd(make_fwd_input(shape, "bn"), cout, STREAM, "tdense_fwd_stream", shape)


# ------------------------------------------------------------------------------- train-dense backward --
BWD_VARIANTS = {"relu": dict(in_relu=True, dx=True, dw=True), "plain": dict(in_relu=False, dx=True, dw=True),
                "no_dx": dict(in_relu=True, dx=False, dw=True), "no_dw": dict(in_relu=True, dx=True, dw=False)}


def _bwd_launch(inp, shape, mode, v, policy, routed, bf):
    from pcr_amd import train_ops as TO
    B, cin1, cin2, cout, Ln = shape
    W = inp["W"].cuda()
    g, pooled = inp["g"], inp["pooled"]
    if mode == 3 and routed:
        g, pooled = torch.where(pooled > 0, g, torch.zeros_like(g)), None
    aff = dict(isc=inp["isc"].cuda(), ish=inp["ish"].cuda(), iinv=(1.0 / inp["isc"]).cuda(), in_relu=True) if v["in_relu"] else {}
    with _policy(policy):
        return TO.tdense_bwd(g.cuda(), inp["x"].cuda(), cout, dy_mode=mode, y=_cu(inp["y"]) if mode else None,
                             k={n: t.cuda() for n, t in inp["k"].items()} if mode in (1, 3) else None,
                             argmax=_cu(inp["argmax"]), pooled=_cu(pooled), K=inp["K"], S=inp["S"], x2=_cu(inp["x2"]),
                             wpT=TO.pack_dev(W, transpose=True) if v["dx"] else None, want_dstats=v["dx"],
                             want_dw=v["dw"], wpT_bf=TO.pack_bf_T(W) if (bf and v["dx"]) else None, **aff)


def _bwd_want(inp, mode, v):
    dy = R.tdense_dy(mode, inp["g"].to(F64), _d(inp["y"]), {n: t.to(F64) for n, t in inp["k"].items()}, inp["argmax"],
                     _d(inp["pooled"]), inp["K"])
    return R.tdense_bwd_ref(dy, inp["x"].to(F64), _d(inp["x2"]), inp["W"].to(F64), inp["isc"].to(F64) if v["in_relu"] else None,
                            inp["ish"].to(F64) if v["in_relu"] else None, v["in_relu"])


def _check_bwd(inp, shape, mode, names, policy, bf, tag, case, worst_all):
    """one conditioned input through the named variants (and, in mode 3, with `pooled` given and routed)"""
    B, cin1, cin2, cout, Ln = shape
    assert R.relu_arg_marginals(inp["x"], inp["isc"], inp["ish"]) == 0
    for name in names:
        v = BWD_VARIANTS[name]
        want = _bwd_want(inp, mode, v)
        for routed in ((False, True) if mode == 3 else (False,)):
            if policy == STREAM and mode == 3 and not routed:
                continue                                   # (the streaming backward takes the routed form only)
            runs = [_bwd_launch(inp, shape, mode, v, policy, routed, bf) for _ in range(2)]
            _same(*runs)
            r = runs[0]
            assert ("dx" in r) == v["dx"] and ("dW" in r) == v["dw"]
            worst = {}
            if v["dx"]:
                worst["dx"] = _vs(r["dx"], want["dx"])
                _rows_vs(worst, "dstats", _sums(r["dstats"], cin1), want["dstats"])
                if policy == STREAM:  # the wave-autonomous kernel took the launch: its grid is not the tile kernels'
                    assert r["dstats"].shape[0] != L.load().pcr_train_groups_bwd(B, Ln, cout, cin1 + cin2)
                if cin2:
                    worst["dx2"] = _vs(r["dx2"], want["dx2"])
            if v["dw"]:
                worst["dW"], worst["db"] = _vs(r["dW"], want["dW"]), _vs(r["db"], want["db"])
            _report(tag, (case, name, "routed" if routed else ""), worst)
            for key, val in worst.items():
                _keep(worst_all, key, val)


@pytest.mark.parametrize("shape,mode,prec", BWD_CASES)
def test_tdense_bwd_tile_matches_float64(shape, mode, prec):
    """dx, dx2, dW, db and the summed dstats within 1e-5 (3e-5 for the split-bf16 128 x 128 kernel) on the tile kernels:
    with and without the input ReLU, without dx (wpT absent), without dW; dy_mode 3 at every K of {1, 5, 32} that divides
    L, with `pooled` given and in the routed form.  Observed worst _rel on the MI355X: dx 7.2e-7, dx2 6.5e-7, dW 3.2e-7,
    db 1.8e-7, dstats 6.3e-7 (sum dx) and 5.3e-7 (sum dx x); split bf16: dx 9.3e-6, dW 9.2e-6, dstats 5.2e-6 both rows."""
    from pcr_amd import train_ops as TO
    prev = TO.set_train_precision(prec)
    try:
        worst = {}
        ks = bwd_ks(shape) if mode == 3 else [0]
        for i, K in enumerate(reversed(ks)):
            inp = make_bwd_input(shape, mode, K)
            _check_bwd(inp, shape, mode, list(BWD_VARIANTS) if i == 0 else ["relu"], TILE, prec == "bf16x3", "tdense_bwd",
                       (shape, mode, prec, K), worst)
    finally:
        TO.set_train_precision(prev)
    assert max(worst.values()) < (BF_BOUND if prec == "bf16x3" else PROD_BOUND), worst


@pytest.mark.parametrize("B,c,S,K,mode", STREAM_BWD)
def test_tdense_bwd_stream_matches_float64(B, c, S, K, mode):
    """the same reference on the wave-autonomous backward, at the shapes test_gpu_train_stream.py lists; the row count of
    dstats shows that the streaming kernel took the launch.  Observed worst _rel on the MI355X: dx 3.1e-7, dW 2.1e-7,
    db 1.7e-7, dstats 1.4e-7 / 1.5e-7."""
    shape = (B, c, 0, c, S * K)
    worst = {}
    _check_bwd(make_bwd_input(shape, mode, K if mode == 3 else 0), shape, mode, ["relu"], STREAM, False, "tdense_bwd_stream",
               (shape, mode, K), worst)
    assert max(worst.values()) < PROD_BOUND, worst


# ------------------------------------------------------------------------------------------- envelope --
@pytest.mark.parametrize("cout,cin", ENVELOPE)
def test_dense_runs_every_shape_of_its_envelope(cout, cin):
    """train_ops.dense forward and backward against float64 within 1e-5 at the corners of the single-launch envelope and
    just past it: every shape dense() accepts must run -- the backward launch holds dy and the input of a 64-token tile in
    LDS together, dense() tiles what that rule refuses and sends the last shapes it admits to one launch.  Observed worst
    _rel on the MI355X: y 1.2e-6, dx 6.3e-7, dW 3.0e-7, db 1.4e-7."""
    from pcr_amd import train_ops as TO
    g = _gen("env", cout, cin)
    x0, W0 = torch.randn(1, cin, 40, generator=g), torch.randn(cout, cin, generator=g) / math.sqrt(cin)
    b0, go = torch.randn(cout, generator=g), torch.randn(1, cout, 40, generator=g)
    runs = []
    for _ in range(2):
        x, W, b = (t.cuda().requires_grad_(True) for t in (x0, W0, b0))
        y = TO.dense(x, W, b)
        runs.append([y.detach()] + list(torch.autograd.grad(y, [x, W, b], go.cuda())))
    _same(*runs)
    x, W, b = (t.to(F64).requires_grad_(True) for t in (x0, W0, b0))
    y = R.tdense_ref(x, None, W, b, None, None, False, None, False)
    want = [y.detach()] + list(torch.autograd.grad(y, [x, W, b], go.to(F64)))
    worst = {n: _vs(a, w) for n, a, w in zip(("y", "dx", "dW", "db"), runs[0], want)}
    _report("dense", (cout, cin), worst)
    assert max(worst.values()) < PROD_BOUND, worst


def test_dense_sends_what_the_lds_rule_admits_to_one_launch():
    """the three shapes the header names as taken fit the backward (test_dense_runs_every_shape_of_its_envelope runs them
    through ONE TDense: dense() tiles only what bwd_fits refuses), their neighbours one block of 32 further do not"""
    from pcr_amd import train_ops as TO
    for cout, cin in ADMITTED:
        assert TO.bwd_fits(cout, cin, cin), (cout, cin)
    for cout, cin in ((320, 288), (352, 256), (384, 224)):
        assert not TO.bwd_fits(cout, cin, cin), (cout, cin)


@pytest.mark.parametrize("cout,cin", [(384, 256), (384, 288), (352, 288), (384, 224)])
def test_tdense_bwd_launch_refuses_what_its_lds_rule_excludes(cout, cin):
    """the low-level backward validates its arguments before it launches: past the LDS rule it returns the
    invalid-argument status (not a launch error)"""
    from pcr_amd import train_ops as TO
    assert not TO.bwd_fits(cout, cin, cin)
    g = _gen("refuse", cout, cin)
    x, W = torch.randn(1, cin, 40, generator=g).cuda(), torch.randn(cout, cin, generator=g).cuda()
    with pytest.raises(L.PcrError, match="pcr_tdense_bwd_f32 failed: invalid argument"):
        TO.tdense_bwd(torch.randn(1, cout, 40, generator=g).cuda(), x, cout, wpT=TO.pack_dev(W, transpose=True))
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------- pooling --
def _pool_launch(inp, shape):
    B, C, S, K = shape
    y, gp = inp["y"].cuda(), inp["gp"].cuda()
    pooled, ym = torch.empty(B, C, S, device="cuda"), torch.empty(B, C, S, device="cuda")
    am = torch.empty(B, C, S, dtype=torch.int32, device="cuda")
    L.run.pcr_sa_pool_fwd_f32(y, inp["scale"].cuda(), inp["shift"].cuda(), pooled, am, ym, B, C, S, K, L.stream_ptr())
    part, gz = _zeros_like_part(B, C), torch.empty(B, C, S, device="cuda")
    L.run.pcr_sa_pool_bwd_stats_f32(gp, pooled, ym, part, gz, B, C, S, L.stream_ptr())
    return [pooled, am, ym, part, gz]


@pytest.mark.parametrize("shape", POOL_CASES)
def test_sa_pool_matches_float64(shape):
    """pooled within 1e-6; argmax = the first maximum of the activation wherever the row is open; ymax bit-equal to y at
    argmax; gz exact; S1 and S2, each under its own norm, within 1e-5 of the float64 sums.  Observed worst _rel on the
    MI355X: pooled 4.2e-8, S1 9.0e-8, S2 1.7e-7."""
    B, C, S, K = shape
    inp = make_pool_input(shape)
    assert R.pool_marginals(inp["y"], inp["scale"], inp["shift"], K) == (0, 0)
    runs = [_pool_launch(inp, shape) for _ in range(2)]
    _same(*runs)
    pooled, am, ym, part, gz = (t.cpu() for t in runs[0])
    p64, arg64, ymax64 = R.sa_pool_ref(inp["y"].to(F64), inp["scale"].to(F64), inp["shift"].to(F64), K)
    open_ = p64 > 0
    assert bool(open_.any()) and bool((~open_).any())
    assert torch.equal(pooled > 0, open_)
    assert torch.equal(am.long()[open_], arg64[open_])
    assert int(am.min()) >= 0 and int(am.max()) < K
    assert torch.equal(torch.gather(inp["y"].view(B, C, S, K), 3, am.long().unsqueeze(3)).squeeze(3), ym)
    gz64, s64 = R.pool_bwd_stats_ref(inp["gp"].to(F64), p64, ymax64)
    assert torch.equal(gz.to(F64), gz64)
    worst = dict(pooled=_rel(pooled.to(F64), p64))
    _rows_vs(worst, "sums", _sums(part, C), s64)
    _report("sa_pool", shape, worst)
    assert worst["pooled"] < MEAN_BOUND and max(worst["sums_1"], worst["sums_2"]) < PROD_BOUND, worst


def test_sa_pool_refuses_more_than_192_rows_per_centre():
    B, C, S, K = 1, 32, 2, 193
    y = torch.zeros(B, C, S * K, device="cuda")
    v = torch.ones(C, device="cuda")
    out = torch.empty(B, C, S, device="cuda")
    with pytest.raises(L.PcrError, match="pcr_sa_pool_fwd_f32 failed: invalid argument"):
        L.run.pcr_sa_pool_fwd_f32(y, v, v, out, torch.empty(B, C, S, dtype=torch.int32, device="cuda"), out.clone(), B, C, S, K,
                                  L.stream_ptr())
    torch.cuda.synchronize()


def _fused_launch(shape):
    """-> (gamma, generator, y, winners or None) of a square train-dense forward asked to pool its output over K"""
    from pcr_amd import train_ops as TO
    B, C, S, K = shape
    g = _gen("fused", shape)
    x, W = torch.randn(B, C, S * K, generator=g), torch.randn(C, C, generator=g) / math.sqrt(C)
    gamma = torch.randn(C, generator=g)
    gamma[0], gamma[1] = -gamma[0].abs() - 0.1, 0.0
    with _policy(STREAM):
        y, _, won = TO.tdense_fwd(x.cuda(), TO.pack_dev(W.cuda()), C, isc=_pos(C, _gen("f", C)).cuda(),
                                  ish=torch.zeros(C, device="cuda"), in_relu=True, bias=None, want_stats=True,
                                  pool=(K, gamma.cuda()))
    return gamma, g, y, won


def test_fused_pooling_declines_what_the_streaming_launch_does_not_take():
    """the pooling cases whose width, K or L the fused launch does not cover leave no winners: the caller pools itself"""
    for shape in UNFUSED:
        assert _fused_launch(shape)[3] is None, shape


@pytest.mark.parametrize("shape", FUSED)
def test_fused_pooling_matches_float64(shape):
    """where pcr_tdense_fwd_pooled takes the launch: the winners it leaves against the float64 pooling of the launch's own
    y on open rows.  (The launch compares float32 y as they are, and relu(scale y + shift) is monotone in y: no decision
    here is marginal.)"""
    B, C, S, K = shape
    runs = []
    for _ in range(2):
        gamma, g, y, won = _fused_launch(shape)
        assert won is not None
        runs.append([y, won[0], won[1]])
    _same(*runs)
    y, ymax, arg = (t.cpu() for t in runs[0])
    scale, shift = (gamma * 0.7).to(F64), (0.3 * torch.randn(C, generator=g)).to(F64)
    p64, arg64, ymax64 = R.sa_pool_ref(y.to(F64), scale, shift, K)
    open_ = p64 > 0
    assert torch.equal(torch.gather(y.view(B, C, S, K), 3, arg.long().unsqueeze(3)).squeeze(3), ymax)
    live = open_ & (scale != 0).view(1, C, 1)
    assert bool(live.any())
    assert torch.equal(arg.long()[live], arg64[live]) and torch.equal(ymax.to(F64)[live], ymax64[live])


# ------------------------------------------------------------------------------------------- finalize --
def make_fin_input(nparts, C):
    """partial records of sum y, sum y^2 whose variance is positive by construction (Cauchy-Schwarz), except channel 2's:
    planted negative; gamma = 0 on channel 1"""
    g = _gen("fin", nparts, C)
    n = 64.0
    CP = L._c32(C)
    mu, sd = torch.randn(CP, generator=g), _pos(CP, g)
    s = n * mu + math.sqrt(n) * sd * torch.randn(nparts, CP, generator=g)
    q = s * s / n + n * sd * sd * (0.5 + torch.rand(nparts, CP, generator=g))
    q[:, CLAMPED] = 0.5 * (s[:, CLAMPED].to(F64).sum() ** 2 / (nparts * nparts * n)).to(torch.float32)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    gamma[1] = 0.0
    return dict(part=torch.stack([s, q], dim=1).contiguous(), R=nparts * n, gamma=gamma, beta=beta,
                rm=torch.randn(C, generator=g), rv=_pos(C, g), shift0=torch.randn(C, generator=g),
                bpart=torch.randn(nparts, 2, CP, generator=g), mean=torch.randn(C, generator=g), invstd=_pos(C, g),
                centre=torch.randn(C, generator=g))


FIN_KEYS = ("scale", "shift", "inv_scale", "mean", "invstd")
BFIN_KEYS = ("ka", "kb", "kc", "dgamma", "dbeta")
CLAMPED = 2                         # make_fin_input's channel of negative variance: invstd = 1 / sqrt(eps), about 316


def _keep_fin(worst, key, got, want, apart=None):
    """one finalize output under `key`; channel `apart` under key + "_clamped" against its own magnitude (the clamped
    channel's invstd, scale and shift are some three hundred times every other channel's and would set the norm for all)"""
    if apart is None:
        return _keep(worst, key, _vs(got, want))
    rest = [c for c in range(want.numel()) if c != apart]
    _keep(worst, key, _vs(got[rest], want[rest]))
    _keep(worst, key + "_clamped", _vs(got[apart:apart + 1], want[apart:apart + 1]))


def _fin_check(inp, nparts, C, Rrows, worst, apart=None):
    from pcr_amd import train_ops as TO
    m = 0.5
    for running in (False, True):
        for off in (False, True):
            runs = []
            for _ in range(2):
                rm, rv = (inp["rm"].cuda(), inp["rv"].cuda()) if running else (None, None)
                o = TO.bn_fwd_finalize(inp["part"].cuda(), nparts, C, Rrows, inp["gamma"].cuda(), inp["beta"].cuda(), EPS, m, rm,
                                       rv, shift0=inp["shift0"].cuda() if off else None)
                runs.append([o[k] for k in FIN_KEYS] + [rm, rv])
            _same(*runs)
            want = R.bn_fwd_consts_ref(inp["part"].to(F64), C, Rrows, inp["gamma"].to(F64), inp["beta"].to(F64), EPS,
                                       inp["shift0"].to(F64) if off else None)
            for k, t in zip(FIN_KEYS, runs[0]):
                _keep_fin(worst, k, t, want[k], apart)
            assert float(runs[0][2][1]) == 0.0                       # gamma = 0: inv_scale = 0
            if running:
                _keep_fin(worst, "running_mean", runs[0][5], R.running_update(inp["rm"].to(F64), want["mean"], m), apart)
                _keep_fin(worst, "running_var", runs[0][6], R.running_update(inp["rv"].to(F64), want["unbiased"], m), apart)
    return want


@pytest.mark.parametrize("nparts,C", FIN_CASES)
def test_bn_finalize_launches_match_float64(nparts, C):
    """pcr_bn_fwd_finalize_f32 and pcr_bn_bwd_finalize_f32 alone on given partial records, every output within 1e-6: with
    and without running buffers (momentum 0.5, non-default starting values), with and without shift0 / centre; gamma = 0
    gives inv_scale = 0; a negative variance is clamped, and that channel (invstd = 1 / sqrt(eps)) is held to 1e-6 of its own
    magnitude apart from the others.  Observed worst _rel on the MI355X: 5.5e-8 (kc) on the ordinary channels, 6.0e-8 (shift)
    on the clamped one."""
    from pcr_amd import train_ops as TO
    inp = make_fin_input(nparts, C)
    worst = {}
    want = _fin_check(inp, nparts, C, inp["R"], worst, apart=CLAMPED)
    assert float(want["var"][CLAMPED]) == 0.0 and float(want["var"].max()) > 0.0    # the planted record is clamped
    for off in (False, True):
        runs = []
        for _ in range(2):
            o = TO.bn_bwd_finalize(inp["bpart"].cuda(), nparts, C, inp["R"], inp["gamma"].cuda(), inp["mean"].cuda(),
                                   inp["invstd"].cuda(), centre=inp["centre"].cuda() if off else None)
            runs.append([o[k] for k in BFIN_KEYS])
        _same(*runs)
        wb = R.bn_bwd_consts_ref(inp["bpart"].to(F64), C, inp["R"], inp["gamma"].to(F64), inp["mean"].to(F64),
                                 inp["invstd"].to(F64), inp["centre"].to(F64) if off else None)
        for k, t in zip(BFIN_KEYS, runs[0]):
            _keep(worst, k, _vs(t, wb[k]))
    _report("bn_finalize", (nparts, C), worst)
    assert max(worst.values()) < MEAN_BOUND, worst


def test_bn_fwd_finalize_of_one_row_applies_no_unbiased_correction():
    """R = 1: the running variance takes the biased variance (R / (R - 1) has no meaning; a 0 * inf there would be a NaN,
    which _keep refuses).  Observed worst _rel on the MI355X: 6.1e-8 (invstd)."""
    C = 33
    g = _gen("fin1", C)
    yv = torch.randn(L._c32(C), generator=g)
    inp = make_fin_input(1, C)
    inp["part"] = torch.stack([yv, yv * yv]).view(1, 2, -1).contiguous()
    worst = {}
    want = _fin_check(inp, 1, C, 1.0, worst)
    assert torch.equal(want["unbiased"], want["var"])
    _report("bn_finalize_R1", C, worst)
    assert max(worst.values()) < MEAN_BOUND, worst


# --------------------------------------------------------------------------------------- compositions --
def _comp_forward(inp, policy):
    """the lower launch and its finalize twice (two running-statistics steps) -> (y1, finalize outputs, running mean, var)"""
    from pcr_amd import train_ops as TO
    c1 = inp["gamma"].numel()
    if inp["low"] == "l1":
        B, N, S, K, _ = COMP_L1
        y1 = torch.empty(B, c1, S * K, device="cuda")
        st = _zeros_like_part(B, c1)
        L.run.pcr_sa_l1_fwd_f32(inp["xyz"].cuda(), inp["idx"].cuda(), inp["tab"].cuda(), inp["wa"].cuda(), inp["bias"].cuda(),
                                y1, st, B, N, S, K, c1, L.stream_ptr())
    else:
        with _policy(policy):
            y1, st = TO.tdense_fwd(inp["x"].cuda(), TO.pack_dev(inp["W"].cuda()), c1, isc=inp["isc"].cuda(),
                                   ish=inp["ish"].cuda(), in_relu=True, bias=inp["bias"].cuda(), want_stats=True)
    g = _gen("run", c1)
    rm, rv = torch.randn(c1, generator=g).cuda(), _pos(c1, g).cuda()
    Rrows = y1.shape[0] * y1.shape[2]
    for _ in range(2):
        n1 = TO.bn_fwd_finalize(st, st.shape[0], c1, Rrows, inp["gamma"].cuda(), inp["beta"].cuda(), EPS, 0.5, rm, rv)
    return y1, n1, rm, rv


def _comp_assert_input(inp, stress):
    assert comp_marginals(inp) == 0
    ratio = _ratio(comp_lower_ref(inp))
    if stress != "none":
        assert 9.0 < float(ratio.min()) and float(ratio.max()) < 11.5
    return float(ratio.min())


def _comp_stats_want(inp):
    y64 = comp_lower_ref(inp)
    gamma, beta = inp["gamma"].to(F64), inp["beta"].to(F64)
    _, mean, var, scale = R._bn(y64, gamma, beta, EPS, (0, 2))
    g = _gen("run", gamma.numel())
    rm0, rv0 = torch.randn(gamma.numel(), generator=g).to(F64), _pos(gamma.numel(), g).to(F64)
    n = y64.shape[0] * y64.shape[2]
    return dict(y=y64, running_mean=R.running_update(rm0, mean, 0.5, 2), running_var=R.running_update(rv0, R._unbiased(var, n), 0.5, 2),
                scale=scale.flatten(), shift=beta - mean * scale.flatten(), inv_scale=1.0 / scale.flatten(), mean=mean,
                invstd=1.0 / torch.sqrt(var + EPS))


@pytest.mark.parametrize("low,stress", COMP_CASES)
def test_forward_statistics_compose_to_float64_batchnorm(low, stress):
    """lower forward launch -> bn_fwd_finalize: mean, invstd, scale, shift and the running statistics after two steps
    against float64 BatchNorm of the float64 y, within 2e-5 -- unstressed and with the channel mean at 10 sigma.  The
    statistics of these launches are uncentred float32 sums (SaEdgeTrain passes no shift0), so 10 sigma costs a factor of
    twenty and still holds the bound by a factor of two.  Observed worst _rel on the MI355X, unstressed: invstd 3.5e-7,
    running var 4.8e-7, scale 3.0e-7, shift 4.0e-7, mean 5.3e-8; at 10 sigma: invstd 6.9e-6 (streaming launch, rank-one
    injection), running var 8.8e-6, shift 6.4e-6, scale 5.5e-6, mean 8.7e-8."""
    inp = make_comp_input(low, stress)
    _comp_assert_input(inp, stress)
    policy = STREAM if low == "stream" else TILE
    runs = []
    for _ in range(2):
        y1, n1, rm, rv = _comp_forward(inp, policy)
        runs.append([y1, rm, rv] + [n1[k] for k in FIN_KEYS])
    _same(*runs)
    want = _comp_stats_want(inp)
    worst = {k: _vs(t, want[k]) for k, t in zip(("y", "running_mean", "running_var") + FIN_KEYS, runs[0])}
    _report("comp_stats", (low, stress), worst)
    assert max(worst.values()) < BN_BOUND, worst


def _comp_bwd_want(inp):
    """float64 autograd through the whole graph: gradients by leaf name"""
    low = inp["low"]
    names = ("tab", "wa", "bias") if low == "l1" else ("z0", "W", "bias")
    d = {k: (v.to(F64) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
    if low != "l1":
        d["z0"] = R._ch(d["isc"]) * d["x"] + R._ch(d["ish"])
    for k in names + ("gamma", "beta", "W2"):
        d[k] = d[k].detach().requires_grad_(True)
    z1 = R._bn(comp_lower_ref(inp, d), d["gamma"], d["beta"], EPS, (0, 2))[0]
    out = torch.einsum("oc,bcl->bol", d["W2"], torch.relu(z1))
    return dict(zip(names + ("gamma", "beta", "W2"),
                     torch.autograd.grad(out, [d[k] for k in names + ("gamma", "beta", "W2")], d["dy2"])))


@pytest.mark.parametrize("low,stress", COMP_CASES)
def test_two_layer_backward_composes_to_float64_autograd(low, stress):
    """upper tdense_bwd (mode 0, input ReLU with the REAL scale / shift / inv_scale of the forward) -> dstats ->
    bn_bwd_finalize -> lower launch in mode 1 (tdense_bwd tile / streaming, sa_l1_bwd), against float64 autograd through
    W2 relu(BatchNorm(y1)): dgamma, dbeta and the lower launch's gradients within 2e-5 -- unstressed and at 10 sigma.  (The
    lower layer's bias gradient is not compared: BatchNorm removes the mean, it is zero but for rounding.)  Observed worst
    _rel on the MI355X, unstressed: dgamma 4.8e-7, dbeta 2.0e-7, dx 4.4e-7, dW 3.8e-7, dtab 1.5e-7, dwa 2.3e-7, dW2 4.1e-7;
    at 10 sigma: dgamma 5.1e-6, dbeta 2.4e-7, dx 5.1e-6, dW 4.9e-6, dtab 3.3e-6, dwa 3.4e-6, dW2 5.8e-6."""
    from pcr_amd import train_ops as TO
    inp = make_comp_input(low, stress)
    _comp_assert_input(inp, stress)
    policy = STREAM if low == "stream" else TILE
    c1 = inp["gamma"].numel()
    W2 = inp["W2"].cuda()

    def chain():
        y1, n1, _, _ = _comp_forward(inp, policy)
        Rrows = y1.shape[0] * y1.shape[2]
        with _policy(TILE):
            up = TO.tdense_bwd(inp["dy2"].cuda(), y1, COMP_C2, dy_mode=0, isc=n1["scale"], ish=n1["shift"], iinv=n1["inv_scale"],
                               in_relu=True, wpT=TO.pack_dev(W2, transpose=True), want_dstats=True)
        k1 = TO.bn_bwd_finalize(up["dstats"], up["dstats"].shape[0], c1, Rrows, inp["gamma"].cuda(), n1["mean"], n1["invstd"])
        out = dict(dgamma=k1["dgamma"], dbeta=k1["dbeta"], dW2=up["dW"])
        if low == "l1":
            B, N, S, K, _ = COMP_L1
            dtab, dwa_p = torch.empty(B, 2 * c1, N, device="cuda"), torch.empty(B, c1, 4, device="cuda")
            L.run.pcr_sa_l1_bwd_f32(inp["xyz"].cuda(), inp["idx"].cuda(), up["dx"], y1, k1["ka"], k1["kb"], k1["kc"], dtab, dwa_p,
                                    B, N, S, K, c1, L.stream_ptr())
            dwa4 = TO.reduce_parts(dwa_p, B, c1 * 4, c1, 4, 4)
            out.update(dtab=dtab, dwa=dwa4[:, :3].contiguous())
        else:
            with _policy(policy):
                lo = TO.tdense_bwd(up["dx"], inp["x"].cuda(), c1, dy_mode=1, y=y1, k=k1, isc=inp["isc"].cuda(),
                                   ish=inp["ish"].cuda(), iinv=(1.0 / inp["isc"]).cuda(), in_relu=True,
                                   wpT=TO.pack_dev(inp["W"].cuda(), transpose=True), want_dstats=True)
            out.update(dx=lo["dx"], dW=lo["dW"])
        return out
    runs = [chain() for _ in range(2)]
    _same(*runs)
    grads = _comp_bwd_want(inp)
    pairs = dict(dgamma="gamma", dbeta="beta", dW2="W2")
    pairs.update(dict(dtab="tab", dwa="wa") if low == "l1" else dict(dx="z0", dW="W"))
    worst = {k: _vs(runs[0][k], grads[v]) for k, v in pairs.items()}
    _report("comp_bwd", (low, stress), worst)
    assert max(worst.values()) < BN_BOUND, worst
