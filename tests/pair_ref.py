"""Float64 restatement of the pair head over embeddings (include/pcr.h, section A10; csrc/pair_kernels.hip), written two
ways -- `head_direct` on the gathered rows [e_i | e_j] with F.linear / F.group_norm, as the model's LinearRes + Linear do,
and `head_split` with the per-object tables u[i] + v[j] -- plus the inputs of tests/test_gpu_pair_head.py, the restated
shape rule and the planted faults of tests/test_pair_ref_cpu.py.  Test-only: nothing of the product imports this."""
import torch
import torch.nn.functional as F

BOUND = 2e-6         # bound (1) of tests/test_gpu_dense_forms.py: the project's f32 bound, err = max|got - ref| / max|ref|
EPS = 1e-5


def pair_head_ok(Fw, groups):
    """pcr_pair_head_ok restated: F in {32, 64, 128}, GroupNorm groups of 4 / 8 / 16 / 32 channels of n = 2F"""
    if Fw not in (32, 64, 128) or groups < 1 or (2 * Fw) % groups:
        return 0
    return int(2 * Fw // groups in (4, 8, 16, 32))


def make_inputs(Fw, groups, M, seed, scale=1.0, pooled="max"):
    """emb (M, F) = the maximum over 64 rows of randn, times `scale`; weights randn / sqrt(n); float32 tensors"""
    g = torch.Generator().manual_seed(seed)
    n = 2 * Fw
    raw = torch.randn(M, 64, Fw, generator=g)
    emb = (raw.amax(dim=1) if pooled == "max" else raw.mean(dim=1)) * scale
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(emb=emb.contiguous(), w1=r(n, n) / n ** 0.5, w2=r(n, n) / n ** 0.5,
                gn1_g=torch.rand(n, generator=g) + 0.5, gn1_b=r(n) * 0.5, gn2_g=torch.rand(n, generator=g) + 0.5,
                gn2_b=r(n) * 0.5, w_out=r(n) / n ** 0.5, b_out=r(1), groups=groups, F=Fw, n=n)


def make_pairs(M, P, seed):
    """(P, 2) int32 with i == j pairs and repeated pairs among them"""
    g = torch.Generator().manual_seed(1000 + seed)
    pairs = torch.randint(0, M, (P, 2), generator=g, dtype=torch.int32)
    if P >= 3:
        pairs[1, 1] = pairs[1, 0]            # i == j
        pairs[P - 1] = pairs[0]              # a repeated pair
    return pairs


def _d(t):
    return t.double()


def head_direct(inp, pairs, dtype=torch.float64):
    """LinearRes(n, n, GN) + Linear(n, 1) on x = [e_i | e_j] (lanegcn_nets.py:228-241, ReIDNet.py:455-458)"""
    c = lambda k: inp[k].to(dtype)
    i, j = pairs[:, 0].long(), pairs[:, 1].long()
    x = torch.cat([c("emb")[i], c("emb")[j]], dim=1)
    out = F.relu(F.group_norm(F.linear(x, c("w1")), inp["groups"], c("gn1_g"), c("gn1_b"), EPS))
    out = F.group_norm(F.linear(out, c("w2")), inp["groups"], c("gn2_g"), c("gn2_b"), EPS)
    out = F.relu(out + x)
    return F.linear(out, c("w_out").view(1, -1), c("b_out")).reshape(-1)


def tables(inp, dtype=torch.float64):
    emb, w1, Fw = inp["emb"].to(dtype), inp["w1"].to(dtype), inp["F"]
    return emb @ w1[:, :Fw].t(), emb @ w1[:, Fw:].t()


def _gn(x, groups, gamma, beta, shift=0):
    """GroupNorm over channel groups of every row, written out (biased variance); shift: the groups start `shift`
    channels late and the last one wraps (a planted fault)"""
    P, n = x.shape
    xs = torch.roll(x, -shift, dims=1).reshape(P, groups, n // groups)
    m = xs.mean(dim=2, keepdim=True)
    v = ((xs - m) ** 2).mean(dim=2, keepdim=True)
    y = torch.roll(((xs - m) / torch.sqrt(v + EPS)).reshape(P, n), shift, dims=1)
    return y * gamma + beta


def head_split(inp, pairs, dtype=torch.float64, fault=None):
    """the launch's form: z = relu(GN1(u[i] + v[j])); y = GN2(W2 z) + [e_i | e_j]; logit = w_out . relu(y) + b_out.
    fault: None, or one of FAULTS -- what a kernel with that slip would compute"""
    c = lambda k: inp[k].to(dtype)
    i, j = pairs[:, 0].long(), pairs[:, 1].long()
    u, v = tables(inp, dtype)
    if fault == "uv_swapped":
        u, v = v, u
    shift = 1 if fault == "groups_shifted" else 0
    emb = c("emb")
    res = torch.cat([emb[j], emb[i]], dim=1) if fault == "residual_swapped" else torch.cat([emb[i], emb[j]], dim=1)
    z = F.relu(_gn(u[i] + v[j], inp["groups"], c("gn1_g"), c("gn1_b"), shift))
    t = z @ c("w2").t()
    if fault == "residual_before_gn2":
        y = _gn(t + res, inp["groups"], c("gn2_g"), c("gn2_b"), shift)
    else:
        y = _gn(t, inp["groups"], c("gn2_g"), c("gn2_b"), shift) + res
    return F.relu(y) @ c("w_out") + c("b_out")


FAULTS = ("uv_swapped", "residual_before_gn2", "residual_swapped", "groups_shifted")     # + "mean_pooled": make_inputs(pooled="mean")


def err(got, ref):
    """max|got - ref| / max|ref|: the quantity BOUND is about"""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
