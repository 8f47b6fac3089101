"""CPU: the float64 references of tests/train_attn_ref.py against torch float64 autograd of the reference project's own
formulation (1e-12), kv_roll against an explicitly rolled copy, the first-index rule of the pair pool on constructed
ties, and -- for every row of the tables of test_gpu_train_attn_ops.py, imported from there so both files share them --
that the input builds, that a token-norm input with a ReLU conditions to ZERO marginal decisions within the moved-share
cap, and what every bound that rests on a float32-CPU yardstick comes to (printed).  Exact-arithmetic zeros are shown to
be what the GPU tests take them for, so none slips into a relative comparison."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_train_attn_ops as G
import train_attn_ref as R
from test_gpu_train_ops import _t_linattn

F64 = torch.float64
TIGHT = 1e-12


def _err(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _randn(*shape, seed=0, grad=True):
    t = torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))
    return t.requires_grad_(True) if grad else t


# ------------------------------------------------------------------------------------ linear attention --
@pytest.mark.parametrize("B,d,H,Lq,Sk", [(2, 8, 2, 5, 7), (1, 6, 1, 1, 1), (3, 16, 4, 9, 2), (2, 4, 4, 3, 3)])
def test_linattn_ref_is_the_reference_formulation(B, d, H, Lq, Sk):
    q, k, v = _randn(B, d, Lq, seed=1), _randn(B, d, Sk, seed=2), _randn(B, d, Sk, seed=3)
    go = _randn(B, d, Lq, seed=4, grad=False)
    want = _t_linattn(q, k, v, H, G.ATTN_EPS)
    out, A, ks = R.linattn_ref(q.detach(), k.detach(), v.detach(), H, G.ATTN_EPS)
    assert _err(out, want) < TIGHT
    dq, dk, dv, (t1, t2), (u1, u2) = R.linattn_bwd_ref(q.detach(), k.detach(), v.detach(), H, G.ATTN_EPS, go)
    for a, b in zip((dq, dk, dv), torch.autograd.grad(want, [q, k, v], go)):
        assert _err(a, b) < TIGHT
    assert torch.equal(dq, t1 + t2) and torch.equal(dk, u1 + u2)
    # the saved records are what the reference formulation sums: KV (with V / Sk) and K.sum
    Kp = (F.elu(k) + 1).reshape(B, H, d // H, Sk)
    assert _err(A, torch.einsum("bhis,bhvs->bhiv", Kp, v.reshape(B, H, d // H, Sk) / Sk)) < TIGHT
    assert _err(ks, Kp.sum(dim=3)) < TIGHT
    # and the backward on GIVEN records differentiates with them: perturbed records move every gradient
    dq2 = R.linattn_bwd_ref(q.detach(), k.detach(), v.detach(), H, G.ATTN_EPS, go, A=A, ks=ks)[0]
    assert torch.equal(dq2, dq)
    assert not torch.equal(R.linattn_bwd_ref(q.detach(), k.detach(), v.detach(), H, G.ATTN_EPS, go, A=A * 1.5, ks=ks)[0], dq)


@pytest.mark.parametrize("kv_roll", [1, -1, 2, 3])
def test_kv_roll_is_a_rolled_copy(kv_roll):
    B, d, H, Lq, Sk = 3, 8, 2, 5, 4
    q, k, v = (_randn(B, d, n, seed=s, grad=False) for n, s in ((Lq, 5), (Sk, 6), (Sk, 7)))
    go = _randn(B, d, Lq, seed=8, grad=False)
    kr, vr = torch.roll(k, -kv_roll, 0), torch.roll(v, -kv_roll, 0)         # kr[b] = k[(b + kv_roll) % B]
    assert torch.equal(kr[0], k[kv_roll % B])
    for a, b in zip(R.linattn_ref(q, k, v, H, G.ATTN_EPS, kv_roll), R.linattn_ref(q, kr, vr, H, G.ATTN_EPS)):
        assert torch.equal(a, b)
    dq, dk, dv = R.linattn_bwd_ref(q, k, v, H, G.ATTN_EPS, go, kv_roll)[:3]
    dq0, dk0, dv0 = R.linattn_bwd_ref(q, kr, vr, H, G.ATTN_EPS, go)[:3]
    assert torch.equal(dq, dq0)
    assert torch.equal(dk, torch.roll(dk0, kv_roll, 0)) and torch.equal(dv, torch.roll(dv0, kv_roll, 0))
    if kv_roll % B:
        assert not torch.equal(dk, dk0)


def test_dq_and_dk_with_one_key_are_cancellations():
    """Sk = 1: out = v a / (a + eps) with a = Q'.K' depends on q and k through a / (a + eps) alone.  At eps = 0 dq and dk
    are zero in exact arithmetic -- below 1e-12 of either cancelling term in float64 -- and at LinearAttention's eps = 1e-6
    dq is eps / (a + eps) of its terms: far below any float32 bound either way, so the GPU test holds both absolutely, on
    the scale of the terms.  With two keys or more neither is small."""
    for case in G.LIN_CASES:
        B, d, H, Lq, Sk = case
        inp = G.make_lin_input(case)
        q, k, v, go = (inp[n].to(F64) for n in ("q", "k", "v", "go"))
        scale = G.lin_want(case)["scale"]
        dq, dk = R.linattn_bwd_ref(q, k, v, H, G.ATTN_EPS, go)[:2]
        share = dict(dq=float(dq.abs().max()) / scale["dq"], dk=float(dk.abs().max()) / scale["dk"])
        if Sk > 1:
            assert min(share.values()) > 1e-3, (case, share)      # nothing else is a zero in disguise
            continue
        print(case, "max|dq| / max|term| = %.3g, max|dk| / max|term| = %.3g" % (share["dq"], share["dk"]))
        assert max(share.values()) < 1e-2 * G.BOUND
        dq0, dk0, _, (t1, t2), (u1, u2) = R.linattn_bwd_ref(q, k, v, H, 0.0, go)
        assert float(dq0.abs().max()) < 1e-12 * max(float(t1.abs().max()), float(t2.abs().max()))
        assert float(dk0.abs().max()) < 1e-12 * max(float(u1.abs().max()), float(u2.abs().max()))
        t1 = R.linattn_bwd_ref(q, k, v, H, G.ATTN_EPS, go)[3][0]
        a = torch.einsum("bhil,bhi->bhl", R._elu1(R._heads(q, H)), R._elu1(R._heads(k, H)).sum(dim=3))
        ratio = (dq.abs() / t1.abs()).reshape(B, H, d // H, Lq)
        expect = (G.ATTN_EPS / (a + G.ATTN_EPS)).unsqueeze(2).expand_as(ratio)
        assert float((ratio / expect - 1).abs().max()) < 1e-3        # (the float64 sum's own cancellation: 1e-16 / 1e-8 ...)
    assert sum(c[4] == 1 for c in G.LIN_CASES) >= 5


def test_linattn_tables_cover_what_they_claim():
    for dh in (32, 64):
        rows = [c for c in G.LIN_CASES if c[1] // c[2] == dh]
        assert {c[3] for c in rows} == {1, 32, 33, 64, 65, 130} and {c[4] for c in rows} == {1, 2, 31, 32, 33, 64, 65, 97}
    assert [(2, 32, 2, 65, 33), (3, 16, 1, 1, 2), (2, 32, 2, 64, 64)] == [c for c in G.LIN_CASES if c[1] // c[2] == 16]
    for d, H in ((256, 2), (128, 1)):
        rows = [c for c in G.LIN_CASES if c[1] == d and c[2] == H]
        assert {c[3] for c in rows} == {c[4] for c in rows} == {1, 15, 16, 17, 33}
    assert {c[1] // c[2] for c in G.ROLL_CASES} == {16, 32, 64, 128} and all(c[0] == 3 and c[3] == c[4] for c in G.ROLL_CASES)


@pytest.mark.parametrize("case", [c for c in G.LIN_CASES + G.ROLL_CASES if G.lin_yard(c)])
def test_linattn_yardsticks(case):
    """head width 128: the float32 CPU evaluation's error y32 per tensor, and the bound max(2e-5, 8 y32) it gives"""
    want = G.lin_want(case)
    for n, y32 in want["y32"].items():
        print(case, n, "y32 = %.3g -> bound %.3g" % (y32, G.lin_bound(case, want, n)))
        assert y32 < G.BOUND          # a yardstick worse than the project bound would say the formula is ill-conditioned here


# ------------------------------------------------------------------------------------------ token norm --
@pytest.mark.parametrize("B,C,Ln,G_", [(2, 12, 7, 1), (3, 12, 5, 3), (1, 8, 1, 2), (2, 4, 3, 4)])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_tnorm_ref_is_layernorm_or_groupnorm_on_the_rows(B, C, Ln, G_, res, relu):
    x, go = _randn(B, C, Ln, seed=11), _randn(B, C, Ln, seed=12, grad=False)
    r = _randn(B, C, Ln, seed=13) if res else None
    norm = (torch.nn.LayerNorm(C) if G_ == 1 else torch.nn.GroupNorm(G_, C)).to(F64)
    with torch.no_grad():
        norm.weight.copy_(_randn(C, seed=14, grad=False))
        norm.bias.copy_(_randn(C, seed=15, grad=False))
    t = norm(x.permute(0, 2, 1).reshape(B * Ln, C)).reshape(B, Ln, C).permute(0, 2, 1)
    t = t if r is None else t + r
    t = F.relu(t) if relu else t
    leaves = [x, norm.weight, norm.bias] + ([r] if res else [])
    want = torch.autograd.grad(t, leaves, go)
    args = (x.detach(), norm.weight.detach(), norm.bias.detach(), None if r is None else r.detach(), G_, norm.eps, relu)
    y, mean, rstd, z = R.tnorm_ref(*args)
    assert _err(y, t) < TIGHT
    xg = x.detach().reshape(B, G_, C // G_, Ln)
    assert _err(mean, xg.mean(dim=2)) < TIGHT and _err(rstd, 1 / torch.sqrt(xg.var(dim=2, unbiased=False) + norm.eps)) < TIGHT
    got = R.tnorm_bwd_ref(*args, go)
    for a, b in zip(got[:3] + ((got[3],) if res else ()), want):
        assert _err(a, b) < TIGHT
    assert (got[3] is None) == (not res)


def test_tnorm_tables_reach_every_plan():
    plans = {}
    for B, C, Ln, G_, res, relu, stress in G.TN_CASES:
        gs = C // G_
        plan = "four%d" % (gs // 4) if gs in (32, 64, 128, 256) else "generic"
        plans.setdefault(plan, []).append((B * Ln, gs, G_, res, relu, stress))
    assert set(plans) == {"four8", "four16", "four32", "four64", "generic"}
    assert all(any(r[5] for r in rows) for rows in plans.values())                       # one stressed row per plan
    assert any(r[2] > 1 for r in plans["four8"])                                         # four-wave with G > 1
    assert {r[1] for r in plans["generic"]} >= {16, 36, 6, 1}
    assert {r[0] for rows in plans.values() for r in rows} >= {63, 64, 65, 150, 70}
    for shape in ((3, 128, 50, 1), (3, 36, 50, 1)):                                      # res x relu in full
        assert {c[4:6] for c in G.TN_CASES if c[:4] == shape and not c[6]} == {(a, b) for a in (False, True) for b in (False, True)}


@pytest.mark.parametrize("case", G.TN_CASES)
def test_tnorm_inputs_condition_to_zero_marginals(case):
    B, C, Ln, G_, res, relu, stress = case
    inp = G.make_tn_input(case)
    assert inp["x"].dtype == torch.float32 and float(inp["gamma"][1]) == 0.0 and float(inp["gamma"][0]) < 0
    if relu:
        assert R.tnorm_marginals(inp["x"], inp["gamma"], inp["beta"], inp["res"], G_, G.NORM_EPS) == 0
        assert inp["moved"] <= G.MOVED_CAP * inp["x"].numel(), (inp["moved"], inp["x"].numel())
    else:
        assert inp["moved"] == 0
    x64 = inp["x"].to(F64).reshape(B, G_, C // G_, Ln)
    if stress:          # the stress survives conditioning: every token's group mean ~ 10 of its standard deviations
        ratio = x64.mean(dim=2).abs() / x64.std(dim=2, unbiased=False)
        assert float(ratio.min()) > 5.0
    want = G.tn_want(case)
    if "y32" in want:
        for n, y32 in want["y32"].items():
            print(case, n, "y32 = %.3g -> bound %.3g" % (y32, G.tn_bound(want, n)))
    if C == G_:         # a group of one: dx and dgamma are exact zeros in the reference; the GPU test holds them on these scales
        assert float(want["dx"].abs().max()) == 0.0 and float(want["dgamma"].abs().max()) == 0.0
        assert want["scale"]["dx"] > 1.0 and want["scale"]["dgamma"] > 1.0
        assert _err(want["rstd"], torch.full((B, G_, Ln), G.NORM_EPS ** -0.5, dtype=F64)) < TIGHT
    else:               # ... and nothing else that is compared relatively is a zero
        for n in ("y", "dx", "dgamma", "dbeta", "rstd"):
            assert float(want[n].abs().max()) > 1e-3, (case, n)


def test_condition_tnorm_moves_what_is_marginal_and_only_that():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 40, generator=g)
    gamma, beta = G._affine(8, g)
    res = torch.randn(2, 8, 40, generator=g)
    ref = lambda: R.tnorm_ref(x.to(F64), gamma.to(F64), beta.to(F64), res.to(F64), 2, G.NORM_EPS, True)     # noqa: E731
    res[0, 1, 3] -= float(ref()[3][0, 1, 3])   # gamma[1] = 0: only the residual can move this one
    res[1, 5, 7] = 0.0
    lo, hi = -20.0, 20.0                       # z rises with x[1, 5, 7] (gamma[5] > 0), from beta - 1.7 gamma to beta + 1.7 gamma
    for _ in range(60):                        # bisection: the token's statistics move with x
        x[1, 5, 7] = 0.5 * (lo + hi)
        lo, hi = (lo, 0.5 * (lo + hi)) if float(ref()[3][1, 5, 7]) > 0 else (0.5 * (lo + hi), hi)
    assert R.tnorm_marginals(x, gamma, beta, res, 2, G.NORM_EPS) >= 2
    x2, res2, moved = R.condition_tnorm(x, gamma, beta, res, 2, G.NORM_EPS)
    assert moved >= 2 and R.tnorm_marginals(x2, gamma, beta, res2, 2, G.NORM_EPS) == 0
    assert int((x2 != x).sum()) + int((res2 != res).sum()) <= moved
    assert x2[0, 1, 3] == x[0, 1, 3] and res2[0, 1, 3] != res[0, 1, 3]


# ------------------------------------------------------------------------------------- local attention --
@pytest.mark.parametrize("B,C,N,K,H", [(2, 8, 7, 3, 2), (1, 6, 5, 5, 3), (2, 4, 6, 1, 4)])
@pytest.mark.parametrize("variant", ["perm", "repeat", "self", "hub"])
def test_local_attn_ref_is_linear_attention_on_the_gathered_rows(B, C, N, K, H, variant):
    g = torch.Generator().manual_seed(C + K)
    if variant == "self":
        idx = torch.arange(N).view(1, N, 1).expand(B, N, K).contiguous()
    elif variant == "hub":
        idx = torch.arange(K).view(1, 1, K).expand(B, N, K).contiguous()
    else:
        idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(N)]) for _ in range(B)])
        if variant == "repeat" and K >= 2:
            idx[:, :, 1] = idx[:, :, 0]
    qkv, go = _randn(B, 3 * C, N, seed=21), _randn(B, C, N, seed=22, grad=False)
    rows = qkv.permute(0, 2, 1)
    nb = torch.gather(rows.unsqueeze(1).expand(-1, N, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, 3 * C))
    D = C // H
    Q = (F.elu(rows[..., :C]) + 1).reshape(B * N, 1, H, D)
    Kf = (F.elu(nb[..., C:2 * C]) + 1).reshape(B * N, K, H, D)
    V = nb[..., 2 * C:].reshape(B * N, K, H, D) / K
    KV = torch.einsum("nshd,nshv->nhdv", Kf, V)
    Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, Kf.sum(dim=1)) + G.ATTN_EPS)
    want = (torch.einsum("nlhd,nhdv,nlh->nlhv", Q, KV, Z) * K).reshape(B, N, C).permute(0, 2, 1)
    assert _err(R.local_attn_ref(qkv.detach(), idx.int(), H, G.ATTN_EPS), want) < TIGHT
    dqkv, edge, scale = R.local_attn_bwd_ref(qkv.detach(), idx.int(), H, G.ATTN_EPS, go)
    assert scale["dq"] >= float(dqkv[:, :C].abs().max()) / 2 and scale["dk"] >= float(dqkv[:, C:2 * C].abs().max()) / 2
    assert _err(dqkv, torch.autograd.grad(want, qkv, go)[0]) < TIGHT
    assert tuple(edge.shape) == (B, 2 * C, N, K)
    if variant == "hub" and K < N:
        assert bool((dqkv[:, C:, K:] == 0).all()) and bool((dqkv[:, C:, :K] != 0).any())


def test_local_attn_tables_build():
    assert len(G.LA_CASES) == 19 and G.LA_EDGE_CASE in G.LA_CASES
    for shape, variant in G.LA_CASES:
        B, C, N, K, H = shape
        inp = G.make_la_input(shape, variant)
        idx = inp["idx"]
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, N, K) and int(idx.min()) >= 0 and int(idx.max()) < N
        idle = G.la_uncited(shape, variant)
        if variant == "repeat":
            assert bool((idx[:, :, 0] == idx[:, :, 1]).all())
        if variant == "self":
            assert bool((idx == torch.arange(N).view(1, N, 1)).all()) and not bool(idle.any())
        if variant == "hub":
            assert int(idle.sum()) == B * (N - K)
def test_local_attn_gradients_with_one_neighbour_are_cancellations():
    """a row that lists ONE distinct neighbour (K = 1, or `self`) has msg_i = v_j a / (a + eps): dq and dk are eps-sized
    against the two parts of da that cancel -- far below any float32 bound -- and the GPU test holds them absolutely; with
    two distinct neighbours or more nothing that is compared relatively is small"""
    singles = 0
    for shape, variant in G.LA_CASES:
        B, C, N, K, H = shape
        want = G.la_want(shape, variant)
        share = dict(dq=float(want["dqkv"][:, :C].abs().max()) / want["scale"]["dq"],
                     dk=float(want["dqkv"][:, C:2 * C].abs().max()) / want["scale"]["dk"])
        assert float(want["msg"].abs().max()) > 1e-3 and float(want["dqkv"][:, 2 * C:].abs().max()) > 1e-3
        if G.la_one_neighbour(shape, variant):
            singles += 1
            assert K == 1 or variant == "self"
            print(shape, variant, "max|dq| / scale = %.3g, max|dk| / scale = %.3g" % (share["dq"], share["dk"]))
            assert max(share.values()) < G.BOUND       # (eps / (a + eps): largest at dh = 1, where a is one small product)
        else:
            assert min(share.values()) > 1e-3, (shape, variant, share)
    assert singles == 4 + 3          # `self` at the four shapes with K > 1, every variant of the K = 1 shape
    want = G.la_want(*G.LA_EDGE_CASE)
    assert float(want["edge"][:, :G.LA_EDGE_CASE[0][1]].abs().max()) > 1e-3 * want["scale"]["ek"]


# ------------------------------------------------------------------------------------------- pair pool --
@pytest.mark.parametrize("P,C,Ln", [(2, 3, 1), (3, 5, 70), (1, 1, 33)])
def test_pool_pair_ref_is_cat_max_mean(P, C, Ln):
    o, g = _randn(2 * P, C, Ln, seed=31), _randn(P, 2 * C, seed=32, grad=False)
    x = torch.cat([o[:P], o[P:]], dim=2)
    mx, targ = x.max(dim=2)
    want = torch.cat([mx, x.mean(dim=2)], dim=1)
    pooled, arg = R.pool_pair_ref(o.detach())
    assert _err(pooled, want) < TIGHT and torch.equal(arg, targ)
    assert _err(R.pool_pair_bwd_ref(g, arg, Ln), torch.autograd.grad(want, o, g)[0]) < TIGHT


def test_pair_pool_ties_go_to_the_first_index():
    o = torch.zeros(2, 4, 3, dtype=F64)
    o[0, 0] = torch.tensor([1.0, 5.0, 2.0])
    o[1, 0] = torch.tensor([5.0, 5.0, 0.0])           # the maximum in both halves: position 1, not 3 or 4
    o[0, 1] = torch.tensor([0.0, 1.0, 7.0])
    o[1, 1] = torch.tensor([7.0, 1.0, 0.0])           # at L - 1 and L: position 2
    o[0, 2] = o[1, 2] = torch.full((3,), -4.0)        # constant: position 0
    o[0, 3] = torch.tensor([0.0, 1.0, 2.0])
    o[1, 3] = torch.tensor([1.0, 9.0, 9.0])           # the second half only, twice: position 4
    pooled, arg = R.pool_pair_ref(o)
    assert arg.tolist() == [[1, 2, 0, 4]] and pooled[0, :4].tolist() == [5.0, 7.0, -4.0, 9.0]
    g = torch.tensor([[1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 6.0]], dtype=F64)
    d = R.pool_pair_bwd_ref(g, arg, 3)
    assert d[0, 0].tolist() == [0.0, 1.0, 0.0] and d[1, 0].tolist() == [0.0, 0.0, 0.0]
    assert d[0, 1].tolist() == [0.0, 0.0, 2.0] and d[1, 1].tolist() == [0.0, 0.0, 0.0]
    assert d[0, 2].tolist() == [3.0, 0.0, 0.0]
    assert d[0, 3].tolist() == [1.0, 1.0, 1.0] and d[1, 3].tolist() == [1.0, 5.0, 1.0]


@pytest.mark.parametrize("case", G.PP_CASES)
def test_pool_tables_plant_every_tie(case):
    P, C, Ln = case
    inp = G.make_pool_input(case)
    kinds = set(inp["kind"].flatten().tolist())
    assert kinds == {0, 1, 2, 3, 4}
    x = torch.cat([inp["o"][:P], inp["o"][P:]], dim=2)
    at_max = x == x.amax(dim=2, keepdim=True)
    k = inp["kind"]
    assert bool((at_max[k == 1].sum(dim=1) == 2).all()) and bool(at_max[k == 1][:, :Ln].any(dim=1).all())
    assert bool(at_max[k == 2][:, Ln - 1].all()) and bool(at_max[k == 2][:, Ln].all())
    assert bool(at_max[k == 3].all())
    assert not bool(at_max[k == 4][:, :Ln].any()) and bool((at_max[k == 4].sum(dim=1) == (2 if Ln > 1 else 1)).all())
    _, arg = R.pool_pair_ref(inp["o"].to(F64))
    planted = G.pool_planted_arg(case)
    assert torch.equal(arg[planted >= 0], planted[planted >= 0])
    # a last-index rule would answer differently on every planted row with two maxima
    last = 2 * Ln - 1 - R.first_argmax(x.flip(2), 2)
    assert bool((last[(k == 1) | (k == 2) | (k == 3)] != arg[(k == 1) | (k == 2) | (k == 3)]).all())


def test_pool_tables_cover_what_they_claim():
    assert {c[2] for c in G.PP_CASES} == {1, 31, 32, 33, 64, 65, 300} and {c[1] for c in G.PP_CASES} == {1, 5, 64}
    assert len(G.PP_CASES) == 21
