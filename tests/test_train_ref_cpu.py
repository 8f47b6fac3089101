"""CPU: the float64 references of tests/train_ref.py against torch.nn / torch.autograd in float64 (1e-12 on tie-free
inputs), their first-index rule on constructed exact ties, and -- for every parametrised input of
test_gpu_train_pointwise_ops.py, imported from there so both files share one table -- that conditioning terminates
with ZERO marginal decisions.  The device tests' inputs are thereby known to be usable before a GPU is involved.  The
same for the grouped-MLP launches and the tables of test_gpu_train_sa_ops.py, with the cap on what conditioning may move."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_train_pointwise_ops as G
import test_gpu_train_sa_ops as S
import train_ref as R

F64 = torch.float64
TIGHT = 1e-12


def _err(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _randn(*shape, seed=0, grad=True):
    t = torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))
    return t.requires_grad_(True) if grad else t


def _layer(cls, C, gamma, beta, momentum):
    bn = cls(C, eps=G.EPS, momentum=momentum).to(F64).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.linspace(-1, 1, C))
        bn.running_var.copy_(torch.linspace(0.5, 2, C))
    return bn


@pytest.mark.parametrize("shape", [(4, 10, 33), (1, 6, 8), (3, 7, 1)])
@pytest.mark.parametrize("act", list(G.BN_ACTS))
@pytest.mark.parametrize("momentum", [0.1, 0.5])
def test_bn_act_ref_is_batchnorm1d(shape, act, momentum):
    B, C, Ln = shape
    on, slope = G.BN_ACTS[act]
    y, go = _randn(B, C, Ln, seed=1), _randn(B, C, Ln, seed=2, grad=False)
    gamma, beta = _randn(C, seed=3), _randn(C, seed=4)
    z, mean, unb = R.bn_act_ref(y, gamma, beta, G.EPS, on, slope)
    ours = [z] + list(torch.autograd.grad(z, [y, gamma, beta], go))
    bn = _layer(torch.nn.BatchNorm1d, C, gamma, beta, momentum)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y2 = y.detach().clone().requires_grad_(True)
    t = bn(y2)
    bn(y2)                                     # a second step on the running statistics
    t = F.leaky_relu(t, slope) if on else t
    want = [t] + list(torch.autograd.grad(t, [y2, bn.weight, bn.bias], go))
    for a, b in zip(ours, want):
        assert _err(a, b) < TIGHT
    assert _err(R.running_update(rm0, mean, momentum, 2), bn.running_mean) < TIGHT
    assert _err(R.running_update(rv0, unb, momentum, 2), bn.running_var) < TIGHT


@pytest.mark.parametrize("B,Co,N,K", [(2, 5, 12, 4), (1, 3, 9, 9), (2, 4, 6, 1)])
def test_edge_conv_ref_is_batchnorm2d_leaky_max(B, Co, N, K):
    tab, gp = _randn(B, 2 * Co, N, seed=5), _randn(B, Co, N, seed=6, grad=False)
    gamma, beta = _randn(Co, seed=7), _randn(Co, seed=8)
    idx = R.knn_ref(_randn(B, 3, N, seed=9, grad=False), K)
    assert bool((idx[:, :, 0].long() == torch.arange(N)).all())
    pooled, arg, mean, unb = R.edge_conv_ref(tab, idx, gamma, beta, G.EPS, G.SLOPE)
    ours = [pooled] + list(torch.autograd.grad(pooled, [tab, gamma, beta], gp))
    bn = _layer(torch.nn.BatchNorm2d, Co, gamma, beta, 0.1)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    tab2 = tab.detach().clone().requires_grad_(True)
    li = idx.long()
    nb = torch.gather(tab2[:, :Co].unsqueeze(2).expand(B, Co, N, N), 3, li.unsqueeze(1).expand(B, Co, N, K))
    t, targ = F.leaky_relu(bn(nb + tab2[:, Co:].unsqueeze(3)), G.SLOPE).max(dim=3)
    want = [t] + list(torch.autograd.grad(t, [tab2, bn.weight, bn.bias], gp))
    for a, b in zip(ours, want):
        assert _err(a, b) < TIGHT
    assert torch.equal(arg, targ)              # (tie-free input: any index rule agrees)
    assert _err(R.running_update(rm0, mean, 0.1), bn.running_mean) < TIGHT
    assert _err(R.running_update(rv0, unb, 0.1), bn.running_var) < TIGHT


@pytest.mark.parametrize("B,k,N", [(1, 1, 1), (3, 5, 17), (2, 64, 9)])
def test_bmm_ref_is_torch_bmm(B, k, N):
    x, T, g = _randn(B, k, N, seed=10), _randn(B, k, k, seed=11), _randn(B, k, N, seed=12, grad=False)
    want = torch.bmm(x.transpose(1, 2), T).transpose(1, 2)
    assert _err(R.bmm_ref(x, T), want) < TIGHT
    for a, b in zip(R.bmm_bwd_ref(x, T, g), torch.autograd.grad(want, [x, T], g)):
        assert _err(a, b) < TIGHT


@pytest.mark.parametrize("P,C,Ln", [(2, 3, 1), (3, 5, 70), (1, 1, 300)])
def test_pool_both_ref_is_max_and_mean(P, C, Ln):
    o, g = _randn(P, C, Ln, seed=13), _randn(P, 2 * C, seed=14, grad=False)
    mx, targ = o.max(dim=2)
    want = torch.cat([mx, o.mean(dim=2)], dim=1)
    pooled, arg = R.pool_both_ref(o.detach())
    assert _err(pooled, want) < TIGHT and torch.equal(arg, targ)
    assert _err(R.pool_both_bwd_ref(g, arg, Ln), torch.autograd.grad(want, o, g)[0]) < TIGHT


@pytest.mark.parametrize("B,C,Ln,W", [(2, 6, 5, 1), (2, 6, 5, 2), (1, 6, 7, 6), (2, 64, 3, 64)])
def test_channel_max_ref_is_maxpool1d(B, C, Ln, W):
    x, g = _randn(B, C, Ln, seed=15), _randn(B, C // W, Ln, seed=16, grad=False)
    want, targ = F.max_pool1d(x.permute(0, 2, 1), W, return_indices=True)
    want = want.permute(0, 2, 1)
    y, arg = R.channel_max_ref(x.detach(), W)
    assert _err(y, want) < TIGHT and torch.equal(arg, targ.permute(0, 2, 1))
    assert _err(R.channel_max_bwd_ref(g, arg, C), torch.autograd.grad(want, x, g)[0]) < TIGHT


def test_exact_ties_go_to_the_first_index():
    v = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0], [-2.0, -1.0, -3.0, -1.0, -1.0]], dtype=F64)
    assert R.first_argmax(v, 1).tolist() == [1, 0, 1]
    assert R.first_argmax(v.t().contiguous(), 0).tolist() == [1, 0, 1]
    # pooling: the maximum twice in a row, and a row of zeros
    pooled, arg = R.pool_both_ref(v.view(1, 3, 5))
    assert arg.tolist() == [[1, 0, 1]] and pooled[0, :3].tolist() == [3.0, 0.0, -1.0]
    g = torch.tensor([[1.0, 2.0, 3.0, 0.0, 0.0, 0.0]], dtype=F64)
    d = R.pool_both_bwd_ref(g, arg, 5)
    assert d[0].nonzero().tolist() == [[0, 1], [1, 0], [2, 1]]
    # channel windows: channels (0, 1) tie at point 0 -> channel 0; (2, 3) tie -> channel 2
    x = torch.tensor([[[5.0, 1.0], [5.0, 2.0], [-1.0, 0.0], [-1.0, 0.0]]], dtype=F64)
    y, arg = R.channel_max_ref(x, 2)
    assert arg.tolist() == [[[0, 1], [2, 2]]] and y.tolist() == [[[5.0, 2.0], [-1.0, 0.0]]]
    assert R.channel_max_bwd_ref(torch.ones(1, 2, 2, dtype=F64), arg, 4)[0].tolist() == [[1, 0], [0, 1], [1, 1], [0, 0]]
    # EdgeConv: neighbour 1 listed twice ahead of nothing larger -> the first listing takes the gradient; with a
    # negative gamma the smallest pre-activation wins, again at its first listing
    tab = torch.tensor([[[0.0, 4.0, 1.0], [0.0, 0.0, 0.0]]], dtype=F64).requires_grad_(True)      # Co = 1, N = 3
    idx = torch.tensor([[[0, 1, 1], [2, 1, 1], [2, 0, 0]]], dtype=torch.int32)
    for gamma, want in ((1.0, [[[1, 1, 0]]]), (-1.0, [[[0, 0, 1]]])):
        pooled, arg, _, _ = R.edge_conv_ref(tab, idx, torch.tensor([gamma], dtype=F64), torch.zeros(1, dtype=F64), G.EPS, 0.2)
        assert arg.tolist() == want


def test_conditioning_moves_marginal_elements_and_keeps_exact_ties():
    g = torch.Generator().manual_seed(0)
    y = torch.randn(4, 8, 50, generator=g)
    gamma, beta = G._affine(8, g)
    for _ in range(30):                        # plant z = 0 at one element (a fixed point: the element moves the statistics)
        y[1, 4, 7] = y[:, 4].mean() - beta[4] * torch.sqrt(y[:, 4].var(unbiased=False) + G.EPS) / gamma[4]
    assert R.marginal_signs(y, gamma, beta, G.EPS) >= 1
    y2, moved = R.condition_signs(y, gamma, beta, G.EPS)
    assert moved >= 1 and R.marginal_signs(y2, gamma, beta, G.EPS) == 0
    assert int((y2 != y).sum()) <= moved
    # EdgeConv: a near-tie is opened, a bit-equal tie (neighbour listed twice) stays
    tab = torch.randn(1, 4, 6, generator=g)
    idx = R.knn_ref(torch.randn(1, 3, 6, generator=g), 4).clone()
    idx[:, :, 3] = idx[:, :, 2]
    gam, bet = torch.tensor([1.0, -1.0]), torch.tensor([0.3, -0.2])
    tab[0, 0, idx[0, 0, 1].long()] = tab[0, 0, idx[0, 0, 0].long()] + 1e-6
    tab2, moved = R.condition_edge(tab, idx, gam, bet, G.EPS)
    assert moved >= 1 and R.edge_marginals(tab2, idx, gam, bet, G.EPS) == (0, 0)
    z = R.edge_pre(tab2.to(F64), idx)
    assert bool((z[..., 2] == z[..., 3]).all())


@pytest.mark.parametrize("shape,act,stress", [c for c in G.BN_CASES if G.BN_ACTS[c[1]][0]])
def test_every_bn_act_input_conditions_to_zero_marginal_signs(shape, act, stress):
    inp = G.make_bn_input(shape, act, stress)
    assert R.marginal_signs(inp["y"], inp["gamma"], inp["beta"], G.EPS) == 0
    assert inp["y"].dtype == torch.float32 and bool(torch.isfinite(inp["y"]).all())
    assert float(inp["gamma"][0]) < 0 and float(inp["gamma"][1]) == 0
    if stress:        # conditioning left the stressed element where it was put: 8 standard deviations out
        y = inp["y"].to(F64)
        assert float((y[0, 2, 0] - y[:, 2].mean()).abs() / y[:, 2].std()) > 6.0


@pytest.mark.parametrize("shape,variant", G.EDGE_CASES)
def test_every_edge_conv_input_conditions_to_zero_marginal_decisions(shape, variant):
    """(neighbour lists from the float64 kNN here, from the device's kNN in the GPU module: the same construction)"""
    inp = G.make_edge_input(shape, variant, R.knn_ref)
    assert R.edge_marginals(inp["tab"], inp["idx"], inp["gamma"], inp["beta"], G.EPS) == (0, 0)
    assert inp["tab"].dtype == torch.float32 and bool(torch.isfinite(inp["tab"]).all())
    if variant == "stress":
        y = R.edge_pre(inp["tab"].to(F64), inp["idx"])
        ratio = y.mean(dim=(0, 2, 3)).abs() / y.std(dim=(0, 2, 3))
        assert 9.0 < float(ratio.min()) and float(ratio.max()) < 11.5
    if variant in ("repeat", "dup") and shape[3] > 1:
        top = R.edge_pre(inp["tab"].to(F64), inp["idx"]).topk(2, dim=3).values
        assert int((top[..., 0] == top[..., 1]).sum()) > 0


def test_planted_pooling_inputs_hold_the_edges_they_claim():
    for P, C, Ln in G.POOL_CASES:
        o = G.make_pool_input(P, C, Ln)["o"].to(F64)
        _, arg = R.pool_both_ref(o)
        rows = o.view(P * C, Ln)
        if P * C >= 6:
            assert bool((rows[0] == 0).all()) and int(arg.view(-1)[1]) == 0 and int(arg.view(-1)[2]) == Ln - 1
            assert int(arg.view(-1)[3]) == Ln // 4 and float(rows[3, Ln - 1]) == float(rows[3].max())
            assert float(rows[4].max()) < 0
    for B, C, Ln, W in G.CMAX_CASES:
        x = G.make_cmax_input(B, C, Ln, W)["x"]
        assert tuple(x.shape) == (B, C, Ln) and x.is_contiguous()


# ============================================================================ grouped-MLP launches (SaEdgeTrain) --
@pytest.mark.parametrize("B,N,S_,K,D,c1", [(2, 12, 5, 4, 3, 6), (1, 9, 9, 9, 2, 5), (2, 7, 3, 1, 0, 4)])
def test_sa_l1_ref_is_the_first_conv_on_the_materialised_rows(B, N, S_, K, D, c1):
    """tables P = Wf f, Q = (Wc - Wf) f gathered by sa_l1_ref against the 1x1 conv [Wa | Wc | Wf] on the rows
    [dxyz, f_c, f_i - f_c] (the reference graph of test_gpu_train_ops._torch_sa): value and every gradient"""
    xyz, go = _randn(B, N, 3, seed=20, grad=False), _randn(B, c1, S_ * K, seed=21, grad=False)
    idx = torch.randint(0, N, (B, S_, K), generator=torch.Generator().manual_seed(22), dtype=torch.int32)
    w1, b1 = _randn(c1, 3 + 2 * D, seed=23), _randn(c1, seed=24)
    feats = _randn(B, D, N, seed=25) if D else None
    leaves = [w1, b1] + ([feats] if D else [])
    tab = None
    if D:
        wc, wf = w1[:, 3:3 + D], w1[:, 3 + D:]
        tab = torch.einsum("oc,bcn->bon", torch.cat([wf, wc - wf], dim=0), feats)
    ours = R.sa_l1_ref(xyz, idx, tab, w1[:, :3], b1)
    want = torch.einsum("oc,bcl->bol", w1, R.sa_l1_rows(xyz, feats, idx)) + b1.view(1, c1, 1)
    assert _err(ours, want) < TIGHT
    for a, b in zip(torch.autograd.grad(ours, leaves, go), torch.autograd.grad(want, leaves, go)):
        assert _err(a, b) < TIGHT
    if D:        # the centre half of the table takes no gradient beyond the S centres
        t = tab.detach().requires_grad_(True)
        dt, = torch.autograd.grad(R.sa_l1_ref(xyz, idx, t, w1[:, :3].detach(), b1.detach()), t, go)
        assert bool((dt[:, c1:, S_:] == 0).all()) and (S_ == N or bool((dt[:, :c1] != 0).any()))


@pytest.mark.parametrize("B,cin1,cin2,cout,Ln", [(3, 5, 0, 7, 11), (2, 4, 3, 6, 9), (1, 8, 0, 8, 33)])
def test_tdense_ref_mode_1_is_autograd_through_batchnorm(B, cin1, cin2, cout, Ln):
    """stats_ref -> bn_fwd_consts_ref -> (sums of the output gradient) -> bn_bwd_consts_ref -> tdense_dy(1) ->
    tdense_bwd_ref, against autograd through W f(x) + b -> nn.BatchNorm1d in float64; and the running update"""
    x, x2 = _randn(B, cin1, Ln, seed=30, grad=False), (_randn(B, cin2, Ln, seed=31) if cin2 else None)
    W, b = _randn(cout, cin1 + cin2, seed=32), _randn(cout, seed=33)
    isc, ish = _randn(cin1, seed=34, grad=False).abs() + 0.5, _randn(cin1, seed=35, grad=False)
    gamma, beta, go = _randn(cout, seed=36), _randn(cout, seed=37), _randn(B, cout, Ln, seed=38, grad=False)
    z0 = (isc.view(1, -1, 1) * x + ish.view(1, -1, 1)).requires_grad_(True)
    f = torch.relu(z0)
    y = torch.einsum("oc,bcl->bol", W, f if x2 is None else torch.cat([f, x2], dim=1)) + b.view(1, -1, 1)
    bn = _layer(torch.nn.BatchNorm1d, cout, gamma, beta, 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    leaves = [z0, W, b, bn.weight, bn.bias] + ([x2] if cin2 else [])
    want = torch.autograd.grad(bn(y), leaves, go)
    # the launches' route
    y_ = R.tdense_ref(x, x2, W, b, isc, ish, True, None, False).detach()
    assert _err(y_, y) < TIGHT
    Rn = B * Ln
    n = R.bn_fwd_consts_ref(R.stats_ref(y_).unsqueeze(0), cout, Rn, gamma.detach(), beta.detach(), G.EPS)
    assert _err(R.running_update(rm0, n["mean"], 0.5), bn.running_mean) < TIGHT
    assert _err(R.running_update(rv0, n["unbiased"], 0.5), bn.running_var) < TIGHT
    sums = torch.stack([go.sum(dim=(0, 2)), (go * y_).sum(dim=(0, 2))]).unsqueeze(0)
    k = R.bn_bwd_consts_ref(sums, cout, Rn, gamma.detach(), n["mean"], n["invstd"])
    r = R.tdense_bwd_ref(R.tdense_dy(1, go, y_, k), x, None if x2 is None else x2.detach(), W.detach(), isc, ish, True)
    ours = [r["dx"], r["dW"], r["db"], k["dgamma"], k["dbeta"]] + ([r["dx2"]] if cin2 else [])
    for a, w in zip(ours, want):
        assert _err(a, w) < 1e-11                 # (E[y^2] - mean^2 in float64: a few 1e-13 on these sizes)
    # the shifted / centred records describe the same constants
    off = n["mean"] + 0.3
    ys = y_ - off.view(1, -1, 1)
    n2 = R.bn_fwd_consts_ref(R.stats_ref(ys).unsqueeze(0), cout, Rn, gamma.detach(), beta.detach(), G.EPS, shift0=off)
    sums2 = torch.stack([go.sum(dim=(0, 2)), (go * ys).sum(dim=(0, 2))]).unsqueeze(0)
    k2 = R.bn_bwd_consts_ref(sums2, cout, Rn, gamma.detach(), n["mean"], n["invstd"], centre=off)
    assert max(_err(n2[q], n[q]) for q in n) < TIGHT and max(_err(k2[q], k[q]) for q in k) < 1e-11


def test_pool_and_route_refs_follow_the_first_index_rule():
    y = torch.tensor([[[1.0, 3.0, 3.0, -1.0, -2.0, -1.0, 0.5, 0.5, 0.5]]], dtype=F64)             # C = 1, S = 3, K = 3
    pooled, arg, ymax = R.sa_pool_ref(y, torch.tensor([1.0], dtype=F64), torch.tensor([0.0], dtype=F64), 3)
    assert pooled.tolist() == [[[3.0, 0.0, 0.5]]] and arg.tolist() == [[[1, 0, 0]]] and ymax.tolist() == [[[3.0, -1.0, 0.5]]]
    pooled, arg, ymax = R.sa_pool_ref(y, torch.tensor([-1.0], dtype=F64), torch.tensor([0.0], dtype=F64), 3)
    assert pooled.tolist() == [[[0.0, 2.0, 0.0]]] and arg.tolist() == [[[0, 1, 0]]] and ymax[0, 0, 1] == -2.0
    gp = torch.tensor([[[5.0, 6.0, 7.0]]], dtype=F64)
    gz, s = R.pool_bwd_stats_ref(gp, pooled, ymax)
    assert gz.tolist() == [[[0.0, 6.0, 0.0]]] and s.tolist() == [[6.0], [-12.0]]
    assert R.route_ref(gp, arg, pooled, 3).tolist() == [[[0, 0, 0, 0, 6.0, 0, 0, 0, 0]]]
    assert R.route_ref(gz, arg, None, 3).tolist() == [[[0, 0, 0, 0, 6.0, 0, 0, 0, 0]]]


def _within_cap(inp):
    assert inp["moved"] <= S.MOVE_CAP * inp["total"], (inp["moved"], inp["total"])


@pytest.mark.parametrize("shape,flags", S.FWD_CASES + [((B, ci, 0, co, Ln), "bn") for B, ci, co, Ln in S.STREAM_FWD])
def test_every_tdense_fwd_input_conditions_to_zero_marginal_decisions(shape, flags):
    inp = S.make_fwd_input(shape, flags)
    assert S.fwd_marginals(inp) == 0
    _within_cap(inp)
    assert all(t is None or (t.dtype == torch.float32 and bool(torch.isfinite(t).all())) for t in (inp["x"], inp["res"]))


BWD_INPUTS = sorted({(s, m, K) for s, m, _ in S.BWD_CASES for K in (S.bwd_ks(s) if m == 3 else [0])} |
                    {((B, c, 0, c, S_ * K), m, K if m == 3 else 0) for B, c, S_, K, m in S.STREAM_BWD})


@pytest.mark.parametrize("shape,mode,K", BWD_INPUTS)
def test_every_tdense_bwd_input_conditions_to_zero_marginal_decisions(shape, mode, K):
    inp = S.make_bwd_input(shape, mode, K)
    assert R.relu_arg_marginals(inp["x"], inp["isc"], inp["ish"]) == 0
    _within_cap(inp)
    if mode == 2:
        assert int((inp["y"] == 0).sum()) > 0
    if mode == 3:
        assert inp["S"] * K == shape[4] and int(inp["argmax"].max()) < K


@pytest.mark.parametrize("shape", S.POOL_CASES)
def test_every_pooling_input_conditions_to_zero_marginal_decisions(shape):
    B, C, S_, K = shape
    inp = S.make_pool_input(shape)
    assert R.pool_marginals(inp["y"], inp["scale"], inp["shift"], K) == (0, 0)
    _within_cap(inp)
    assert float(inp["scale"][0]) < 0 and float(inp["scale"][1]) == 0
    # the planted edges are there: closed rows, open rows, and (K > 1) exact ties at the top of open rows
    pooled, arg, _ = R.sa_pool_ref(inp["y"].to(F64), inp["scale"].to(F64), inp["shift"].to(F64), K)
    assert bool((pooled > 0).any()) and bool((pooled == 0).any())
    if K > 1:
        z = inp["scale"].to(F64).view(1, C, 1, 1) * inp["y"].to(F64).view(B, C, S_, K) + inp["shift"].to(F64).view(1, C, 1, 1)
        top = z.topk(2, dim=3).values
        assert int(((top[..., 0] == top[..., 1]) & (top[..., 0] > 0)).sum()) > 0
        assert int((arg == K - 1).sum()) > 0 and int((arg == 0).sum()) > 0


@pytest.mark.parametrize("low,stress", S.COMP_CASES)
def test_every_composition_input_conditions_to_zero_marginal_decisions(low, stress):
    inp = S.make_comp_input(low, stress)
    assert S.comp_marginals(inp) == 0
    _within_cap(inp)
    assert inp["changed"] <= (1 if low == "l1" else S.COMP_DENSE[1]) * inp["moved"]
    ratio = S._ratio(S.comp_lower_ref(inp))
    if stress != "none":
        assert 9.0 < float(ratio.min()) and float(ratio.max()) < 11.5
    else:
        assert float(ratio.max()) < 5.0
