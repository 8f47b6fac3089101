"""CPU: the float64 restatement of the fused attention chains (tests/train_chain_ref.py) against torch float64 autograd of
the blocks' own formulation -- nn.Linear / nn.LayerNorm / ReLU composed as Tail._torch and Head._head_torch of
test_gpu_train_chain.py compose them, after the reference project's Self_Attention, FP_SA and corss_attention -- at 1e-12;
and, for every case test_gpu_train_chain_forms.py runs (built by the same `build_case`, so both files see the same
tensors): ZERO marginal ReLU decisions after conditioning, at most MOVED_CAP of the tokens touched, the yardsticks y32 and
ysplit (printed), and four planted faults, each of which at least one case of the list must catch."""
import pytest
import torch
import torch.nn as nn

import train_chain_ref as R

F64 = torch.float64
TIGHT = 1e-12


def _modules_tail(shape, p):
    d, c1, hid, out = shape
    merge = nn.Linear(d, d, bias=False)
    mlp = nn.Sequential(nn.Linear(c1 + d, hid, bias=False), nn.ReLU(True), nn.Linear(hid, out, bias=False))
    n1, n2 = nn.LayerNorm(d), nn.LayerNorm(out)
    mods = nn.ModuleList([merge, mlp, n1, n2]).double()
    with torch.no_grad():
        for t, k in ((merge.weight, "Wm"), (mlp[0].weight, "W0"), (mlp[2].weight, "W2"), (n1.weight, "g1"), (n1.bias, "b1"),
                     (n2.weight, "g2"), (n2.bias, "b2")):
            t.copy_(p[k])
    return mods, dict(Wm=merge.weight, W0=mlp[0].weight, W2=mlp[2].weight, g1=n1.weight, b1=n1.bias, g2=n2.weight, b2=n2.bias)


@pytest.mark.parametrize("shape,residual", R.TAIL_FORMS)
def test_tail_ref_is_the_blocks_formulation(shape, residual):
    case = R.build_case(("tail", (shape, residual), 3, 37, "plain"))
    (merge, mlp, n1, n2), params = _modules_tail(shape, case["p"])
    msg, res = case["msg"].to(F64).requires_grad_(True), case["res"].to(F64).requires_grad_(True)
    x = n1(merge(msg.permute(0, 2, 1)))
    y = n2(mlp(torch.cat([res.permute(0, 2, 1), x], dim=2)))
    if residual:
        y = y + res.permute(0, 2, 1)
    y = y.permute(0, 2, 1)
    names = ["dmsg", "dres"] + ["d" + k for k in params]
    auto = dict(zip(names, torch.autograd.grad(y, [msg, res] + list(params.values()), case["dout"].to(F64))))
    out, grads = R.evaluate(case)
    assert R.rel(out, y.detach()) < TIGHT
    assert set(grads) == set(auto)
    for k in auto:
        assert R.rel(grads[k], auto[k]) < TIGHT, k


@pytest.mark.parametrize("shape", R.HEAD_SHAPES)
def test_head_ref_is_the_blocks_formulation(shape):
    c, hd, d, n, src = shape
    case = R.build_case(("head", shape, 3, 37, "plain"))
    pos = nn.Sequential(nn.Linear(3, hd), nn.ReLU(True), nn.Linear(hd, c)).double()
    proj = nn.ModuleList([nn.Linear(c, d, bias=False) for _ in range(n)]).double()
    params = dict(P1=pos[0].weight, c1=pos[0].bias, P2=pos[2].weight, c2=pos[2].bias)
    params.update({"W_%d" % j: proj[j].weight for j in range(n)})
    with torch.no_grad():
        for k, t in params.items():
            t.copy_(case["p"][k])
    x = case["x"].to(F64).requires_grad_(True)
    xt = x.permute(0, 2, 1)
    fp = xt + pos(case["xyz"].to(F64).permute(0, 2, 1))
    y = torch.cat([pr(fp if (src >> j) & 1 else xt) for j, pr in enumerate(proj)], dim=2).permute(0, 2, 1)
    auto = dict(zip(["dx"] + ["d" + k for k in params], torch.autograd.grad(y, [x] + list(params.values()), case["dout"].to(F64))))
    out, grads = R.evaluate(case)
    assert R.rel(out, y.detach()) < TIGHT
    assert set(grads) == set(auto)
    for k in auto:
        assert R.rel(grads[k], auto[k]) < TIGHT, k


def test_the_plans_restated_here_are_the_ones_the_case_list_names():
    assert [s for s in R.TAIL_SHAPES if not R.tail_sep(s)] == [(64, 64, 128, 128)]
    occ2 = lambda lds: R.groups_cap(lds, 256) == 512                     # noqa: E731
    assert [s for s in R.TAIL_SHAPES if occ2(R.tail_lds(s))] == [(32, 32, 64, 32)]
    assert [s for s in R.HEAD_SHAPES if occ2(R.head_lds(s))] == [(32, 32, 32, 3, 7)]
    assert R.multi_tile_B(512) == 342 and 3 * 341 <= 2 * 512 < 3 * 342
    assert R.multi_tile_B(256) == 171 and 3 * 170 <= 2 * 256 < 3 * 171
    for kind, form, B, Ln, _ in R.multi_rows():
        lds = R.tail_lds(form[0]) if kind == "tail" else R.head_lds(form)
        assert Ln in (131, 132) and 3 * B > 2 * R.groups_cap(lds, R.NOMINAL_CUS)
    assert len(R.all_cases()) == len(set(R.all_cases()))
    # the position-independence layouts hold the same 384 tokens
    assert {B * Ln for B, Ln in R.POS_LAYOUTS} == {384}
    t = torch.arange(6 * 2 * 64.0).reshape(6, 2, 64)
    for B, Ln in R.POS_LAYOUTS:
        assert torch.equal(R.relayout(R.relayout(t, B, Ln), 6, 64), t)
    assert torch.equal(R.relayout(t, 3, 128)[1], torch.cat([t[2], t[3]], dim=1))


def _hidden(case):
    if case["kind"] == "tail":
        return R.tail_hidden(case["msg"], case["res"], case["p"])
    return R.head_hidden(case["xyz"], case["p"])


@pytest.mark.parametrize("key", R.all_cases(), ids=repr)
def test_every_case_conditions_to_zero_marginals_within_the_cap(key):
    case = R.build_case(key)
    h = _hidden(case)
    print(key, "touched %.4f of the tokens, %d passes, %d redrawn" % (case["share"], case["passes"], case["redrawn"]))
    assert R.marginals(h) == 0
    assert case["share"] <= R.MOVED_CAP
    assert all(v.dtype == torch.float32 for v in case.values() if isinstance(v, torch.Tensor))
    again = R.build_case(key)                                        # seeded from the key alone
    assert all(torch.equal(case[k], again[k]) for k in case if isinstance(case[k], torch.Tensor))
    if key[4] == "shut":                                             # closed on every token (a draw may add a unit of its own)
        shut = (h <= 0).all(dim=2).all(dim=0).nonzero().flatten().tolist()
        assert set(R.SHUT_ROWS) <= set(shut) and len(shut) <= len(R.SHUT_ROWS) + 2
    if key[4] == "stress":
        t = case["msg" if case["kind"] == "tail" else "x"]
        assert float((t.mean(dim=1) / t.std(dim=1)).min()) > 5.0
        if case["kind"] == "tail":
            assert float(case["p"]["g1"][3]) < -0.5 and float(case["p"]["g1"][7]) == 0.0


def test_conditioning_moves_one_element_per_token_and_pass():
    key = ("tail", ((64, 64, 128, 64), True), 3, 100, "plain")
    case = R.build_case(key)
    g = R._gen(key)
    r = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    p = R.tail_params(case["shape"], g)
    msg, res = r(3, 64, 100), r(3, 64, 100)
    assert torch.equal(msg, case["msg"]) and all(torch.equal(p[k], case["p"][k]) for k in p)
    moved = (res != case["res"])
    assert R.marginals(R.tail_hidden(msg, res, p)) > 0                 # the raw draw does have marginal elements
    assert int(moved.sum()) > 0 and int(moved.sum(dim=1).max()) <= max(1, case["passes"])
    assert float(moved.float().mean()) <= 0.0013                      # at most 0.13 % of the elements of res (c1 >= 32)


_SMALL = [k for k in R.all_cases() if k[2] <= 6]


@pytest.mark.parametrize("key", _SMALL, ids=repr)
def test_yardsticks(key):
    """y32 and ysplit of every small row.  8 y32 and the operand model itself must fit under the plain bounds, or no kernel
    could; a stress row gets its bound from these figures (train_chain_ref.bounds)"""
    case, want = R.reference(key)
    y = R.yardsticks(case, want)
    print(key, "y32 fwd %.3g grad %.3g" % y["y32"],
          " ".join("ysplit[%s] fwd %.3g grad %.3g" % ((a,) + y["ysplit"][a]) for a in y["ysplit"]))
    assert y["ysplit"]["bf16x3"][0] == 0.0                            # the f32 forward: nothing of it is split
    if key[4] != "stress":
        assert R.YARD * max(y["y32"]) < R.BOUNDS["f32"][0]            # 8 x the float32 yardstick is below the plain bound
        for a in R.ARITHS[1:]:
            assert y["ysplit"][a][0] < R.BOUNDS[a][0] and y["ysplit"][a][1] < R.BOUNDS[a][1], (a, y)
    else:
        print(key, "bounds", {a: R.bounds(a, y) for a in R.ARITHS})


@pytest.mark.parametrize("kind,form,B,Ln,ariths", R.multi_rows(), ids=repr)
def test_yardsticks_of_the_multi_tile_rows(kind, form, B, Ln, ariths):
    case, want = R.reference((kind, form, B, Ln, "plain"))
    y32 = R.compare(case, R.evaluate(case, torch.float32), want)[:2]
    ys = {a: R.compare(case, R.evaluate(case, F64, a), want)[:2] for a in ariths if a != "f32"}
    print(kind, form, B, Ln, "y32 fwd %.3g grad %.3g" % y32, ys)
    assert max(y32) < R.BOUNDS["f32"][0] / R.YARD
    for a, (f, g) in ys.items():
        assert f < R.BOUNDS[a][0] and g < R.BOUNDS[a][1]


# ---- negative controls: each planted fault must fail at least one case of the list --------------------------------------
@pytest.mark.parametrize("fault,kind", [("drop_last", "tail"), ("drop_last", "head"), ("pad_beta", "tail"),
                                        ("no_resid", "tail"), ("src_x", "head")])
def test_the_case_list_sees_each_planted_fault(fault, kind):
    caught, missed = [], []
    for key in [k for k in _SMALL if k[0] == kind and k[4] == "plain" and (k[2], k[3]) in R.EDGE_BL]:
        case, want = R.reference(key)
        fwd, grad, per = R.compare(case, R.evaluate(case, fault=fault), want)
        (caught if max(fwd, grad) > R.BOUNDS["f32"][1] else missed).append((key, max(per, key=per.get), max(fwd, grad)))
    print(fault, kind, "caught by %d cases, e.g. %s; not visible in %d" % (len(caught), caught[:2], len(missed)))
    assert caught
    keys = {k for k, _, _ in caught}
    if fault in ("drop_last", "pad_beta"):            # faults of a partial tile: every ragged L sees them, no whole one does
        assert {k[3] for k in keys} == {1, 63, 65, 100, 130} and {k[3] for k, _, _ in missed} == {64}
    if fault == "no_resid":                           # ... of the residual: every residual form, no other
        assert all(k[1][1] for k in keys) and not any(k[1][1] for k, _, _ in missed)
    if fault == "src_x":
        assert not missed
