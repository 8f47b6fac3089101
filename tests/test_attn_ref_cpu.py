"""CPU: the float64 attention reference of tests/attn_ref.py and the yardsticks of tests/test_gpu_attn_forms.py, proven
before a GPU is involved.  The rows are that file's own table, imported so both share one.

  * attn_ref (written from include/pcr.h: M, ksum, apply) equals oracle/model_oracle.py (the reference's order:
    projections, einsum attention, merge) evaluated in float64, to 1e-12 of the output's largest magnitude, on every row;
  * the index form equals explicit gathering, the pooled form the max / sum of the block output, exactly;
  * AttnPlan's host fold, reached without a device by handing the plan an identity in place of the weight packer: the
    block evaluated through the folded, once-rounded float32 matrices as pcr.h states the two launches (float64
    otherwise) stays within the row's float32 yardstick;
  * yardsticks: ysplit > 4 y32 on every row, so the f32 bound can see a phase computed in split bf16 (smallest ratio
    measured: see RATIOS);
  * the layout unpack_state reads M in is the host packers' (f32 and bf16 hi / lo images);
  * sensitivity: faults planted in the REFERENCE, never in a kernel, move the output beyond the f32 bound 4 y32 on every
    row they apply to -- (a) Self_Attention keys without the position term (not at Sk = 1, where the key cancels),
    (b) the value bias Wv b2 dropped, (c) key sums that count the padding of a ragged Sk, (d) the residual taken from
    the position-encoded features.  (e), the mean over Sk + 1 key tokens, CANNOT be seen in the output: norm1 cancels
    the scale Sk / (Sk + 1), only its eps = 1e-5 lets 0.04 to 0.9 of the bound through on the rows with Sk >= 24.  It is
    asserted against the bound on the state M instead, which test_gpu_attn_forms.py holds on the device.

RATIOS measured on this table (seeded weights, randn inputs): ysplit / y32 >= 11.3 (self-d128-h1-L256; 8.5 with the
features x 16), y32 = 1.0e-6 .. 3.1e-6, ysplit = 2.6e-5 .. 5.1e-5; host fold: at most 0.08 y32; smallest
fault / (4 y32): (a) 8390, (b) 17986, (c) 590 (cross-d64-h2-33x200), (d) 367189; (e) on M: 68 (self-d128-h4-L512).
"""
import pytest
import torch

import attn_ref as R
import test_gpu_attn_forms as G

F64 = torch.float64
ROWS = G.CASES + G.SPLIT_CASES + list(G.MANY.values())
IDS = [c.name for c in ROWS]


@pytest.mark.parametrize("case", ROWS, ids=IDS)
def test_reference_equals_the_oracle_in_float64(case):
    y = G.yardsticks(case)
    want = G.oracle_eval(case, y.data, F64)
    assert y.ref.dtype == F64 and y.ref.shape == want.shape
    assert float((y.ref - want).abs().max()) <= 1e-12 * float(want.abs().max())


def _flags(case):
    pos_name, q_pos, k_pos, residual = G.FLAGS[case.kind]
    return pos_name, q_pos, k_pos, residual


def _state(case, dt, mm=R.exact_mm):
    pos_name, _, k_pos, _ = _flags(case)
    return R.kv_state(dt.sd, pos_name, dt.fk, dt.xk, case.nhead, k_pos, mm=mm)


def _apply(case, dt, M, ksum, Sk=None, **kw):
    pos_name, q_pos, _, residual = _flags(case)
    return R.apply_block(dt.sd, pos_name, dt.fq, dt.xq if q_pos else None, M, ksum, case.Sk if Sk is None else Sk,
                         case.nhead, q_pos, residual, final=dt.final, kv_index=case.kv_index, q_index=case.q_index,
                         n_out=case.n_out, **kw)


@pytest.mark.parametrize("name", ["cross-reversed", "cross-gallery-L64", "cross-gallery-L33"])
def test_index_form_is_explicit_gathering(name):
    case = G.BY_NAME[name]
    y = G.yardsticks(case)
    dt = y.data
    n = case.n_out if case.n_out is not None else case.B
    qi = torch.tensor(case.q_index or tuple(range(n)))
    ki = torch.tensor(case.kv_index or tuple(range(n)))
    plain = R.cross_attention(dt.sd, dt.fq[qi], dt.xq[qi], dt.fk[ki], dt.xk[ki], case.nhead)
    assert torch.equal(y.ref, plain)
    # n_out cuts the list of virtual clouds
    M, ksum = _state(case, dt)
    head = R.apply_block(dt.sd, "pos_mlp", dt.fq, None, M, ksum, case.Sk, case.nhead, 0, 1, kv_index=ki, q_index=qi, n_out=2)
    assert torch.equal(head, plain[:2])


@pytest.mark.parametrize("name", ["cross-gallery-L64", "self-d32-h2-L45", "fp-3-64-64-32-f64-ragged"])
def test_pooled_is_max_and_sum_of_the_block_output(name):
    case = G.BY_NAME[name]
    y = G.yardsticks(case)
    pooled = G.ref_eval(case, y.data, pooled=True)
    assert pooled.shape == (y.ref.shape[0], 2, y.ref.shape[1])
    assert torch.equal(pooled[:, 0], y.ref.amax(dim=2)) and torch.equal(pooled[:, 1], y.ref.sum(dim=2))


# ------------------------------------------------------------------------------------------ host fold --
def _folded_plan(case, monkeypatch):
    """engine.AttnPlan built on the CPU from the module alone, with the MFMA weight packers replaced by the identity: its
    tensors are then the folded float32 matrices themselves"""
    from pcr_amd import engine
    as_matrix = lambda w, device: w.detach().reshape(w.shape[0], -1).to(torch.float32).clone()      # noqa: E731
    monkeypatch.setattr(engine, "pack_weight", as_matrix)
    monkeypatch.setattr(engine, "pack_weight_bf", as_matrix)
    m, conv = G.build_module(case)
    pos_name, q_pos, k_pos, residual = _flags(case)
    return engine.AttnPlan(m, pos_name, torch.device("cpu"), case.nhead, q_pos=q_pos, k_pos=k_pos, residual=residual,
                           final=conv)


def _folded_eval(case, plan, dt):
    """the two launches as include/pcr.h states them, on the plan's folded matrices, in float64"""
    t = {k: v.to(F64) for k, v in plan.t.items()}
    d, nhead, Sk = plan.d, plan.nhead, case.Sk
    dh = d // nhead
    hidden = lambda xyz: torch.relu(xyz.to(F64) @ t["pos0_w"].T + t["pos0_b"])      # noqa: E731
    tok = lambda f: f.to(F64).transpose(1, 2)      # noqa: E731
    # pcr_attn_kv_f32: one fused projection of [feat_k ; h]
    kvp = torch.cat([tok(dt.fk), hidden(dt.xk)], dim=2) @ t["wkv"].T + t["bkv"]
    K, V = torch.nn.functional.elu(kvp[..., :d]) + 1, kvp[..., d:] / Sk
    M = torch.zeros(K.shape[0], d, d, dtype=F64)
    for h in range(nhead):
        hs = slice(h * dh, (h + 1) * dh)
        KV = K[..., hs].transpose(1, 2) @ V[..., hs]                       # [dd][v]
        M[:, :, hs] = (KV @ t["wmerge"][:, hs].T).transpose(1, 2)          # M[o][dd]
    ksum = K.sum(dim=1)
    # pcr_attn_apply_f32
    n = case.n_out if case.n_out is not None else case.B
    qi = torch.tensor(case.q_index or tuple(range(n)))
    ki = torch.tensor(case.kv_index or tuple(range(n)))
    x = tok(dt.fq)[qi]
    xin = torch.cat([x, hidden(dt.xq[qi])], dim=2) if plan.q_pos else x
    Q = torch.nn.functional.elu(xin @ t["wq"].T + t["bq"]) + 1
    B, L, _ = Q.shape
    den = (Q * ksum[ki].unsqueeze(1)).view(B, L, nhead, dh).sum(-1, keepdim=True) + 1e-6
    Qn = (Q.view(B, L, nhead, dh) * Sk / den).reshape(B, L, d)
    ln = torch.nn.functional.layer_norm
    msg = ln(torch.einsum("bod,bld->blo", M[ki], Qn), (d,), t["ln1_g"], t["ln1_b"], 1e-5)
    ff = torch.relu(torch.cat([x, msg], dim=2) @ t["wmlp0"].T) @ t["wmlp2"].T
    out = ln(ff, (plan.cout,), t["ln2_g"], t["ln2_b"], 1e-5)
    if plan.residual:
        out = out + x
    if plan.cfinal:
        out = out @ t["wfinal"].T + t["bfinal"][:plan.cfinal]
    return out.transpose(1, 2)


@pytest.mark.parametrize("case", ROWS, ids=IDS)
def test_host_fold_stays_within_the_float32_yardstick(case, monkeypatch):
    y = G.yardsticks(case)
    plan = _folded_plan(case, monkeypatch)
    c1, c2, d, cout = case.dims
    assert plan.t["wq"].shape == (d, c1 + d if plan.q_pos else c1) and plan.t["wkv"].shape == (2 * d, c2 + d)
    assert plan.t["wq"].dtype == torch.float32 and plan.t["bkv"].shape == (2 * d,)
    err = float((_folded_eval(case, plan, y.data) - y.ref).abs().max())
    print("ATTN_FOLD %s err %.3e y32 %.3e" % (case.name, err, y.y32))
    assert err <= y.y32, (err, y.y32)


@pytest.mark.parametrize("d", [32, 64, 96, 128, 256])
def test_state_unpacking_inverts_the_host_packers(d):
    """unpack_state restates the layout the kv kernels write M in; the host packers build the same A-operand images"""
    from pcr_amd import engine
    W = torch.randn(d, d, generator=torch.Generator().manual_seed(d))
    tail = torch.arange(d, dtype=torch.float32)
    M, ksum = G.unpack_state(torch.cat([engine.pack_weight(W, "cpu"), tail]).unsqueeze(0), d, False)
    assert torch.equal(M[0], W.double()) and torch.equal(ksum[0], tail.double())
    if d <= 128:
        Mb, _ = G.unpack_state(torch.cat([engine.pack_weight_bf(W, "cpu"), tail]).unsqueeze(0), d, True)
        hi = W.to(torch.bfloat16)
        lo = (W - hi.float()).to(torch.bfloat16)
        assert torch.equal(Mb[0], hi.double() + lo.double())
        assert float((Mb[0] - W.double()).abs().max()) <= 2.0 ** -16 * float(W.abs().max())


# ------------------------------------------------------------------------------------------ yardsticks --
@pytest.mark.parametrize("case", ROWS, ids=IDS)
def test_split_yardstick_is_visible_to_the_f32_bound(case):
    y = G.yardsticks(case)
    print("ATTN_YARD %s y32 %.3e ysplit %.3e ratio %.1f max|out| %.2f"
          % (case.name, y.y32, y.ysplit, y.ysplit / y.y32, float(y.ref.abs().max())))
    assert y.y32 > 0 and y.ysplit > 4.0 * y.y32, (y.y32, y.ysplit)


@pytest.mark.parametrize("name", G.SCALE_CASES)
def test_yardsticks_follow_the_input_scale(name):
    case = G.BY_NAME[name]
    y = G.yardsticks(case, 16.0)
    print("ATTN_YARD %s[x16] y32 %.3e ysplit %.3e ratio %.1f max|out| %.2f"
          % (case.name, y.y32, y.ysplit, y.ysplit / y.y32, float(y.ref.abs().max())))
    assert torch.isfinite(y.ref).all() and y.ysplit > 4.0 * y.y32


# ------------------------------------------------------------------------------------------ sensitivity --
def _no_key_position(case, dt):
    """(a) Self_Attention keys without the position term"""
    M, ksum = R.kv_state(dt.sd, "pos_mlp", dt.fk, dt.xk, case.nhead, 0)
    return _apply(case, dt, M, ksum)


def _no_value_bias(case, dt):
    """(b) V without Wv b2: M loses sum_{v in head(dd)} Wm[o][v] ksum[dd] (Wv b2)[v] / Sk"""
    pos_name = _flags(case)[0]
    M, ksum = _state(case, dt)
    vb = dt.sd["v_proj.weight"].to(F64) @ dt.sd[pos_name + ".2.bias"].to(F64)
    Wm = dt.sd["merge.weight"].to(F64)
    d = vb.shape[0]
    dh = d // case.nhead
    Mb = torch.zeros_like(M)
    for h in range(case.nhead):
        hs = slice(h * dh, (h + 1) * dh)
        Mb[:, :, hs] = (Wm[:, hs] @ vb[hs]).view(1, d, 1) * ksum[:, hs].unsqueeze(1) / case.Sk
    return _apply(case, dt, M - Mb, ksum)


def _padded_key_sums(case, dt):
    """(c) ragged Sk: ksum also counts the padding up to the next multiple of 32, elu(0) + 1 = 1 per padded token"""
    M, ksum = _state(case, dt)
    return _apply(case, dt, M, ksum + float(-case.Sk % 32))


def _residual_from_encoded(case, dt):
    """(d) the residual taken from x + pos instead of x"""
    return G.ref_eval(case, dt) + R.pos_encoding(dt.sd, "pos_mlp", dt.xq).transpose(1, 2)


def _mean_over_sk_plus_one(case, dt):
    """(e) msg divided by Sk + 1 instead of Sk, as the block's OUTPUT shows it"""
    M, ksum = _state(case, dt)
    return _apply(case, dt, M * (case.Sk / (case.Sk + 1.0)), ksum)


FAULTS = {
    # (one key token: msg = V Sk (Q.K) / (Q.K + 1e-6) -- the key cancels, no fault in K can show)
    "a-keys-without-position": (_no_key_position, lambda c: c.kind == "self" and c.Sk > 1),
    "b-value-bias-dropped": (_no_value_bias, lambda c: True),
    "c-key-sums-count-padding": (_padded_key_sums, lambda c: c.Sk % 32 != 0),
    "d-residual-from-encoded": (_residual_from_encoded, lambda c: c.kind == "self"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_f32_bound_sees_planted_faults(fault):
    fn, applies = FAULTS[fault]
    rows = [c for c in ROWS if applies(c)]
    assert rows
    worst = None
    for case in rows:
        y = G.yardsticks(case)
        err = float((fn(case, y.data) - y.ref).abs().max())
        ratio = err / (4.0 * y.y32)
        print("ATTN_FAULT %s %s err %.3e bound %.3e ratio %.1f" % (fault, case.name, err, 4.0 * y.y32, ratio))
        if worst is None or ratio < worst[0]:
            worst = (ratio, case.name)
    print("ATTN_FAULT %s smallest ratio %.1f at %s" % ((fault,) + worst))
    assert worst[0] > 1.0, worst


def test_the_state_bound_sees_a_wrong_mean_over_the_key_tokens():
    """(e) V / (Sk + 1) scales M Q' by Sk / (Sk + 1) in front of norm1, and LayerNorm cancels a uniform scale: the block's
    output moves only through norm1's eps = 1e-5, by 0.04 to 0.9 of the f32 bound 4 y32 on every row with Sk >= 24 (above
    it only at Sk = 1, and at d = 32 with Sk <= 32: 1.2 to 6.2) -- NO bound on the output can see this fault, whatever the
    kernel.  It is visible where it happens: in M, which test_gpu_attn_forms.test_kv_state_against_float64 unpacks from
    the kv launch's image and holds to float64.  Asserted here: the fault moves M beyond that test's bound, in either
    arithmetic mode, on every row; the output figures are printed."""
    worst = None
    for case in ROWS:
        y, ys = G.yardsticks(case), G.state_yardsticks(case)
        out_err = float((_mean_over_sk_plus_one(case, y.data) - y.ref).abs().max())
        err = float(ys.M.abs().max()) / (case.Sk + 1.0)
        lim = max(G.state_bounds(ys, case, "f32")[0], G.state_bounds(ys, case, "bf16x3")[0])
        print("ATTN_FAULT e-mean-over-Sk-plus-1 %s output err / (4 y32) %.2f | M err %.3e bound %.3e ratio %.1f"
              % (case.name, out_err / (4.0 * y.y32), err, lim, err / lim))
        if worst is None or err / lim < worst[0]:
            worst = (err / lim, case.name)
    print("ATTN_FAULT e-mean-over-Sk-plus-1 smallest M ratio %.1f at %s" % worst)
    assert worst[0] > 1.0, worst
