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
  * the dispatch (library built, no device): the form the library reports for a block (pcr_attn_launch_form) equals the
    restatement attn_ref.kv_form / apply_form over a grid of shapes, modes, operand sets and the gate (630 180 kv and
    2 545 344 apply blocks; nothing disagreed); every entry of the GPU file's table of kernels, and of
    test_gpu_match_live.py's gated tables, is what the library reports for the block engine.AttnPlan builds; every
    instantiation the restatement can reach has an entry; a gated query gives the un-gated form with gated = 1 exactly
    where pcr_attn_live_ok says yes; the query refuses what the launches refuse;
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


# ------------------------------------------------------------------------------------------ the dispatch --
# The library's own report of what it would launch (pcr_attn_launch_form: the dispatcher's plan, no device) against the
# restatement attn_ref.kv_form / apply_form, the GPU file's table, and the gate.
D_MODEL, C1, C2, COUT, CFINAL = (32, 64, 96, 128, 256, 512), (3, 16, 32, 64, 128), (32, 64, 128), (32, 64, 128, 160), (0, 32, 64, 128)
NHEAD, TOKENS, SPLITS = (1, 2, 3, 4, 8), (1, 31, 32, 64, 96, 128, 160, 255, 256, 512, 1024), (0, 2, 3, 65)
_REQUIRED = ("feat_q", "feat_k", "xyz_k", "kv", "pos0_w", "pos0_b", "wq", "bq", "wkv", "bkv", "wmerge", "wmlp0", "wmlp2",
             "ln1_g", "ln1_b", "ln2_g", "ln2_b")
_OPTIONAL = ("xyz_q", "wfinal", "bfinal") + R.WIDE_IMAGES + R.BF_IMAGES + ("wmlp0_bf_xpad", "kv_part", "out", "pool_out")
_INTS = ("B", "Lq", "Sk", "c1", "c2", "d", "cout", "nhead", "q_pos", "residual", "cfinal", "kv_splits", "precision")
_ALWAYS = frozenset(("xyz_q", "wfinal", "bfinal", "kv_part") + R.WIDE_IMAGES)      # given whether or not the shape reads them


class _Query:
    """one reused parameter block and form buffer: ask(block, apply, gated) -> the reported attn_ref form, or None"""

    def __init__(self):
        import ctypes
        from pcr_amd import _lib, abi
        self.fn = _lib.load().pcr_attn_launch_form
        self.p, self.form = abi.AttnParams(), (ctypes.c_int * 16)()
        self.live = abi.LiveParams()
        self.live.count, self.live.period, self.live.offset = G._DUMMY, 11, 0
        self.pref, self.lref = ctypes.byref(self.p), ctypes.byref(self.live)
        for k in _REQUIRED:
            setattr(self.p, k, G._DUMMY)
        self.has = None
        self.asked = 0

    def ask(self, b, apply, gated):
        p = self.p
        if b.has is not self.has:
            for k in _OPTIONAL:
                setattr(p, k, G._DUMMY if k in b.has else None)
            self.has = b.has
        for k in _INTS:
            setattr(p, k, getattr(b, k))
        self.form[1] = -7
        status = self.fn(self.pref, self.lref if gated else None, apply, self.form)
        self.asked += 1
        if status != 0:
            assert status == 1 and self.form[1] == -7          # refused, form untouched
            return None
        return R.from_library(self.form[:], apply)


def _shapes():
    """every (d, c1, c2, cout, cfinal, q_pos, residual, nhead) of the grid, refused ones included"""
    import itertools
    return itertools.product(D_MODEL, C1, C2, COUT, CFINAL, (0, 1), (0, 1), NHEAD)


def test_the_library_reports_the_kv_form_the_restatement_names():
    """pcr_attn_launch_form(apply = 0) == attn_ref.kv_form.  Axes: every shape of `_shapes` x precision x {every bf16
    image, none} x gated.  Pruned -- Lq, wmlp0_bf_xpad and pool_out, which the kv side does not read; and, because c1, cout,
    cfinal, q_pos and residual reach the kv side only through the validity rule, the choice of the unit and the gate: a
    shape the validity rule refuses is asked at one (Sk, kv_splits); a valid one at two, and over the whole
    TOKENS x SPLITS product where its (c1, cout, cfinal, q_pos, residual) is one of five tuples (plain, residual,
    self-attention, the c1 = 3 block with a conv, the widest block).  FOUND on the way: nothing disagreed."""
    import itertools
    q = _Query()
    variants = [frozenset(_ALWAYS | {"out"} | (set(R.BF_IMAGES) if bf else set())) for bf in (0, 1)]
    everywhere = list(itertools.product(TOKENS, SPLITS))
    for d, c1, c2, cout, cfinal, q_pos, residual, nhead in _shapes():
        b = R.Block(d=d, c1=c1, c2=c2, cout=cout, cfinal=cfinal, q_pos=q_pos, residual=residual, nhead=nhead, has=variants[0])
        full = (c1, cout, cfinal, q_pos, residual) in ((64, 64, 0, 0, 0), (c2, c2, 0, 0, 1), (d, d, 0, 1, 1), (3, 32, 64, 0, 0),
                                                       (128, 160, 128, 0, 0))
        points = everywhere if full else ([(32, 0), (255, 2)] if R.block_valid(b) else [(32, 0)])
        for has in variants:
            b.has = has
            for b.precision in (0, 1, 2):
                for b.Sk, b.kv_splits in points:
                    for gated in (False, True):
                        assert q.ask(b, 0, gated) == R.kv_form(b, gated), (d, c1, c2, cout, cfinal, q_pos, residual, nhead,
                                                                            b.Sk, b.kv_splits, b.precision, sorted(has), gated)
    print("ATTN_DISPATCH kv: %d blocks compared" % q.asked)
    assert q.asked > 500000


def test_the_library_reports_the_apply_form_the_restatement_names():
    """pcr_attn_launch_form(apply = 1) == attn_ref.apply_form.  Axes: every shape of `_shapes` x Lq x precision x {every
    bf16 image, none} x pooled x gated.  Pruned -- Sk, which the apply side does not read; wmlp0_bf_xpad, read for c1 < 16
    only, is toggled there and given elsewhere; kv_splits, read by the gate only, is 0, and 2 at one gated point per shape;
    c2, read by the validity rule (q_pos) and the gate only: a valid shape with c2 != min(d, 128) is asked at two Lq, as
    is every shape the validity rule refuses.  FOUND on the way: nothing disagreed."""
    q = _Query()
    variants = {}
    for bf in (0, 1):
        for xpad in (0, 1):
            for pooled in (0, 1):
                variants[bf, xpad, pooled] = frozenset(_ALWAYS | {"pool_out" if pooled else "out"} |
                                                       (set(R.BF_IMAGES) if bf else set()) | ({"wmlp0_bf_xpad"} if xpad else set()))
    for d, c1, c2, cout, cfinal, q_pos, residual, nhead in _shapes():
        b = R.Block(d=d, c1=c1, c2=c2, cout=cout, cfinal=cfinal, q_pos=q_pos, residual=residual, nhead=nhead,
                    has=variants[0, 1, 0])
        lqs = TOKENS if R.block_valid(b) and c2 == min(d, 128) else (64, 255)
        for (bf, xpad, pooled), has in variants.items():
            if not xpad and c1 >= 16:
                continue
            b.has = has
            for b.precision in (0, 1, 2):
                for b.Lq in lqs:
                    for gated in (False, True):
                        assert q.ask(b, 1, gated) == R.apply_form(b, gated), (d, c1, c2, cout, cfinal, q_pos, residual, nhead,
                                                                               b.Lq, b.precision, sorted(has), gated)
                b.kv_splits = 2
                assert q.ask(b, 1, True) is None and R.apply_form(b, True) is None
                b.kv_splits = 0
    print("ATTN_DISPATCH apply: %d blocks compared" % q.asked)
    assert q.asked > 500000


def test_the_library_reports_every_row_of_the_gpu_file():
    """the block engine.AttnPlan builds for a row on the CPU gets the kernels the table names, in both modes; and the table
    has a row for every case the GPU file runs"""
    plans = {}
    for key, case, prec, splits, pooled in G.table_rows():
        plan = plans.setdefault(case.name, G.host_plan(case))
        kv, ap = G.host_blocks(plan, case, prec, splits=splits, pooled=pooled)
        assert (G.reported(kv, 0)[0], G.reported(ap, 1)[0]) == G.expect(key, prec), (key, prec)
    for case in ROWS:
        assert case.name in G.EXPECT or all(case.name + "[splits=%d]" % ns in G.EXPECT for ns in (2, 3)), case.name
    assert all(n + "[pooled]" in G.EXPECT for n in G.POOL_CASES + [G.MANY["cross"].name])


def test_the_library_reports_every_gated_row_of_the_match_live_file():
    import ctypes
    import test_gpu_match_live as ML
    from pcr_amd import abi
    live = abi.LiveParams()
    live.count, live.period, live.offset = G._DUMMY, ML.PERIOD, 3
    lv = ctypes.byref(live)
    rows = [(("cross", 2, 0, Ln, prec), want, True) for (Ln, prec), want in ML.GATED.items()]
    for (kind, nhead, cfinal, Ln, prec), want, with_pooled in rows + [(k, v, False) for k, v in ML.TWINS.items()]:
        case = ML.gated_case(kind, nhead, cfinal, Ln)
        plan = G.host_plan(case)
        kv, ap = G.host_blocks(plan, case, prec)
        assert (G.reported(kv, 0, lv)[0], G.reported(ap, 1, lv)[0]) == want[:2], (case.name, prec)
        if with_pooled:
            assert G.reported(G.host_blocks(plan, case, prec, pooled=True)[1], 1, lv)[0] == want[2], (case.name, prec)


def test_every_reachable_instantiation_has_a_row():
    """every (family, template arguments, gated) the restatement reaches over the grid with the operands AttnPlan builds
    (attn_ref.images_of_plan; pooled where pool_ok says yes) is the kernel of a table entry or, gated, of a row of
    tests/test_gpu_match_live.py"""
    import test_gpu_match_live as ML
    reach = set()
    for d, c1, c2, cout, cfinal, q_pos, residual, nhead in _shapes():
        has = R.images_of_plan(d, c1, c2, nhead, q_pos, cfinal)
        b = R.Block(d=d, c1=c1, c2=c2, cout=cout, cfinal=cfinal, q_pos=q_pos, residual=residual, nhead=nhead, has=has)
        if not R.block_valid(b):
            continue
        for b.precision in (0, 1):
            for tok in TOKENS:
                b.Lq = b.Sk = tok
                for gated in (False, True):
                    for b.kv_splits in ((0, 2) if not gated else (0,)):
                        b.has = has | {"kv_part"}
                        f = R.kv_form(b, gated)
                        reach.add(R.kernel_name(f) if f else None)
                    b.kv_splits = 0
                    for pooled in (False, True):
                        b.has = (has - {"out"}) | {"pool_out"} if pooled else has
                        f = R.apply_form(b, gated) if not pooled or R.pool_ok(b) else None
                        reach.add(R.kernel_name(f) if f else None)
    reach.discard(None)
    rows = {k for pair in G.EXPECT.values() for mode in pair for k in mode if k}
    rows |= {k for v in list(ML.GATED.values()) + list(ML.TWINS.values()) for k in v if k}
    assert reach <= rows, sorted(reach - rows)
    print("ATTN_DISPATCH %d instantiations reachable, %d kernels in the tables" % (len(reach), len(rows)))


def test_gated_queries_report_the_ungated_form_or_refuse():
    """where pcr_attn_live_ok says 1 the gated query returns the un-gated form with gated = 1 on both sides, pooled apply
    included; where it says 0 it refuses"""
    import ctypes
    from pcr_amd import _lib
    q = _Query()
    live_ok = _lib.load().pcr_attn_live_ok
    n_ok = 0
    for d, c1, c2, cout, cfinal, q_pos, residual, nhead in _shapes():
        if 64 not in (d, c1, c2, cout) and (d, nhead) != (128, 2):
            continue                                  # (far from the gate: one family of refusals is kept)
        base = R.images_of_plan(d, c1, c2, nhead, q_pos, cfinal) | {"kv_part"}
        b = R.Block(d=d, c1=c1, c2=c2, cout=cout, cfinal=cfinal, q_pos=q_pos, residual=residual, nhead=nhead, has=base)
        for b.precision in (0, 1):
            for tok in (32, 48, 160):
                b.Lq = b.Sk = tok
                for b.kv_splits in (0, 1, 2):
                    for pooled in (False, True):
                        b.has = (base - {"out"}) | {"pool_out"} if pooled else base
                        plain = [q.ask(b, side, False) for side in (0, 1)]
                        gated = [q.ask(b, side, True) for side in (0, 1)]
                        if live_ok(ctypes.byref(q.p)):
                            n_ok += 1
                            assert R.live_ok(b)
                            for u, g in zip(plain, gated):
                                assert (u is None and g is None) or (g[3] == 1 and g[:3] + (0,) + g[4:] == u), (u, g)
                            assert plain[0] is not None and gated[0] is not None
                        else:
                            assert not R.live_ok(b) and gated == [None, None]
    assert n_ok >= 2 * 3 * 2 * 2 * 4 * 4


def test_the_form_query_refuses_what_the_launches_refuse():
    import ctypes
    from pcr_amd import _lib
    lib = _lib.load()
    form = (ctypes.c_int * 16)()
    case = G.SPLIT_CASES[1]                           # cross-d64-h2-33x200
    plan = G.host_plan(case)
    kv, ap = G.host_blocks(plan, case, "bf16x3", splits=2)
    for side in (0, 1):
        assert lib.pcr_attn_launch_form(None, None, side, form) == 1
        assert lib.pcr_attn_launch_form(ctypes.byref(kv), None, side, None) == 1
    assert G.reported(kv, 0)[0] == G._KO3 and G.reported(ap, 1)[0] == G._AT21
    kv.kv_part = None                                 # a token split without its workspace
    assert G.reported(kv, 0) == (None, None)
    kv.kv_splits = 1
    assert G.reported(kv, 0)[0] == G._KO3
    kv.kv_splits, kv.kv_part = 65, G._DUMMY           # more than 64 splits
    assert G.reported(kv, 0) == (None, None)
    ap.pool_out = G._DUMMY                            # pooled output where pool_ok says no (Lq = 33)
    assert not lib.pcr_attn_apply_pool_ok(ctypes.byref(ap)) and G.reported(ap, 1) == (None, None)
    ap.pool_out = ap.out = None                       # no output at all
    assert G.reported(ap, 1) == (None, None)
    ap.out = G._DUMMY
    ap.B = 65536                                      # the apply grid's y
    assert G.reported(ap, 1) == (None, None)
    ap.B = 0                                          # an empty launch reports its plan
    assert G.reported(ap, 1)[0] == G._AT21
    wide = G.BY_NAME["self-d256-h2-L40"]
    kvw, _ = G.host_blocks(G.host_plan(wide), wide, "f32")
    assert G.reported(kvw, 0)[0] == G._KW2
    kvw.B = 65536                                     # the wide kv grid's y
    assert G.reported(kvw, 0) == (None, None)
    kvw.B, kvw.wkv_wide = 2, None                     # the wide images
    assert G.reported(kvw, 0) == (None, None)
    from pcr_amd import abi
    live = abi.LiveParams()                           # a gate without a count, and a gate on a shape it does not cover
    live.period = 11
    kv64, _ = G.host_blocks(G.host_plan(G.BY_NAME["cross-reversed"]), G.BY_NAME["cross-reversed"], "bf16x3")
    assert G.reported(kv64, 0, ctypes.byref(live)) == (None, None)
    live.count = G._DUMMY
    assert G.reported(kv64, 0, ctypes.byref(live))[0] == "attn_kv_stream64_kernel<true, true, 4, true, true>"
    assert G.reported(kvw, 0, ctypes.byref(live)) == (None, None)


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
