"""CPU: tests/dense_ref.py held to account before tests/test_gpu_dense_forms.py relies on it.  The float64 restatements
against a second formulation (torch.nn.functional conv1d / group_norm on rows / torch.bmm, a per-point loop for the
EdgeConv maximum, the oracle's linear_attention for the local attention); the bf16 split against the library's own weight
packer; planted faults -- what a kernel with a bookkeeping slip would compute -- which must move the result by ten times the
sharpest bound of every row they apply to; the restated shape rules against the library's exported shape queries (the
library loads without a device); the GPU file's frozen row tables against the restatement, complete over a grid of shapes;
and the rows' instantiations against the kernel names of one kernel-trace run.

Planted faults and the rows they are planted on (every distinct row; a row's sharpest bound is 2e-6 in the f32 unit and
8 y32e -- check (2) of the GPU file -- in the bf16 units, where y32e must itself stay inside the unit's bound):
  a  the last k-block (8 channels in the f32 image, 16 in the bf16 image) left out       every dense row
  b  the W_hi x_lo term of one 16-channel step left out                                    bf16x3 rows
  c  the last token taken from its neighbour                                               L >= 2
  d  the last cout of a partly filled 32-block dropped                                     cout % 32 != 0
  e  the GroupNorm groups start one band (4 channels) late                                 group sizes 8 / 16 / 32 / 64
  f  eps 1e-6 instead of 1e-5                                                              GroupNorm rows
  g  leaky slope 0.1                                                                       act = 2, edge rows
  h  the residual added ahead of the normalisation                                         GroupNorm rows with a residual
  i  a point's last neighbour ignored                                                      edge / local rows, K >= 2
  j  local attention's denominator without eps                                             local rows
NOT SEPARATED: (e) at group size 4 -- one band IS the group, the shifted grouping is the same grouping with the last
group wrapped -- and at group size 2, where groupnorm_kernel has no bands.  Nothing else stayed below its margin."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_ref as R
import test_gpu_dense_forms as G


def _distinct(rows, key):
    seen, out = set(), []
    for r in rows:
        if key(r) not in seen:
            seen.add(key(r))
            out.append(r)
    return out


DENSE = _distinct(G.ROWS, lambda r: r[:1] + r[2:])        # (the asked precision alone changes neither inputs nor unit)


# ---- the restatements against a second formulation ------------------------------------------------------------------
def test_dense_restatements_agree_with_torch_modules_in_float64():
    g = torch.Generator().manual_seed(1)
    B, cin, cout, L = 3, 20, 24, 37
    x, w = torch.randn(B, cin, L, generator=g), torch.randn(cout, cin, generator=g)
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    conv = F.conv1d(x.double(), w.double().unsqueeze(-1)) * sc.double().view(1, -1, 1) + sh.double().view(1, -1, 1)
    for act, fn in ((0, lambda v: v), (1, F.relu), (2, lambda v: F.leaky_relu(v, 0.2))):
        assert float((R.dense_ref(x, w, sc, sh, act) - fn(conv)).abs().max()) < 1e-13
        assert torch.equal(R.dense_ref(x.transpose(1, 2).contiguous(), w, sc, sh, act, x_pm=True), R.dense_ref(x, w, sc, sh, act))
    assert torch.equal(R.dense_max_ref(x, w, sc, sh, 1), R.dense_ref(x, w, sc, sh, 1).amax(dim=2).t())
    assert R.dense_max_ref(x, w, sc, sh, 1).shape == (cout, B)
    # GroupNorm: torch's own on (M, C) rows, as the model applies it (lanegcn_nets.py LinearRes)
    gamma, beta, res = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), torch.randn(B, cout, L, generator=g)
    pre = R.product(x, w)
    rows = pre.permute(0, 2, 1).reshape(B * L, cout)
    for groups in (1, 2, 3, 6, 12, 24):
        gn = F.group_norm(rows, groups, gamma.double(), beta.double(), 1e-5).view(B, L, cout).permute(0, 2, 1)
        assert float((R.groupnorm_ref(pre, gamma, beta, groups) - gn).abs().max()) < 1e-12
        assert float((R.dense_gn_ref(x, w, gamma, beta, groups, res, True) - F.relu(gn + res.double())).abs().max()) < 1e-12
    # per-cloud weights: torch.bmm on the transposed cloud, and the table pcr_pack_bmm_f32 reads
    t = torch.randn(B, cin, cin, generator=g)
    want = torch.bmm(x.double().transpose(1, 2), t.double()).transpose(1, 2)
    assert float((R.bmm_ref(x, t) - want).abs().max()) < 1e-13
    tab = R.bmm_table(t)
    assert tab.shape == (1, cin * cin, B) and float(tab[0, 3 * cin + 5, 2]) == float(t[2, 3, 5])


def test_edge_and_local_restatements_agree_with_a_second_formulation():
    import model_oracle as MO
    B, N, Co, K = 2, 19, 5, 4
    ta, tb, idx, shift = R.edge_inputs(B, N, Co, K)
    want = torch.empty(B, Co, N, dtype=torch.float64)
    for b in range(B):
        for i in range(N):
            m = torch.stack([ta[b, int(j)].double() for j in idx[b, i]]).amax(dim=0)
            want[b, :, i] = F.leaky_relu(m + tb[b, i].double() + shift.double(), 0.2)
    assert float((R.edge_max_ref(ta, tb, idx, shift) - want).abs().max()) < 1e-14
    assert int(idx.max()) == N - 1
    C, nhead = 16, 2
    qkv, idx = R.local_inputs(B, N, C, K)
    r = qkv.double()
    nb = r[torch.arange(B).view(B, 1, 1), idx.long()]                       # (B,N,K,3C)
    q = r[:, :, :C].reshape(B * N, 1, nhead, C // nhead)
    k = nb[..., C:2 * C].reshape(B * N, K, nhead, C // nhead)
    v = nb[..., 2 * C:].reshape(B * N, K, nhead, C // nhead)
    want = MO.linear_attention(q, k, v).reshape(B, N, C).permute(0, 2, 1)
    assert abs(MO.ATTN_EPS - 1e-6) < 1e-12
    got = R.local_attn_ref(qkv, idx, nhead, 1e-6)
    # (1e-10: at the point whose Q is exp(-16) the oracle's v / K ... * K and 1 / (den + eps) round a quotient of 1e-6 sized terms)
    assert float((got - want).abs().max()) < 1e-10 * float(want.abs().max())


# ---- planted faults -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(row):
    d = G.row_inputs(row)
    ref, sharp, yard = G.row_yardsticks(row, d)
    return d, ref, sharp, yard


def _moved(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("row", DENSE, ids=[G.row_id(r) for r in DENSE])
def test_planted_faults_clear_ten_bounds_on_the_dense_rows(row):
    entry, prec, B, cin, cout, L, x_pm, act, groups, res, expect = row
    d, ref, sharp, yard = _case(row)
    unit = R.unit_of(expect)
    assert ref.shape == ((cout, B) if entry == "max" else (B, cout, L))
    if unit == 0:
        assert yard < G.BOUNDS["f32"], "torch float32 itself is outside the f32 bound: %g" % yard
        margin = 10 * G.BOUNDS["f32"]
    else:
        # the emulated arithmetic is inside the unit's bound of the restatement, and its float32 evaluation far inside
        assert R.rel_err(sharp, ref) < G.BOUNDS[R.UNIT[unit]] and G.YARD * yard < G.BOUNDS["bf16x3"]
        margin = 10 * G.YARD * yard
    stored = row if entry != "max" else ("dense",) + row[1:]                # (token faults are planted ahead of the maximum)
    fin = (lambda v: v.amax(dim=2).t()) if entry == "max" else (lambda v: v)
    moved = {}
    kb = 16 if unit else 8
    moved["a"] = _moved(R.dense_row_eval(row, d, drop_k=kb * ((cin - 1) // kb)), ref)
    if unit == 1:
        moved["b"] = _moved(R.dense_row_eval(row, d, "emul", drop_lo_step=(cin // 16) // 2), sharp)
    if L >= 2:
        v = R.dense_row_eval(stored, d).clone()
        v[:, :, L - 1] = v[:, :, L - 2]
        moved["c"] = _moved(fin(v), ref)
    if cout % 32:
        v = R.dense_row_eval(stored, d).clone()
        v[:, cout - 1] = 0
        moved["d"] = _moved(fin(v), ref)
    if entry == "gn":
        if cout // groups >= 8 and groups >= 2:
            moved["e"] = _moved(R.dense_row_eval(row, d, band_shift=4), ref)
        moved["f"] = _moved(R.dense_row_eval(row, d, eps=1e-6), ref)
        if res:
            moved["h"] = _moved(R.dense_row_eval(row, d, res_first=True), ref)
    elif act == 2 and entry != "max":        # (a maximum over leaky values is positive: the slope does not show)
        moved["g"] = _moved(R.dense_row_eval(row, d, slope=0.1), ref)
    for name, m in sorted(moved.items()):
        assert m > margin, "fault (%s) moves the result by %.3g of its scale only, ten bounds are %.3g" % (name, m, margin)
    if entry == "max":
        # the first token, the last and the two beside a 64-token tile boundary each own some channel's maximum, in every cloud
        owner = R.dense_row_eval(stored, d).argmax(dim=2)                   # (B,cout)
        for tok in R.marked_tokens(L):
            assert bool((owner == tok).any(dim=1).all()), tok
    if entry == "gn":
        # the small token's variance is of the order of eps; the residual is nowhere the output
        tok = R.product(d["x"], d["w"])[:, :, min(1, L - 1)]
        var = tok.reshape(B, groups, -1).var(dim=2, unbiased=False)
        assert 1e-7 < float(var.median()) < 1e-3
        assert res == (d["res"] is not None) and (not res or float((d["res"].double() - ref).abs().min()) > 0)


@pytest.mark.parametrize("row", G.EDGE_ROWS, ids=[G.edge_id(r) for r in G.EDGE_ROWS])
def test_planted_faults_on_the_edge_rows(row):
    B, N, Co, K, _, expect = row
    ta, tb, idx, shift = R.edge_inputs(B, N, Co, K)
    ref = R.edge_max_ref(ta, tb, idx, shift)
    assert float((R.edge_max_ref(ta, tb, idx, shift, 0.2, torch.float32).double() - ref).abs().max()) < 2e-6 * float(ref.abs().max())
    assert int(idx.max()) == N - 1 and int(idx.min()) >= 0
    margin = 10 * G.BOUNDS["f32"]
    assert _moved(R.edge_max_ref(ta, tb, idx, shift, 0.1), ref) > margin
    if K >= 2:
        assert _moved(R.edge_max_ref(ta, tb, idx, shift, drop_last=True), ref) > margin
        # every point's first neighbour owns the maximum of channel i % Co; its last that of channel (i + 1) % Co unless the
        # first owns that too
        nb = ta[torch.arange(B).view(B, 1, 1), idx.long()]                  # (B,N,K,Co)
        pts = torch.arange(N)
        of = lambda ch: nb.gather(3, ch.view(1, N, 1, 1).expand(B, N, K, 1)).squeeze(-1)      # noqa: E731  (B,N,K)
        own = of(pts % Co)
        at = own[:, :, 0] if Co >= 2 else torch.where(pts % 2 == 1, own[:, :, K - 1], own[:, :, 0])
        assert bool((at == own.amax(dim=2)).all())
        if Co >= 2:
            nxt = of((pts + 1) % Co)
            top = nxt.amax(dim=2)
            assert bool(((nxt[:, :, K - 1] == top) | (nxt[:, :, 0] == top)).all())
            assert float((nxt[:, :, K - 1] == top).float().mean()) > 0.5


@pytest.mark.parametrize("row", G.LOCAL_ROWS, ids=[G.local_id(r) for r in G.LOCAL_ROWS])
def test_planted_faults_on_the_local_attention_rows(row):
    B, N, C, K, nhead, expect = row
    qkv, idx = R.local_inputs(B, N, C, K)
    ref = R.local_attn_ref(qkv, idx, nhead, 1e-6)
    assert R.rel_err(R.local_attn_ref(qkv, idx, nhead, 1e-6, torch.float32), ref) < G.BOUNDS["f32"]
    assert int(idx.max()) == N - 1
    margin = 10 * G.BOUNDS["f32"]
    assert _moved(R.local_attn_ref(qkv, idx, nhead, 1e-6, den_eps=False), ref) > margin
    assert _moved(R.local_attn_ref(qkv, idx, nhead, 1e-6, drop_last=True), ref) > margin


# ---- the row tables against the restated dispatchers ---------------------------------------------------------------------
def _name(row):
    entry, prec, B, cin, cout, L, x_pm, act, groups, res, _ = row
    return R.dispatch(entry, B, cin, cout, L, R.PREC[prec] if entry in ("dense", "gn") else 0, x_pm, cout // groups if groups else 0)


CINS = (3, 8, 16, 20, 24, 32, 33, 64, 100, 128, 129, 192, 200, 256, 283, 284, 320, 384, 512, 640, 768, 1024, 1280, 1536, 2048)
COUTS = (1, 3, 7, 32, 33, 48, 64, 72, 96, 100, 128, 129, 160, 256, 288, 512, 1024)
LENS = (1, 17, 32, 33, 64, 66, 100, 127, 128, 131, 196, 256, 384)


def test_row_tables_match_the_restatement_and_cover_every_reachable_instantiation():
    for row in G.ROWS:
        assert _name(row) == row[10], G.row_id(row)
        assert row[0] != "bmm" or row[3] == row[4]
    assert len({G.row_id(r) for r in G.ROWS}) == len(G.ROWS)
    for B, N, Co, K, _, expect in G.EDGE_ROWS:
        assert R.edge_dispatch(N, Co, K, B) == expect
    for B, N, C, K, nhead, expect in G.LOCAL_ROWS:
        assert R.local_dispatch(N, C, K, nhead, B) == expect
    # (a launch rows.dense_gn falls back to is the dense launch and groupnorm_kernel, each an instantiation of its own)
    listed = {part for r in G.ROWS for part in r[10].split(" + ")}
    # every instantiation the restated rules reach over a grid of shapes, in every mode, is a row
    reach = set()
    for cin in CINS:
        for cout in COUTS:
            for L in LENS:
                reach.add(R.dispatch("max", 3, cin, cout, L))
                if cin == cout:
                    reach.add(R.dispatch("bmm", 3, cin, cout, L))
                for prec in (0, 1, 2):
                    for x_pm in (0, 1):
                        reach.add(R.dispatch("dense", 3, cin, cout, L, prec, x_pm))
                    for gs in (1, 2, 4, 8, 16, 32, 64):
                        if cout % gs == 0:
                            reach.add(R.dispatch("gn", 3, cin, cout, L, prec, 0, gs))
    reach = {part for name in reach for part in name.split(" + ")} - {"refused"}
    assert reach <= listed, sorted(reach - listed)
    assert listed <= reach, sorted(listed - reach)
    edge = {R.edge_dispatch(N, Co, K) for N in range(1, 1100) for Co in (1, 40, 256) for K in (1, 20, 64)}
    assert edge == {r[5] for r in G.EDGE_ROWS}
    local = {R.local_dispatch(N, C, K, h) for N in range(1, 700, 3) for C in (8, 16, 32, 48, 64) for K in (1, 7, 20, 48)
             for h in (1, 2, 3, 4, 8) if C % h == 0}
    local.discard("refused")
    assert local == {r[5] for r in G.LOCAL_ROWS}
    # one row with more clouds than XCDs per kernel family and unit, and a single cloud once per family of the dense file
    for rows, col, bcol in ((G.ROWS, 10, 2), (G.EDGE_ROWS, 5, 0), (G.LOCAL_ROWS, 5, 0)):
        fam = {r[col].split("<")[0] for r in rows}
        assert fam == {r[col].split("<")[0] for r in rows if r[bcol] == 11}, sorted(fam)
    assert any(r[2] == 1 for r in G.ROWS) and any(r[0] == 1 for r in G.EDGE_ROWS)
    # the edges that are code paths of their own are rows: both load paths and the ragged tile of the resident-weight kernel,
    # a cout block beyond coutP, the forms the issue found unreached
    have = {(r[10], r[3], r[4], r[5]) for r in G.ROWS}
    for want in (("f32 rw<4,store>", 16, 128, 128), ("f32 rw<4,store>", 24, 160, 131), ("f32 rw<8,store>", 64, 288, 196),
                 ("f32 tile<1,plain>", 320, 160, 50), ("f32 tile<1,plain>", 1024, 160, 40), ("f32 max<>", 3, 256, 37),
                 ("f32 max<>", 200, 512, 130), ("bf16x3 pc<plain,2>", 256, 160, 128), ("bf16 pc<gn,2>", 256, 288, 256)):
        assert want in have, want
    assert {r[4] // r[8] for r in G.ROWS if r[0] == "gn" and " bf<gn" in r[10]} == {4, 8, 16, 32}
    assert {r[4] // r[8] for r in G.ROWS if r[0] == "gn" and " tile<" in r[10] and "+" not in r[10]} == {4, 8, 16, 32}
    assert {r[4] // r[8] for r in G.ROWS if "+ groupnorm" in r[10]} >= {2, 64, 48}
    assert {r[5] for r in G.LOCAL_ROWS} == {"local lds<32>", "local<32>", "local<16>", "local<0>"}
    assert any(r[1] > 512 and 256 % r[2] and r[3] % 4 for r in G.EDGE_ROWS)      # gather, Co not dividing 256, K % 4 != 0


def test_every_listed_instantiation_was_seen_in_the_kernel_trace():
    """profiles/r17a_dense_forms_kernels.txt: the distinct kernels of one kernel-trace run of the GPU file alone"""
    from conftest import ROOT
    seen = open(os.path.join(ROOT, "profiles", "r17a_dense_forms_kernels.txt")).read()
    names = {r[10] for r in G.ROWS} | {r[5] for r in G.EDGE_ROWS} | {r[5] for r in G.LOCAL_ROWS}
    wanted = {R.kernel_name(n) for n in names} | {"groupnorm_kernel("}
    missing = sorted(n for n in wanted if "::" + n not in seen)
    assert not missing, missing
    # and no dense / edge / local-attention kernel ran that the tables do not name
    ran = {line.split("::", 1)[1].split("(")[0] for line in seen.splitlines() if "::" in line}
    ours = ("dense_", "edge_max", "local_attn", "groupnorm_kernel")
    extra = sorted(n for n in ran if n.startswith(ours) and not any(w.rstrip("(") == n for w in wanted))
    assert not extra, extra
    assert "edge_max_lds_kernel<64>" not in seen            # (PCR_EDGE_CS = 64 only: NOT RUN)


# ---- the restated rules against the library --------------------------------------------------------------------------------
def _lib():
    """the library, which needs no device for its shape queries and its host-side packers.  Skipped only where it is not
    built or the loader cannot open it (no ROCm runtime on this host); a broken import or another ABI fails"""
    import torch  # noqa: F401  (must precede the HIP library)
    from pcr_amd import _lib as L
    if not os.path.exists(L.SO_PATH):
        pytest.skip("libpcr_hip is not built")
    try:
        return L.load()
    except OSError as e:
        pytest.skip("libpcr_hip does not load: %s" % e)


def test_restated_rules_equal_the_exported_shape_queries():
    lib = _lib()
    for cin in tuple(range(1, 130)) + CINS + (2304, 4096):
        for cout in tuple(range(1, 140)) + COUTS:
            for L in (0, 1, 33, 128):
                assert lib.pcr_dense_prec_ok(cin, cout, L) == R.prec_ok(cin, cout, L), (cin, cout, L)
                assert lib.pcr_dense_xpm_prec_ok(cin, cout, L) == R.xpm_prec_ok(cin, cout, L), (cin, cout, L)
                assert lib.pcr_dense_max_ok(cin, cout, L) == R.max_ok(cin, cout, L), (cin, cout, L)
    for cin in range(200, 300):
        assert lib.pcr_dense_max_ok(cin, 256, 64) == R.max_ok(cin, 256, 64)
    assert R.xpm_prec_ok(2048, 128, 128) == 0 and R.xpm_prec_ok(256, 128, 128) == 1 and R.xpm_prec_ok(320, 128, 128) == 0 and R.max_ok(240, 256, 1) and not R.max_ok(241, 256, 1)


def test_the_bf16_split_is_the_weight_packers_split():
    """hi = bf16(v), lo = bf16(v - hi), round to nearest even: dense_ref.bf_split against pcr_pack_weight_bf16x2_f32 (a
    host function), values with ties, values near a binade's end and small ones among them"""
    import ctypes
    lib = _lib()
    g = torch.Generator().manual_seed(3)
    cout, cin = 40, 50
    w = torch.randn(cout, cin, generator=g)
    w[0, :8] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.998046875, 3.0e-5, 1.99609375, 255.5, -0.0])   # ties
    w[1] = (w[1].view(torch.int32) | 0x8000).view(torch.float32)[:cin]           # halfway-or-above patterns
    w[2] = (w[2].view(torch.int32) & ~0xFFFF | 0x8000).view(torch.float32)[:cin]    # exact ties on the hi rounding
    n = lib.pcr_packed_weight_bf16_floats(cout, cin)
    out = np.zeros(n, np.float32)
    wn = w.numpy()
    assert lib.pcr_pack_weight_bf16x2_f32(wn.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p)) == 0
    img = torch.from_numpy(out.view(np.uint16).astype(np.int32)).view((cin + 15) // 16, R.ceil32(cout) // 32, 2, 64, 8)
    hi, lo = R.bf_split(w)
    bits = lambda t: (t.view(torch.int32) >> 16) & 0xFFFF      # noqa: E731
    kpos = lambda h, j: 4 * h + j if j < 4 else 8 + 4 * h + (j - 4)      # noqa: E731  (tile_dense.h: bf_kpos)
    for s in range(img.shape[0]):
        for cb in range(img.shape[1]):
            for lane in range(64):
                for j in range(8):
                    o, k = cb * 32 + (lane & 31), 16 * s + kpos(lane >> 5, j)
                    inside = o < cout and k < cin
                    assert int(img[s, cb, 0, lane, j]) == (int(bits(hi[o, k])) if inside else 0), (o, k)
                    assert int(img[s, cb, 1, lane, j]) == (int(bits(lo[o, k])) if inside else 0), (o, k)
    # and the split is what the emulated product uses: three terms against one
    x = torch.randn(2, cin, 5, generator=g)
    full = R.product(x, w)
    assert torch.equal(R.dense_emul(x, w, ns=3), R.product_emul(x, w, 3)) and torch.equal(R.dense_emul(x, w, ns=1, act=1), torch.relu(R.product_emul(x, w, 1)))
    gam, bet = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    assert torch.equal(R.dense_gn_emul(x, w, gam, bet, 5), R.groupnorm_ref(R.product_emul(x, w, 3), gam, bet, 5))
    assert 1e-7 < R.rel_err(R.product_emul(x, w, 3), full) < 2e-5 < R.rel_err(R.product_emul(x, w, 1), full) < 2e-2
