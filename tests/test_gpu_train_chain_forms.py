"""GPU: the two fused per-token chains of the attention blocks in training mode (pcr_attn_tail_{fwd,bwd}_f32,
pcr_attn_head_{fwd,bwd}_f32; csrc/train_chain_kernels.hip) through train_ops.attn_tail / attn_head against the float64
restatement of tests/train_chain_ref.py: forward, every input gradient and every parameter gradient, tensor by tensor
(`rel` = max|a - b| / max|b|; every projection of a head to its own norm), under each of the three arithmetics, every
case twice for bit-equality.  test_gpu_train_chain.py holds fused against unfused; this file holds the launches to
float64, tile by tile:

  L edges            (B, L) = (2,1) (2,63) (2,64) (2,65) (3,100) (2,130), every instantiation, one tile per workgroup:
                     whole tiles through ck_load3, partial ones through load_tile, L % 4 != 0 through the scalar stores;
                     and there the forward under "bf16x3" is the "f32" one bit for bit
  several tiles      L = 132 / 131 (three tiles per cloud: full, full, partial) with the smallest B whose tiles exceed
                     twice the grid -- read from pcr_attn_*_groups, asserted -- so that persistent workgroups walk two
                     and three tiles, a partial one behind a full one and a full one behind a partial one; one shape
                     per plan
  position           the same 384 tokens as (6,64) (3,128) (4,96) (2,192): per-token outputs bit-equal across layouts
  unaligned base     L = 128 with msg | x, then d out, 4-byte but not 16-byte aligned (the second half of ck_whole's test;
                     include/pcr.h asks no alignment of them): bit-equal to the aligned run
  shut units         head: a hidden unit closed on every token has dP1 row and dc1 exactly 0, and no other has
  records / guards   the launches themselves, descriptors filled as train_ops fills them: sentinels around every output,
                     part_stride = record + 32 with the spare floats untouched, the dead columns of dW0 exactly 0, and
                     reduce_regions of the records = the Function's gradients bit for bit
  stress             every token's channel mean of msg | x at 10 sigma, gamma1 with a negative and a zero channel

Bounds (train_chain_ref.BOUNDS): 2e-5 under "f32"; under "bf16x3" the forward 2e-5 (it IS the f32 forward) and the
gradients 3e-5; 5e-5 under "bf16x3_all".  Stress rows: max(that, 8 x the row's own CPU yardstick), never a figure read
off the kernel.  Every input is conditioned to zero marginal ReLU decisions (test_train_chain_ref_cpu.py shows it for
every key built here); no token is masked out of any comparison."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn as nn

import train_chain_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 98765.0
GUARD = 64                 # sentinel floats on each side of a carved output
SPARE = 32                 # part_stride - record


@contextlib.contextmanager
def _arith(name):
    from pcr_amd import train_ops as TO
    prev = TO.set_train_precision(name)
    try:
        yield
    finally:
        TO.set_train_precision(prev)


def _set(t, v):
    with torch.no_grad():
        t.copy_(v)


def _tail_module(case):
    d, c1, hid, out = case["shape"]
    m = nn.Module()
    m.merge = nn.Linear(d, d, bias=False)
    m.mlp = nn.Sequential(nn.Linear(c1 + d, hid, bias=False), nn.ReLU(True), nn.Linear(hid, out, bias=False))
    m.norm1, m.norm2 = nn.LayerNorm(d), nn.LayerNorm(out)
    named = dict(Wm=m.merge.weight, g1=m.norm1.weight, b1=m.norm1.bias, W0=m.mlp[0].weight, W2=m.mlp[2].weight,
                 g2=m.norm2.weight, b2=m.norm2.bias)
    for k, t in named.items():
        _set(t, case["p"][k])
    m.cuda()
    return m, named


def _head_module(case):
    c, hd, d, n, _ = case["shape"]
    m = nn.Module()
    m.pos_mlp = nn.Sequential(nn.Linear(3, hd), nn.ReLU(True), nn.Linear(hd, c))
    m.proj = nn.ModuleList([nn.Linear(c, d, bias=False) for _ in range(n)])
    named = dict(P1=m.pos_mlp[0].weight, c1=m.pos_mlp[0].bias, P2=m.pos_mlp[2].weight, c2=m.pos_mlp[2].bias)
    named.update({"W_%d" % j: m.proj[j].weight for j in range(n)})
    for k, t in named.items():
        _set(t, case["p"][k])
    m.cuda()
    return m, named


def _place(t, off):
    """t on the device as a contiguous tensor whose base address is 4 * off bytes past a 16-byte boundary"""
    if not off:
        return t.cuda()
    buf = torch.empty(t.numel() + 4, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def run_chain(case, off_in=0, off_dout=0):
    """-> (out, {gradient name: tensor}) of one fused forward + backward through train_ops, on the CPU, under the arithmetic
    in force"""
    from pcr_amd import train_ops as TO
    dout = _place(case["dout"], off_dout)
    if case["kind"] == "tail":
        m, named = _tail_module(case)
        a = _place(case["msg"], off_in).requires_grad_(True)
        b = case["res"].cuda().requires_grad_(True)
        out = TO.attn_tail(m, a, b, case["residual"])
        names, leaves = ["dmsg", "dres"], [a, b]
    else:
        m, named = _head_module(case)
        a = _place(case["x"], off_in).requires_grad_(True)
        out = TO.attn_head(m.pos_mlp, a, case["xyz"].cuda(), tuple(p.weight for p in m.proj), case["src"])
        names, leaves = ["dx"], [a]
    assert out is not None, "no fused instantiation"
    grads = torch.autograd.grad(out, leaves + list(named.values()), dout)
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: g.cpu() for k, g in zip(names + ["d" + k for k in named], grads)}


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def check(case, want, arith, row, yard=None):
    """run twice under `arith`, bit-equal; every tensor within the bounds.  -> the first run"""
    with _arith(arith):
        got = run_chain(case)
        assert _same(got, run_chain(case)), (case["key"], arith, "two runs differ")
    bf, bg = R.bounds(arith, yard)
    _, _, per = R.compare(case, got, want)
    for k, v in per.items():
        print("FIG %s %s %s %s %.3g" % (row, case["kind"], arith, k, v))
    bad = {k: v for k, v in per.items() if not v < (bf if k.startswith("out") else bg)}
    assert not bad, (case["key"], arith, bad, (bf, bg))
    return got


# ------------------------------------------------------------------------------------------- L edges --
_EDGE = [("tail", f, B, Ln) for f in R.TAIL_FORMS for B, Ln in R.EDGE_BL] + \
        [("head", s, B, Ln) for s in R.HEAD_SHAPES for B, Ln in R.EDGE_BL]


@pytest.mark.parametrize("kind,form,B,Ln", _EDGE, ids=repr)
def test_every_instantiation_at_the_tile_edges(kind, form, B, Ln):
    case, want = R.reference((kind, form, B, Ln, "plain"))
    got = {a: check(case, want, a, "edge") for a in R.ARITHS}
    # "bf16x3" keeps the f32 forward: every value, and with it every ReLU mask, is the f32 graph's
    assert torch.equal(got["f32"][0], got["bf16x3"][0])


# ------------------------------------------------------------------ a workgroup walking several tiles --
def _cap(kind, form, Ln):
    """the grid cap, as pcr_attn_*_groups of a descriptor with B = 4096 gives it"""
    from pcr_amd import _lib as L
    from pcr_amd.abi import _AttnHeadP, _AttnTailP
    lib = L.load()
    if kind == "tail":
        p = _AttnTailP()
        p.B, p.L, (p.d, p.c1, p.hid, p.out) = 4096, Ln, form[0]
        return lib.pcr_attn_tail_groups(ctypes.byref(p)), R.tail_lds(form[0])
    p = _AttnHeadP()
    p.B, p.L, (p.c, p.hd, p.d, p.np, p.src) = 4096, Ln, form
    return lib.pcr_attn_head_groups(ctypes.byref(p)), R.head_lds(form)


@pytest.mark.parametrize("kind,form,Ln,ariths", [(k, f, Ln, a) for k, f, _, Ln, a in R.multi_rows()], ids=repr)
def test_a_workgroup_walks_full_and_partial_tiles(kind, form, Ln, ariths):
    cap, lds = _cap(kind, form, Ln)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cap == R.groups_cap(lds, cus)                       # the plan restated in train_chain_ref is the library's
    B = R.multi_tile_B(cap)
    tiles, groups = B * ((Ln + R.TILE - 1) // R.TILE), min(cap, B * ((Ln + R.TILE - 1) // R.TILE))
    assert tiles == 3 * B and tiles > 2 * groups and 3 * (B - 1) <= 2 * groups
    assert groups % 3 != 0          # a workgroup's successive tiles (stride = grid) then change position in their cloud
    case, want = R.reference((kind, form, B, Ln, "plain"))
    for a in ariths:
        check(case, want, a, "multi%d" % Ln)


# ------------------------------------------------------------------------------ position independence --
@pytest.mark.parametrize("kind,form", [("tail", f) for f in R.TAIL_PLANS] + [("head", s) for s in R.HEAD_PLANS], ids=repr)
def test_per_token_outputs_do_not_depend_on_the_layout(kind, form):
    base = R.build_case((kind, form, 6, 64, "pos"))
    per_token = ("dmsg", "dres") if kind == "tail" else ("dx",)
    for a in ("f32", "bf16x3_all"):
        first = None
        for B, Ln in R.POS_LAYOUTS:
            case = R.with_layout(base, B, Ln)
            out, grads = check(case, R.evaluate(case), a, "pos")
            flat = [R.relayout(t, 6, 64) for t in [out] + [grads[k] for k in per_token]]
            first = first or flat
            assert all(torch.equal(x, y) for x, y in zip(flat, first)), (kind, form, a, (B, Ln))


# ------------------------------------------------------------------------------------- unaligned base --
@pytest.mark.parametrize("kind,form", [("tail", R.TAIL_PLANS[1]), ("head", R.HEAD_PLANS[2])], ids=repr)
def test_a_chunk_aligned_L_on_an_unaligned_base_takes_the_scalar_loads(kind, form):
    case, want = R.reference((kind, form, 2, 128, "plain"))
    aligned = check(case, want, "bf16x3", "unaligned")
    with _arith("bf16x3"):
        assert _same(run_chain(case, off_in=1), aligned)
        assert _same(run_chain(case, off_dout=1), aligned)
        assert _same(run_chain(case, off_in=1, off_dout=1), aligned)


# ----------------------------------------------------------------------------------------- shut units --
@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=repr)
def test_a_hidden_unit_shut_on_every_token_has_exactly_zero_gradients(shape):
    case, want = R.reference(("head", shape, 3, 100, "shut"))
    shut = (R.head_hidden(case["xyz"], case["p"]) <= 0).all(dim=2).all(dim=0)
    assert set(R.SHUT_ROWS) <= set(shut.nonzero().flatten().tolist())
    assert torch.equal((want[1]["dP1"] == 0).all(dim=1), shut) and torch.equal(want[1]["dc1"] == 0, shut)
    for a in ("f32", "bf16x3"):
        _, grads = check(case, want, a, "shut")
        assert torch.equal((grads["dP1"] == 0).all(dim=1), shut), a
        assert torch.equal(grads["dc1"] == 0, shut), a
        assert bool((grads["dP2"][:, shut] == 0).all()), a         # relu(pre) = 0 there: its column of dP2 as well


# ----------------------------------------------------------------------------------- records and guards --
def _carve(shape, fill=SENTINEL):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
def test_tail_launches_write_their_outputs_and_records_and_nothing_else(arith):
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    shape = (64, 3, 128, 32)
    d, c1, hid, out = shape
    case, _ = R.reference(("tail", (shape, False), 3, 100, "plain"))
    B, Ln = 3, 100
    with _arith(arith):
        ref_out, ref_g = run_chain(case)
        bf = TO._chain_bf()
        w = {k: v.cuda() for k, v in case["p"].items()}
        msg, res, dout = case["msg"].cuda(), case["res"].cuda(), case["dout"].cuda()
        images = [TO._chain_images(w[k], bf) for k in ("Wm", "W0", "W2")]
        p, _ = TO._tail_params(msg, res, w["Wm"], w["g1"], w["b1"], w["W0"], w["W2"], w["g2"], w["b2"], False, R.NORM_EPS,
                               images, bf)
        lib = L.load()
        rec, nwg = lib.pcr_attn_tail_part_floats(d, c1, hid, out), lib.pcr_attn_tail_groups(ctypes.byref(p))
        assert rec == R.tail_rec(shape) and nwg == B * 2
        stride = rec + SPARE
        (ob, o), (mb, dmsg), (rb, dres), (pb, parts) = (_carve(s) for s in ((B, out, Ln), (B, d, Ln), (B, c1, Ln), (nwg, stride)))
        p.outp = TO._p(o)
        L.run.pcr_attn_tail_fwd_f32(ctypes.byref(p), L.stream_ptr())
        p.dout, p.dmsg, p.dres, p.parts, p.part_stride = TO._p(dout), TO._p(dmsg), TO._p(dres), TO._p(parts), stride
        L.run.pcr_attn_tail_bwd_f32(ctypes.byref(p), L.stream_ptr())
        torch.cuda.synchronize()
        cup = R.c32(c1 + d)
        o0, o2 = d * d, d * d + hid * cup
        og = o2 + out * hid
        regs = [(0, d, d, d), (o0, hid, c1 + d, cup), (o2, out, hid, hid), (og, 1, d, d), (og + d, 1, d, d),
                (og + 2 * d, 1, out, out), (og + 2 * d + out, 1, out, out)]
        red = TO.reduce_regions(parts, nwg, stride, regs)
        torch.cuda.synchronize()
    assert all(_guards_intact(b) for b in (ob, mb, rb, pb))
    assert bool((parts[:, rec:] == SENTINEL).all())                             # the spare floats of every record
    assert not bool((parts[:, :rec] == SENTINEL).any())                         # ... and the record itself is written
    dead = parts[:, o0:o2].view(nwg, hid, cup)[:, :, c1 + d:]
    assert dead.numel() == nwg * hid * (cup - c1 - d) and bool((dead == 0).all())
    assert torch.equal(o.cpu(), ref_out) and torch.equal(dmsg.cpu(), ref_g["dmsg"]) and torch.equal(dres.cpu(), ref_g["dres"])
    for k, t in zip(("dWm", "dW0", "dW2", "dg1", "db1", "dg2", "db2"), red):
        assert torch.equal(t.cpu().reshape(ref_g[k].shape), ref_g[k]), k


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
def test_head_launches_write_their_outputs_and_records_and_nothing_else(arith):
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    shape = (64, 64, 64, 3, 4)
    c, hd, d, n, src = shape
    case, _ = R.reference(("head", shape, 3, 100, "plain"))
    B, Ln = 3, 100
    with _arith(arith):
        ref_out, ref_g = run_chain(case)
        bf = TO._chain_bf()
        w = {k: v.cuda() for k, v in case["p"].items()}
        Ws = [w["W_%d" % j] for j in range(n)]
        x, xyz, dout = case["x"].cuda(), case["xyz"].cuda(), case["dout"].cuda()
        images = [TO.pack_both(w["P1"]), TO._chain_images(w["P2"], bf)] + [TO._chain_images(W, bf) for W in Ws]
        p, _ = TO._head_params(x, xyz, w["P1"], w["c1"], w["P2"], w["c2"], src, Ws, images, bf)
        lib = L.load()
        rec, nwg = lib.pcr_attn_head_part_floats(c, hd, d, n, src), lib.pcr_attn_head_groups(ctypes.byref(p))
        assert rec == R.head_rec(shape) and nwg == B * 2
        stride = rec + SPARE
        (ob, o), (xb, dx), (pb, parts) = (_carve(s) for s in ((B, n * d, Ln), (B, c, Ln), (nwg, stride)))
        p.outp = TO._p(o)
        L.run.pcr_attn_head_fwd_f32(ctypes.byref(p), L.stream_ptr())
        p.dout, p.dx, p.parts, p.part_stride = TO._p(dout), TO._p(dx), TO._p(parts), stride
        L.run.pcr_attn_head_bwd_f32(ctypes.byref(p), L.stream_ptr())
        torch.cuda.synchronize()
        o_p2 = hd * 32
        o_w = o_p2 + c * hd
        o_c1 = o_w + n * d * c
        regs = [(0, hd, 3, 32), (o_c1, 1, hd, hd), (o_p2, c, hd, hd), (o_c1 + hd, 1, c, c)] + \
               [(o_w + j * d * c, d, c, c) for j in range(n)]
        red = TO.reduce_regions(parts, nwg, stride, regs)
        torch.cuda.synchronize()
    assert all(_guards_intact(b) for b in (ob, xb, pb))
    assert bool((parts[:, rec:] == SENTINEL).all())
    assert not bool((parts[:, :rec] == SENTINEL).any())
    assert bool((parts[:, :o_p2].view(nwg, hd, 32)[:, :, 3:] == 0).all())       # dP1 [hd][32]: the columns past xyz
    assert torch.equal(o.cpu(), ref_out) and torch.equal(dx.cpu(), ref_g["dx"])
    for k, t in zip(["dP1", "dc1", "dP2", "dc2"] + ["dW_%d" % j for j in range(n)], red):
        assert torch.equal(t.cpu().reshape(ref_g[k].shape), ref_g[k]), k


# --------------------------------------------------------------------------------------------- stress --
@pytest.mark.parametrize("kind,form", [("tail", f) for f in R.TAIL_PLANS] + [("head", s) for s in R.HEAD_PLANS], ids=repr)
def test_token_means_at_ten_sigma_and_a_dead_and_a_negative_gamma(kind, form):
    case, want = R.reference((kind, form, 3, 100, "stress"))
    yard = R.yardsticks(case, want)
    for a in R.ARITHS:
        print("BOUND stress %s %s %s fwd %.3g grad %.3g" % ((kind, form, a) + R.bounds(a, yard)))
        check(case, want, a, "stress", yard)
