"""GPU: attn_kv_stream64_kernel leaves out the K rows x hidden columns of the fused projection where that block of the
weight image is all zeros (every block built with k_pos = False: wkv = [[Wk, 0], [Wv, Wv W2]]) and forms the hidden-layer
and feature operands step by step.  Held here, per shape, head count and arithmetic unit, on an FP_SA block's seeded
weights:

  weights   (a) k_pos = False, as the modules build it -- the zero block;
            (b) the same block with k_pos = True -- a dense block, never skipped;
            (c) the image of (a) with ONE nonzero planted in the block, at its first element (wkv[0, c2]) and at its last
                (wkv[d - 1, c2 + d - 1]), re-packed through engine.pack_weight / pack_weight_bf: the flag stays off and the
                planted weight shows in the state;
            (d) the image of (a) with the block filled with -0.0: counts as zero;
            (e) the image of (a) with 2^-126 planted at the block's first element.  A nonzero, so the FULL form runs -- and
                a product of at most a few 2^-126 cannot move a float32 accumulator that already holds the feature steps' sum
                (nor, where that sum were 0, anything elu + 1 passes on), so (e) must give the bits of (a).
  checks    full form == skipped form, bit for bit, twice over: (a) and (d) under PCR_ATTN_KV_FULL=1 against themselves
            without it -- the switch is read per launch by a library built with -DPCR_TUNING=1 and ignored by the shipped
            one, where the comparison is of a launch with itself -- and (e) against (a), which needs no switch and so says
            the same of the shipped library: the work left out was not needed;
            M and ksum unpacked from the launch's buffer against attn_ref.kv_state in float64 fed the same, possibly
            planted, weights (the planted column through the restatement's product hook), under
            test_gpu_attn_forms.state_bounds with the two yardsticks recomputed for these weights on the CPU;
            every launch twice with equal bits; every cloud alone (B = 1: a workgroup round with dead cloud slots) gives
            the bits it gives in the batch of three.
  shapes    the smallest at which each path can go wrong: c2 = 64 (XS = 4) with Sk = 32 and 96 (one wave per cloud, one
            and three blocks), 160 (five blocks on four waves: one wave takes a second block while its neighbours take one
            -- a partly filled last pass) and 256 (two blocks on each of four waves); c2 = 128 (XS = 8) with Sk = 128
            and 160; one head (four KV tiles) and two (the diagonal ones).  In f32 mode the c2 = 128 rows run the tile
            kernel, which has no such block to skip; they are held to the same checks.
  gated     one launch with a device count below capacity, as tests/test_gpu_match_live.py sets it up: live clouds give
            the un-gated bits with and without the switch and with the (e) image (the gated twin's full form, no switch
            needed), dead clouds are not written.

Bounds are the existing ones; none is read off a kernel."""
import functools
import os
import types

import pytest
import torch
import torch.nn.functional as F

import attn_ref as R
import test_gpu_attn_forms as G

pytestmark = pytest.mark.gpu

D = 64
POS = "pos_mlp2"
SHAPES = [(64, 32), (64, 96), (64, 160), (64, 256), (128, 128), (128, 160)]      # (c2, Sk)
VARIANTS = ("a", "b", "c_first", "c_last", "d", "e")
PLANT = 0.5
TINY = 2.0 ** -126
SWITCH = "PCR_ATTN_KV_FULL"


class full_form:
    """PCR_ATTN_KV_FULL=1 around the launches inside (read at every launch by a tuning build of the library)"""

    def __enter__(self):
        self.prev = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1"

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = self.prev


@functools.lru_cache(maxsize=None)
def block(c2, nhead, Sk):
    """the seeded FP_SA block of a row (CPU) with its inputs: three key clouds"""
    from pcr_amd import testing as T
    from mmdet3d.models.pointnet2_utils import FP_SA
    m = FP_SA(0, 32, c2, D, 64, nhead)
    m.load_state_dict(T.seeded_state_dict(T.manifest_of(m), 5))
    m.eval()
    g = torch.Generator().manual_seed(7000 + 8 * Sk + c2 + nhead)
    fk, xk = torch.randn(3, c2, Sk, generator=g), torch.randn(3, Sk, 3, generator=g)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return types.SimpleNamespace(m=m, sd=sd, fk=fk, xk=xk, case=G.Case("kvskip", "fp", (32, c2, D, 64), nhead, 3, 32, Sk))


def planted_block(variant, c2):
    """the K rows x hidden columns block a variant puts in the place of (a)'s zeros (None: the plan's own image)"""
    if variant in ("a", "b"):
        return None
    kz = torch.zeros(D, D, dtype=torch.float64)
    if variant == "c_first":
        kz[0, 0] = PLANT
    elif variant == "c_last":
        kz[D - 1, D - 1] = PLANT
    elif variant == "d":
        kz = -kz                      # every element -0.0
        assert bool(torch.signbit(kz).all())
    else:
        kz[0, 0] = TINY
    return kz


def fused_wkv(sd, kz):
    """[[Wk, kz], [Wv, Wv W2]] as engine.AttnPlan builds it (float64, rounded to float32 once)"""
    f64 = lambda k: sd[k].double()      # noqa: E731
    Wk, Wv, W2 = f64("k_proj.weight"), f64("v_proj.weight"), f64(POS + ".2.weight")
    return torch.cat([torch.cat([Wk, kz], dim=1), torch.cat([Wv, Wv @ W2], dim=1)], dim=0).float()


def device_plan(blk, variant):
    """engine.AttnPlan of the row on the device, its kv images replaced by the variant's"""
    from pcr_amd import engine
    dev = torch.device("cuda")
    plan = engine.AttnPlan(blk.m, POS, dev, blk.case.nhead, q_pos=0, k_pos=int(variant == "b"), residual=0)
    if variant != "b":
        # (the restatement of the fused matrix above IS the engine's: its image of (a) is the plan's, bit for bit)
        own = fused_wkv(blk.sd, torch.zeros(D, D, dtype=torch.float64))
        assert torch.equal(engine.pack_weight(own, dev), plan.t["wkv"])
        assert torch.equal(engine.pack_weight_bf(own, dev).view(torch.int32), plan.t["wkv_bf"].view(torch.int32))
    kz = planted_block(variant, blk.case.dims[1])
    if kz is not None:
        w = fused_wkv(blk.sd, kz)
        if variant == "d":
            assert bool(torch.signbit(w[:D, blk.case.dims[1]:]).all())
        plan.t["wkv"], plan.t["wkv_bf"] = engine.pack_weight(w, dev), engine.pack_weight_bf(w, dev)
    return plan


# ------------------------------------------------------------------------------------------ CPU side --
def _hidden(sd, xyz, dtype):
    return F.relu(F.linear(xyz.to(dtype), sd[POS + ".0.weight"].to(dtype), sd[POS + ".0.bias"].to(dtype)))


def planted_mm(sd, xyz, kz, mm):
    """attn_ref's product hook with the planted block: the K projection gains hid kz^T, every other product is mm's"""
    Wk, hid = sd["k_proj.weight"].double(), _hidden(sd, xyz, torch.float64)

    def hook(x, w):
        y = mm(x, w)
        if w.shape == Wk.shape and x.shape[:-1] == hid.shape[:-1] and torch.equal(w, Wk):
            y = y + mm(hid, kz)
        return y
    return hook


def state32(blk, k_pos, kz):
    """(M, ksum) in float32 torch, the oracle's order of operations (test_gpu_attn_forms.state32 with the planted block)"""
    sd = {k: v.float() for k, v in blk.sd.items()}
    H = blk.case.nhead
    with torch.no_grad():
        f = blk.fk.float().permute(0, 2, 1)
        hid = _hidden(sd, blk.xk, torch.float32)
        pos = F.linear(hid, sd[POS + ".2.weight"], sd[POS + ".2.bias"])
        B, S, _ = f.shape
        pre = F.linear(f + pos if k_pos else f, sd["k_proj.weight"])
        if kz is not None:
            pre = pre + F.linear(hid, kz.float())
        K = (F.elu(pre) + 1).view(B, S, H, D // H)
        V = F.linear(f + pos, sd["v_proj.weight"]).view(B, S, H, D // H) / S
        KV = torch.einsum("nshd,nshv->nhdv", K, V)
        M = torch.einsum("ohv,nhdv->nohd", sd["merge.weight"].view(D, H, D // H), KV).reshape(B, D, D)
        return M, K.sum(dim=1).reshape(B, D)


@functools.lru_cache(maxsize=None)
def yardsticks(c2, nhead, Sk, variant):
    """test_gpu_attn_forms.state_yardsticks for a variant's weights: .M, .ksum (float64) and (y32, ysplit) of each"""
    blk = block(c2, nhead, Sk)
    k_pos = int(variant == "b")
    kz = planted_block(variant, c2)
    # (the kernels see the planted weight rounded to float32; 0.5 and 2^-126 are exact there)
    hook = (lambda mm: mm) if kz is None else (lambda mm: planted_mm(blk.sd, blk.xk, kz, mm))
    M, ksum = R.kv_state(blk.sd, POS, blk.fk, blk.xk, nhead, k_pos, mm=hook(R.exact_mm))
    Ms, ks = R.kv_state(blk.sd, POS, blk.fk, blk.xk, nhead, k_pos, mm=hook(R.split_mm))
    M32, k32 = state32(blk, k_pos, kz)
    gap = lambda a, b: float((a.double() - b).abs().max())      # noqa: E731
    return types.SimpleNamespace(M=M, ksum=ksum, yM32=gap(M32, M), yk32=gap(k32, ksum), yMsplit=gap(Ms, M),
                                 yksplit=gap(ks, ksum))


# ------------------------------------------------------------------------------------------ GPU side --
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("nhead", [1, 2])
@pytest.mark.parametrize("c2,Sk", SHAPES)
def test_zero_block_skip(c2, Sk, nhead, prec):
    from pcr_amd import engine
    blk = block(c2, nhead, Sk)
    fk, xk = blk.fk.cuda(), blk.xk.cuda()
    bf = G.bf_unit(blk.case, prec)
    state = {}
    with engine.precision(prec), torch.no_grad():
        for v in VARIANTS:
            plan = device_plan(blk, v)
            got = plan.kv(fk, xk).clone()
            assert torch.isfinite(got).all()
            assert torch.equal(plan.kv(fk, xk), got), (v, "a second launch gives other bits")
            for b in range(3):                                     # a cloud alone: B = 1
                alone = plan.kv(fk[b:b + 1].contiguous(), xk[b:b + 1].contiguous())
                assert torch.equal(alone[0], got[b]), (v, b, "a cloud alone gives other bits than in the batch")
            if v in ("a", "d"):
                with full_form():
                    full, one = plan.kv(fk, xk).clone(), plan.kv(fk[2:3].contiguous(), xk[2:3].contiguous())
                assert torch.equal(full, got) and torch.equal(one[0], got[2]), (v, "the full form gives other bits")
            state[v] = got
            ys = yardsticks(c2, nhead, Sk, v)
            M, ksum = G.unpack_state(got, D, bf)
            eM, ek = float((M - ys.M).abs().max()), float((ksum - ys.ksum).abs().max())
            bM, bk = G.state_bounds(ys, blk.case, prec)
            print("KV_SKIP c2=%d Sk=%d h=%d %s (%s) M err %.3e bound %.3e ratio %.3f | ksum err %.3e bound %.3e ratio %.3f"
                  % (c2, Sk, nhead, prec, v, eM, bM, eM / bM, ek, bk, ek / bk))
            assert eM <= bM and ek <= bk, (v, eM, bM, ek, bk)
    # -0.0 is a zero, and so (for the result) is 2^-126: the full form (e) computes what the skipped form (a) computes
    assert torch.equal(state["d"], state["a"])
    assert torch.equal(state["e"], state["a"])
    # a planted weight is seen: key channel 0 / d - 1 of K moves, and with it that channel's key sum
    ka = state["a"][:, D * D:]
    for v, row in (("c_first", 0), ("c_last", D - 1)):
        kc = state[v][:, D * D:]
        assert bool((kc[:, row] != ka[:, row]).all()), (v, "the planted weight does not show in ksum")
        others = [r for r in range(D) if r != row]
        assert torch.equal(kc[:, others], ka[:, others])
    assert not torch.equal(state["b"], state["a"])


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("Sk", [96, 160])
def test_gated_launch_skips_too(Sk, prec):
    """the GATE twins share the body: 22 virtual clouds, 2 of every 11 live (count 5, offset 3)"""
    from pcr_amd import engine, testing as T
    from mmdet3d.models.pointnet2_utils import FP_SA
    period, count, offset, sentinel = 11, 5, 3, -12345.0
    m = FP_SA(0, 64, 64, D, 64, 2)
    m.load_state_dict(T.seeded_state_dict(T.manifest_of(m), 5))
    plan = engine.AttnPlan(m.eval(), POS, torch.device("cuda"), 2, q_pos=0, k_pos=0, residual=0)
    g = torch.Generator().manual_seed(9000 + Sk)
    B = 2 * period
    fk, xk = torch.randn(B, 64, Sk, generator=g).cuda(), torch.randn(B, Sk, 3, generator=g).cuda()
    alive = (torch.arange(B, device="cuda") % period) < min(max(count - offset, 0), period)
    with engine.precision(prec), torch.no_grad():
        assert plan.live_ok()
        ref = plan.kv(fk, xk).clone()
        fv, xv = fk.clone(), xk.clone()
        fv[~alive], xv[~alive] = float("nan"), float("nan")      # nothing of a dead cloud is read
        live = (torch.tensor([count], dtype=torch.int32, device="cuda"), period, offset)
        for forced in (False, True):
            buf = torch.full_like(ref, sentinel)
            if forced:
                with full_form():
                    got = plan.kv(fv, xv, live=live, out=buf)
            else:
                got = plan.kv(fv, xv, live=live, out=buf)
            assert torch.equal(got[alive], ref[alive]), "a live cloud differs from the un-gated launch"
            assert bool((got[~alive] == sentinel).all()), "a dead cloud was written"
        # the full form of the gated twin without the switch: the (e) image, 2^-126 planted in the zero block -- the flag stays
        # off, the K half of the hidden steps runs, and the live clouds come out with the bits of the skipped form
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        w = fused_wkv(sd, planted_block("e", 64))
        plan.t["wkv"], plan.t["wkv_bf"] = engine.pack_weight(w, torch.device("cuda")), engine.pack_weight_bf(w, torch.device("cuda"))
        buf = torch.full_like(ref, sentinel)
        got = plan.kv(fv, xv, live=live, out=buf)
        assert torch.equal(got[alive], ref[alive]), "the gated full form gives other bits than the skipped form"
        assert bool((got[~alive] == sentinel).all()), "a dead cloud was written"
