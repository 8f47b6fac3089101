"""GPU: gated launches (include/pcr.h, pcr_live): the matching stages' attention launches and the pooling head read a
DEVICE pair count and do no work for the pairs beyond it.  What is held here, bit for bit throughout:
  * a live cloud's output is what the un-gated launch writes for it; a dead cloud's rows keep the sentinel they were
    filled with, and nothing of a dead cloud is read -- its q_index / kv_index entries point at an in-range "poison"
    cloud of NaNs (a wrong gate then fails the comparison, it cannot fault);
  * match_gallery(count=c)[:c] == match_gallery(pairs)[:c], the rest is dead_value exactly, also in chunks (offset);
  * a captured graph follows the count from replay to replay;
  * track_step(live_only=True) makes the decisions and the bank state of live_only=False;
  * shapes the gate does not cover are refused, never scored in full.
Shapes: Lq = Sk of 32 / 128 / 256 tokens (one block; the one-wave kv form; the multi-wave form with its barriers) and 48
(no multiple of 32: the tile kernels); period 11 -> 22 virtual clouds, no multiple of the 2 / 4 / 8 clouds of a workgroup
round; counts at both ends, inside, at and past the period; offsets 0 and 3."""
import ctypes

import numpy as np
import pytest
import torch

from pcr_amd import _lib as L
from pcr_amd import engine, testing as T

import test_gpu_attn_forms as G

pytestmark = pytest.mark.gpu

PERIOD = 11
COUNTS = [0, 1, 5, 11, 12]
OFFSETS = [0, 3]
SENTINEL = -12345.0
NOBJ = 6                      # real clouds; cloud NOBJ is the poison cloud


# ---- which gated kernels run here, spelled as attn_ref.kernel_name spells a gated twin: (kv, apply, pooled apply or None).
# tests/test_attn_ref_cpu.py holds every entry to what the library reports for the block, and every gated instantiation the
# dispatch can reach to an entry.  GATED: (Ln, mode) of test_gated_attention_launches (corss_attention(64, 2)); TWINS:
# (kind, heads, trailing conv, Ln, mode) of test_gated_twins_beyond_the_matching_stages, kinds as tests/test_gpu_attn_forms.py's.
_KS_F, _KS_1W, _KS_B = ("attn_kv_stream64_kernel<%s, true>" % a for a in ("%s, false, 4, false", "%s, true, 4, true", "%s, true, 4, false"))
_KO3_G, _AT_G = "attn_kv_kernel_o3_live<2, 1, 1, 1>", "attn_apply_kernel<2, 1, true>"
_AS_G = "attn_apply_stream64_kernel<%s, 4, %d, 2, 2, %s, true>"
_ASX_G, _ASP_G = _AS_G % ("false", 0, "false"), _AS_G % ("false", 0, "true")
GATED = {
    (32, "bf16x3"): (_KS_1W % "true", _ASX_G, _ASP_G), (128, "bf16x3"): (_KS_1W % "true", _ASX_G, _ASP_G),
    (256, "bf16x3"): (_KS_B % "true", _ASX_G, _ASP_G), (48, "bf16x3"): (_KO3_G, _AT_G, None),
    (32, "f32"): (_KS_F % "true", _AT_G, None), (128, "f32"): (_KS_F % "true", _AT_G, None),
    (256, "f32"): (_KS_F % "true", _AT_G, None), (48, "f32"): (_KO3_G, _AT_G, None),
}
TWINS = {
    ("cross", 1, 0, 32, "bf16x3"): (_KS_1W % "false", _ASX_G, None),
    ("cross", 1, 0, 160, "bf16x3"): (_KS_B % "false", _ASX_G, None),
    ("cross", 1, 0, 32, "f32"): (_KS_F % "false", _AT_G, None),
    ("fpq", 2, 0, 32, "bf16x3"): (_KS_1W % "true", _AS_G % ("true", 0, "false"), None),
    ("fpq", 2, 128, 32, "bf16x3"): (_KS_1W % "true", _AS_G % ("true", 4, "false"), None),
    ("fp", 2, 128, 32, "bf16x3"): (_KS_1W % "true", _AS_G % ("false", 4, "false"), None),
}


def gated_case(kind, nhead, cfinal, Ln):
    """the d = c1 = c2 = cout = 64 block of a GATED / TWINS row as a row of tests/test_gpu_attn_forms.py"""
    import test_gpu_attn_forms as G
    return G.Case("gated-%s-h%d-f%d-L%d" % (kind, nhead, cfinal, Ln), kind, (64, 64, 64, 64), nhead, 2 * PERIOD, Ln, Ln, cfinal)


def live_pairs(count, offset, period=PERIOD):
    return min(max(count - offset, 0), period)


def live_mask(count, offset, B, period=PERIOD):
    """(B,) bool, on the device: cloud b is live iff b % period < clamp(count - offset, 0, period)"""
    return (torch.arange(B, device="cuda") % period) < live_pairs(count, offset, period)


def dev_count(c):
    return torch.tensor([c], dtype=torch.int32, device="cuda")


def assert_gated(got, ref, alive, what):
    assert torch.equal(got[alive], ref[alive]), "%s: a live cloud differs from the un-gated launch" % (what,)
    dead = got[~alive]
    assert bool((dead == SENTINEL).all()), "%s: a dead cloud was written" % (what,)


@pytest.fixture(scope="module")
def cross_block():
    from mmdet3d.models.attention import corss_attention
    m = corss_attention(64, 2)
    m.load_state_dict(T.seeded_state_dict(T.manifest_of(m), 3))
    return m.cuda().eval()


# ---- 1. kernel level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("Ln", [32, 128, 256, 48])
def test_gated_attention_launches(cross_block, Ln, prec):
    plan = cross_block.plan(torch.device("cuda"))
    g = torch.Generator().manual_seed(1000 + Ln)
    B = 2 * PERIOD
    feat = torch.randn(NOBJ + 1, 64, Ln, generator=g).cuda()
    xyz = torch.randn(NOBJ + 1, Ln, 3, generator=g).cuda()
    feat[NOBJ], xyz[NOBJ] = float("nan"), float("nan")
    q_idx = torch.randint(0, NOBJ, (B,), generator=g).to(torch.int32).cuda()
    k_idx = torch.randint(0, NOBJ, (B,), generator=g).to(torch.int32).cuda()
    featv = torch.randn(B, 64, Ln, generator=g).cuda()           # the key side of a stage-2 launch: one cloud per virtual cloud
    xyzv = torch.randn(B, Ln, 3, generator=g).cuda()
    poison = torch.full((B,), NOBJ, dtype=torch.int32, device="cuda")
    with engine.precision(prec), torch.no_grad():
        assert plan.live_ok()
        pooled = plan.pool_ok(Ln, Ln)
        assert pooled == (prec == "bf16x3" and Ln % 32 == 0)
        kv_obj = plan.kv(feat, xyz)                              # per object (the poison cloud's state is NaN)
        ref_kv = plan.kv(featv, xyzv)
        ref_out = plan.apply(feat, None, kv_obj, Ln, kv_index=k_idx, q_index=q_idx, n_out=B)
        ref_pool = plan.apply(feat, None, kv_obj, Ln, kv_index=k_idx, q_index=q_idx, n_out=B, pooled=True) if pooled else None
        assert not torch.isnan(ref_kv).any() and not torch.isnan(ref_out).any()
        for count in COUNTS:
            for offset in OFFSETS:
                what = "L=%d %s count=%d offset=%d" % (Ln, prec, count, offset)
                alive = live_mask(count, offset, B)
                live = (dev_count(count), PERIOD, offset)
                # kv: the features of the dead clouds are NaN
                fv, xv = featv.clone(), xyzv.clone()
                fv[~alive], xv[~alive] = float("nan"), float("nan")
                buf = torch.full_like(ref_kv, SENTINEL)
                got = plan.kv(fv, xv, live=live, out=buf)
                assert got is buf
                assert_gated(got, ref_kv, alive, what + " kv")
                # apply: the index entries of the dead clouds point at the poison cloud
                qi, ki = torch.where(alive, q_idx, poison), torch.where(alive, k_idx, poison)
                buf = torch.full_like(ref_out, SENTINEL)
                got = plan.apply(feat, None, kv_obj, Ln, kv_index=ki, q_index=qi, n_out=B, live=live, out=buf)
                assert_gated(got, ref_out, alive, what + " apply")
                if pooled:
                    buf = torch.full_like(ref_pool, SENTINEL)
                    got = plan.apply(feat, None, kv_obj, Ln, kv_index=ki, q_index=qi, n_out=B, pooled=True, live=live, out=buf)
                    assert_gated(got, ref_pool, alive, what + " pooled apply")
        if pooled:     # without a buffer of the caller's, the pooled rows of dead clouds are zeros (read in full downstream)
            got = plan.apply(feat, None, kv_obj, Ln, kv_index=k_idx, q_index=q_idx, n_out=B, pooled=True,
                             live=(dev_count(5), PERIOD, 3))
            alive = live_mask(5, 3, B)
            assert torch.equal(got[alive], ref_pool[alive]) and bool((got[~alive] == 0).all())
        # live=None is the un-gated call
        assert torch.equal(plan.kv(featv, xyzv, live=None), ref_kv)
        # the blocks of gated launches get the table's gated twins
        live = (dev_count(5), PERIOD, 3)
        with G.launched_blocks() as seen:
            plan.kv(featv, xyzv, live=live, out=torch.full_like(ref_kv, SENTINEL))
            plan.apply(feat, None, kv_obj, Ln, kv_index=k_idx, q_index=q_idx, n_out=B, live=live, out=torch.full_like(ref_out, SENTINEL))
            if pooled:
                plan.apply(feat, None, kv_obj, Ln, kv_index=k_idx, q_index=q_idx, n_out=B, pooled=True, live=live)
        assert gated_kernels(seen, live) == GATED[Ln, prec]


def gated_kernels(seen, live):
    """(kv, apply, pooled apply or None) the library reports for the gated blocks in `seen` (launched_blocks)"""
    lv = ctypes.byref(engine._live_block(live))
    names = [G.reported(seen["kv"][0], 0, lv)[0]] + [G.reported(p, 1, lv)[0] for p in seen["apply"]]
    return tuple(names + [None] * (3 - len(names)))


@pytest.mark.parametrize("row", sorted(TWINS), ids=lambda r: "%s-h%d-f%d-L%d-%s" % r)
def test_gated_twins_beyond_the_matching_stages(row):
    """the gated instantiations the matching stages' corss_attention(64, 2) does not reach -- one head, q_pos, a trailing
    conv -- through engine.AttnPlan itself: a live cloud gets the un-gated launch's bits, a dead cloud (NaN features) is
    neither read nor written.  B = 22 clouds of 32 tokens (160: the multi-wave kv form)."""
    kind, nhead, cfinal, Ln, prec = row
    case = gated_case(kind, nhead, cfinal, Ln)
    plan = G.host_plan(case, "cuda")
    g = torch.Generator().manual_seed(2000 + Ln + nhead)
    B = case.B
    feat, xyz = torch.randn(B, 64, Ln, generator=g).cuda(), torch.randn(B, Ln, 3, generator=g).cuda()
    xq = lambda x: x if plan.q_pos else None      # noqa: E731
    with engine.precision(prec), torch.no_grad():
        assert plan.live_ok()
        ref_kv = plan.kv(feat, xyz)
        ref_out = plan.apply(feat, xq(xyz), ref_kv, Ln)
        assert not torch.isnan(ref_kv).any() and not torch.isnan(ref_out).any()
        for count, offset in ((5, 3), (12, 0), (0, 0)):
            what = "%s count=%d offset=%d" % (case.name, count, offset)
            alive, live = live_mask(count, offset, B), (dev_count(count), PERIOD, offset)
            fv, xv = feat.clone(), xyz.clone()
            fv[~alive], xv[~alive] = float("nan"), float("nan")
            with G.launched_blocks() as seen:
                got = plan.kv(fv, xv, live=live, out=torch.full_like(ref_kv, SENTINEL))
                assert_gated(got, ref_kv, alive, what + " kv")
                got = plan.apply(fv, xq(xv), ref_kv, Ln, live=live, out=torch.full_like(ref_out, SENTINEL))
                assert_gated(got, ref_out, alive, what + " apply")
            assert gated_kernels(seen, live) == TWINS[row]


# ---- 2. head --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    """the toy Point-Transformer of test_track_step_equals_the_pieces_driven_by_hand (n = 128), calibrated once, with a
    gallery of NOBJ encoded objects and a poison object of NaNs behind them"""
    import bench
    n = 128
    model, _ = bench.build_pt_model([n, 64, 32])
    clouds = T.synthetic_clouds(NOBJ + 2, n + 20, seed=31, kind="box").cuda()
    with torch.no_grad():
        model.calibrate_precision(clouds[:NOBJ // 2 + 1], clouds[NOBJ // 2 + 1:])
        xyz, h = model.forward_inference(clouds[:NOBJ + 1])[:2]
    h, xyz = h.contiguous().clone(), xyz.contiguous().clone()
    h[NOBJ], xyz[NOBJ] = float("nan"), float("nan")
    return model, h, xyz


def test_gated_pool_head(toy):
    model, _, _ = toy
    head = model._head(torch.device("cuda"))
    g = torch.Generator().manual_seed(5)
    P, C, Ln = PERIOD, head.n // 2, 128
    o = torch.randn(2 * P, C, Ln, generator=g).cuda()
    with torch.no_grad():
        ref_logits, ref_pooled = head.run(o, want_pooled=True)
        for count in COUNTS:
            for offset in OFFSETS:
                alive = live_mask(count, offset, P)
                od = o.clone()
                od[torch.cat([~alive, ~alive])] = float("nan")
                live = (dev_count(count), P, offset)
                logits, pooled = head.run(od, want_pooled=True, live=live, dead_value=-7.5)
                assert torch.equal(logits[alive], ref_logits[alive]) and torch.equal(pooled[alive], ref_pooled[alive])
                assert bool((logits[~alive] == -7.5).all()) and bool((pooled[~alive] == 0).all())
                assert torch.equal(head.run(od, live=live)[~alive], torch.zeros(int((~alive).sum()), device="cuda"))
        assert torch.equal(head.run(o, live=None), ref_logits)


# ---- 3. model level -------------------------------------------------------------------------------------------------------
NPAIRS = 12


def toy_pairs(seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, NOBJ, (NPAIRS, 2), generator=g).cuda()


def poisoned(pairs, count):
    p = pairs.clone()
    p[count:] = NOBJ
    return p


@pytest.mark.parametrize("prec,chunk", [("bf16x3", None), ("bf16x3", 7), ("f32", None), ("f32", 7)])
def test_match_gallery_scores_the_live_pairs_only(toy, prec, chunk, monkeypatch):
    model, h, xyz = toy
    pairs = toy_pairs()
    with engine.precision(prec), torch.no_grad():
        ref = model.match_gallery(h, xyz, pairs)
        assert ref.shape == (NPAIRS,) and not torch.isnan(ref).any()
        if chunk is not None:
            monkeypatch.setattr(type(model), "GALLERY_CHUNK", chunk)
        for count in COUNTS:
            c = min(count, NPAIRS)
            got = model.match_gallery(h, xyz, poisoned(pairs, c), count=dev_count(count), dead_value=-3.25)
            assert got.shape == ref.shape
            assert torch.equal(got[:c], ref[:c]), (prec, chunk, count)
            assert bool((got[c:] == -3.25).all()), (prec, chunk, count)
        got = model.match_gallery(h, xyz, poisoned(pairs, 5), count=dev_count(5))
        assert torch.equal(got[:5], ref[:5]) and bool((got[5:] == 0).all())


# ---- 4. graph -------------------------------------------------------------------------------------------------------------
def test_a_captured_match_follows_the_device_count(toy):
    model, h, xyz = toy
    pairs = toy_pairs(seed=10)
    t = dev_count(NPAIRS)
    with torch.no_grad():
        model.match_gallery(h, xyz, pairs, count=t, dead_value=-1.0)        # warm: nothing is loaded inside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model.match_gallery(h, xyz, pairs, count=t, dead_value=-1.0)
        for c in (3, 0, NPAIRS):
            t.fill_(c)
            graph.replay()
            torch.cuda.synchronize()
            got = out.clone()
            eager = model.match_gallery(h, xyz, pairs, count=dev_count(c), dead_value=-1.0)
            assert torch.equal(got, eager), c
            assert bool((got[c:] == -1.0).all())


# ---- 5. frame -------------------------------------------------------------------------------------------------------------
def test_track_step_live_only_makes_the_same_frame(toy):
    from pcr_amd import tracks as TR
    from test_gpu_tracks import LIMIT, THRESH, dev, host, same_bits, toy_frames
    model = toy[0]
    C, D, M, W, n = 16, 8, 6, 9, 128
    frames = toy_frames(3, M, n + 20, W, seed=31)
    shift = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0], np.float32)
    back = np.array([1, 0, 0, -0.5, 0, 1, 0, 0.25, 0, 0, 1, 0], np.float32)
    banks = [TR.TrackBank(C, D, feat_shape=(64, n), box_width=W) for _ in range(2)]
    with torch.no_grad():
        for f, (pts, boxes, labels, scores) in enumerate(frames):
            outs = [model.track_step(bank, dev(pts), dev(boxes), dev(labels), dev(scores), carry=dev(shift),
                                     carry_inv=dev(back), crop_args=dict(seed=5 + f), frame_limit=LIMIT,
                                     suppress_threshold=THRESH, live_only=lo) for bank, lo in zip(banks, (False, True))]
            full, live = outs
            cnt = int(full["count"][0])
            assert sorted(full) == sorted(live)
            for k in full:
                if full[k] is None:
                    assert live[k] is None
                elif k == "logits":
                    assert same_bits(host(full[k])[:cnt], host(live[k])[:cnt]), f
                    assert (host(live[k])[cnt:] == 0).all(), f
                else:
                    assert same_bits(host(full[k]), host(live[k])), (f, k)
            sa, sb = banks[0].state(), banks[1].state()
            for k in sa:
                assert same_bits(host(sa[k]), host(sb[k])), (f, k)
            assert same_bits(host(banks[0].feats), host(banks[1].feats)) and same_bits(host(banks[0].xyz), host(banks[1].xyz))
            if f:
                assert 0 < cnt < C * D                   # some pairs are live, most of the list is padding


# ---- 6. refusal -----------------------------------------------------------------------------------------------------------
def test_shapes_outside_the_gate_are_refused():
    from mmdet3d.models.attention import corss_attention
    m = corss_attention(128, 2)
    m.load_state_dict(T.seeded_state_dict(T.manifest_of(m), 3))
    plan = m.cuda().eval().plan(torch.device("cuda"))
    assert not plan.live_ok()
    g = torch.Generator().manual_seed(2)
    feat, xyz = torch.randn(4, 128, 32, generator=g).cuda(), torch.randn(4, 32, 3, generator=g).cuda()
    live = (dev_count(1), 2, 0)
    kv = plan.kv(feat, xyz)
    buf = torch.full_like(kv, SENTINEL)
    with pytest.raises(L.PcrError):
        plan.kv(feat, xyz, live=live, out=buf)
    out = torch.full((4, 128, 32), SENTINEL, device="cuda")
    with pytest.raises(L.PcrError):
        plan.apply(feat, None, kv, 32, live=live, out=out)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((out == SENTINEL).all())        # refused, not scored in full
    # the entry point's own status
    p = plan._params(4, 1, 32, feat, xyz, feat, xyz, buf, buf)
    lv = engine._live_block(live)
    assert L.load().pcr_attn_live_ok(ctypes.byref(p)) == 0
    assert L.load().pcr_attn_kv_live_f32(ctypes.byref(p), ctypes.byref(lv), L.stream_ptr()) == 1      # PCR_ERR_INVALID
    # the count is an int32 device tensor, nothing else
    with pytest.raises(L.PcrError):
        engine._live_block((dev_count(1).float(), 2, 0))
