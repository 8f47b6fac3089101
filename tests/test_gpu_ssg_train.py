"""GPU: PointNet++ SSG in training mode.  A PointSAModule with `hip_training` on (sampler, gather_points, ball query,
pcr_amd.train_ops.SaGroupTrain) against the float64 restatement of tests/ssg_train_ref.py on conditioned inputs (zero
marginal float64 decisions, shown without a device by test_ssg_train_ref_cpu.py), then a ReIDNet with the
PointNet2SSG(trainable=True) backbone behind the unchanged train_step / Trainer.

Bounds: BatchNorm compositions BN_BOUND = 2e-5 (`_rel`, each tensor under its own norm), BF_BOUND = 3e-5 where
TRAIN_PRECISION puts the 128 x 128 backward on split bf16; selections and indices exact.  The whole step is held by the
rule of test_gpu_train_variants.py: a gradient is within grad_floor of the float32 restatement's, or no further from the
float64 one than max(grad_floor, twice the float32 restatement's own distance)."""
import copy
import json
import math

import numpy as np
import pytest
import torch

import ssg_train_ref as G
from test_ssg_train_ref_cpu import model_cfg, model_inputs, model_state_dict

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def _vs(got, want):
    return _rel(got.detach().cpu().to(F64), want.detach().to(F64))


# ------------------------------------------------------------------------------------------ the module --
def _module(i):
    from mmdet3d.ops import PointSAModule
    c, case = G.MODULE_CASES[i], G.module_case(i)
    m = PointSAModule(mlp_channels=list(c["mlp"]), num_point=c["S"], radius=c["r"], num_sample=c["K"])
    m.load_state_dict(case["sd"], strict=True)
    m.hip_training = True
    return m.cuda().train(), c, case


@pytest.mark.parametrize("i", range(len(G.MODULE_CASES)))
def test_sa_module_trains_against_float64(i):
    """output, winning slots, running statistics, num_batches_tracked, every conv / BatchNorm gradient and the feature
    gradient of one training forward + backward; then .eval() on the updated module against model_oracle.ssg_sa_layer on its new state
    dict.
    Observed worst _rel on the MI355X: output 2.6e-7 / 2.8e-7 / 4.1e-7 / 2.8e-7, running statistics <= 4.9e-8, gradients
    8.8e-7 / 7.0e-7, on the split-bf16 128 x 128 backward of the third case (bound BF_BOUND) 6.2e-6, on the wave-autonomous
    kernels of the fourth 9.1e-7; every live winner on the float64 slot."""
    import model_oracle as MO
    from pcr_amd import train_ops as TO
    m, c, case = _module(i)
    bf = TO._bwd_bf() and c["mlp"][1:3] == [128, 128]
    bound = G.BF_BOUND if bf else G.BN_BOUND
    assert G.count_marginals(G.layers_of(case["sd"]), case["xyz"], case["feats"], case["idx"], case["centre"]) == 0
    xyz = case["xyz"].cuda()
    feats = None if case["feats"] is None else case["feats"].cuda().requires_grad_(True)
    from pcr_amd import _lib, engine
    # (the fourth case runs layers 2 and 3 on the wave-autonomous kernels, layer 3 with the max over K inside its launch:
    # their block threshold is lowered for it, and the launch record must then hold no separate pooling launch)
    old = _lib.load().pcr_set_stream_min_blocks(0) if c.get("stream") else None
    engine.PROFILE = []
    try:
        new_xyz, out, indices = m(xyz, feats)
        saved = [t for t in out.grad_fn.saved_tensors if t is not None and t.dtype == torch.int32]
        (out * case["w"].cuda()).sum().backward()
        launched = [rec[0].split("[")[0] for rec in engine.PROFILE]
    finally:
        engine.PROFILE = None
        if old is not None:
            _lib.load().pcr_set_stream_min_blocks(old)
    assert ("sa_pool_fwd" in launched) != bool(c.get("stream")), launched
    assert "sa_l1c_fwd" in launched and "sa_l1c_bwd" in launched
    # indices and centres: exact
    assert torch.equal(indices.cpu().to(torch.int32), case["centre"])
    assert torch.equal(new_xyz.cpu(), torch.gather(case["xyz"], 1, case["centre"].long().unsqueeze(2).expand(-1, -1, 3)))
    assert not new_xyz.requires_grad and tuple(out.shape) == (c["B"], c["mlp"][-1], c["S"])
    assert any(tuple(t.shape) == tuple(case["idx"].shape) and torch.equal(t.cpu(), case["idx"]) for t in saved)
    want = G.scale_outputs(case["sd"], case["xyz"], case["feats"], case["idx"], case["centre"], case["w"])
    arg = [t for t in saved if tuple(t.shape) == tuple(out.shape)][-1].cpu().long()
    live = want["out"] > 0
    # the winning slot wherever a gradient passes: exact, and never a copy (a copy holds its row 0's bits and comes later)
    assert torch.equal(arg[live], want["arg"][live])
    assert bool((arg < G.genuine_count(case["idx"]).unsqueeze(1))[live].all())
    worst = dict(out=_vs(out, want["out"]))
    mlp = m.mlps[0]
    for j, layer in enumerate(mlp.children()):
        assert layer.conv.bias is None
        for name, p in (("conv.weight", layer.conv.weight), ("bn.weight", layer.bn.weight), ("bn.bias", layer.bn.bias)):
            worst["grad:layer%d.%s" % (j, name)] = _vs(p.grad, want["grad:layer%d.%s" % (j, name)])
        for name, buf in (("running_mean", layer.bn.running_mean), ("running_var", layer.bn.running_var)):
            worst["layer%d.bn.%s" % (j, name)] = _vs(buf, want["layer%d.bn.%s" % (j, name)])
        assert int(layer.bn.num_batches_tracked) == 1
    if feats is not None:
        worst["grad:feats"] = _vs(feats.grad, want["grad:feats"])
    print(json.dumps(dict(op="PointSAModule.train", case=i, bound=bound, worst=worst)))
    assert all(math.isfinite(v) for v in worst.values()), worst
    assert max(worst.values()) < bound, worst
    # .eval() picks the new running statistics up (engine.param_version keys)
    m.eval()
    with torch.no_grad():
        _, out_eval, _ = m(xyz, None if feats is None else feats.detach())
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        _, ref = MO.ssg_sa_layer(sd, case["xyz"], case["feats"], c["S"], c["r"], c["K"])
    assert not torch.equal(sd["mlps.0.layer0.bn.running_mean"], case["sd"]["mlps.0.layer0.bn.running_mean"])
    assert float((out_eval.cpu() - ref).abs().max()) < 5e-5


def test_sa_module_forward_twice_gives_the_same_bits():
    outs = []
    for _ in range(2):
        m, c, case = _module(1)
        f = case["feats"].cuda().requires_grad_(True)
        _, out, _ = m(case["xyz"].cuda(), f)
        (out * case["w"].cuda()).sum().backward()
        outs.append([out.detach(), f.grad] + [p.grad for p in m.parameters()] + [b for b in m.buffers()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- the model --
LOSSES = dict(kl=False, match=True, cls=False, shape=False, fp=False, triplet=False)


def _model():
    from mmdet3d.models import build_model
    cfg = model_cfg()
    cfg["losses_to_use"] = dict(LOSSES)
    m = build_model(cfg)
    m.load_state_dict(model_state_dict(), strict=True)
    return m.cuda().train()


def _data(dev="cuda"):
    s1, s2, _ = model_inputs()
    n = s1.shape[0]
    ids1 = torch.arange(n)
    ids2 = torch.where(ids1 < n // 2, ids1, ids1 + 100)
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    return dict(sparse_1=list(s1.to(dev)), sparse_2=list(s2.to(dev)), dense_1=list(s1.to(dev)), dense_2=list(s2.to(dev)),
                label_1=[zero] * n, label_2=[zero] * n,
                id_1=[i.view(1).to(dev) for i in ids1], id_2=[i.view(1).to(dev) for i in ids2])


@pytest.fixture(scope="module")
def step_refs():
    """the float64 restatement of the step and the float32 one (the yardstick), computed once"""
    s1, s2, match = model_inputs()
    sd = model_state_dict()
    return {dt: G.step_ref(sd, s1, s2, match, dict(G.MODEL_BACKBONE), G.oracle_query, dt) for dt in (F64, torch.float32)}


def test_train_step_matches_the_float64_restatement(step_refs, grad_floor):
    """loss and every gradient of ReIDNet.train_step with the trainable SSG backbone; no parameter is left without a
    gradient; two runs from one state give the same bits.  Observed on the MI355X: loss 1.05396307 against 1.05396294;
    worst gradient 8.2e-6 ("f32") / 1.3e-5 ("bf16x3") of its tensor's scale from the float32 restatement, 1.3e-5 from
    float64, the float32 restatement's own distance 8.5e-6."""
    loss64, g64, _, _ = step_refs[F64]
    _, g32, _, _ = step_refs[torch.float32]
    m = _model()
    twin = copy.deepcopy(m)
    runs = []
    for model in (m, twin):
        out = model.train_step(_data(), None)
        out["loss"].backward()
        runs.append([out["loss"].detach()] + [p.grad for _, p in sorted(model.named_parameters())])
    params = dict(m.named_parameters())
    assert sorted(k for k, p in params.items() if p.grad is None) == []
    assert sorted(params) == sorted(g64)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    loss = float(runs[0][0])
    vs32, own, vs64 = {}, {}, {}
    for k, p in params.items():
        got = p.grad.detach().cpu().to(F64)
        scale = max(1e-3, float(g32[k].abs().max()))
        vs32[k] = float((got - g32[k].to(F64)).abs().max()) / scale
        own[k] = float((g32[k].to(F64) - g64[k]).abs().max()) / scale
        vs64[k] = float((got - g64[k]).abs().max()) / scale
    print(json.dumps(dict(loss=loss, loss64=float(loss64), worst_vs32=max(vs32.values()), worst_vs64=max(vs64.values()),
                          worst_own=max(own.values()))))
    assert abs(loss - float(loss64)) < 1e-4
    for k in vs32:
        assert vs32[k] < grad_floor or vs64[k] < max(grad_floor, 2.0 * own[k]), (k, vs32[k], vs64[k], own[k])


def test_trainer_steps_decrease_the_loss_and_eval_sees_the_new_weights():
    import model_oracle as MO
    from pcr_amd import train
    m = _model()
    tr = train.Trainer(m, max_iters=40, lr=3e-4, grad_clip=1.0)
    data = _data()
    losses = [float(tr.step(data)["loss"].detach()) for _ in range(12)]
    print(json.dumps(dict(losses=losses)))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    m.eval()
    s1, s2, _ = model_inputs()
    with torch.no_grad():
        xyz1, xyz2, h1, h2 = m.siamese_forward(s1.cuda(), s2.cuda())
        logits = m.match_forward_inference(h1, h2, xyz1, xyz2).cpu()
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        want = MO.ssg_pairs(sd, s1, s2, **{k: G.MODEL_BACKBONE[k] for k in ("num_points", "radii", "num_samples")})
    assert float((logits - want).abs().max()) < 1e-4


def test_eval_after_one_step_matches_the_oracle_on_the_new_state_dict():
    import model_oracle as MO
    m = _model()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    out = m.train_step(_data(), None)
    out["loss"].backward()
    m.eval()
    assert not torch.equal(before["backbone.SA_modules.0.mlps.0.layer0.bn.running_mean"],
                           m.state_dict()["backbone.SA_modules.0.mlps.0.layer0.bn.running_mean"])
    s1, s2, _ = model_inputs()
    with torch.no_grad():
        xyz1, xyz2, h1, h2 = m.siamese_forward(s1.cuda(), s2.cuda())
        logits = m.match_forward_inference(h1, h2, xyz1, xyz2).cpu()
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        want = MO.ssg_pairs(sd, s1, s2, **{k: G.MODEL_BACKBONE[k] for k in ("num_points", "radii", "num_samples")})
    assert float((logits - want).abs().max()) < 1e-4


def test_trainer_graph_mode_gives_the_eager_bits():
    from pcr_amd import train
    runs = {}
    for mode in (False, True):
        m = _model()
        tr = train.Trainer(m, max_iters=12, lr=1e-3, grad_clip=1.0, graph=mode)
        data = _data()
        rec = []
        for _ in range(6):
            out = tr.step(data)
            rec.append((float(out["loss"].detach()), float(out["grad_norm"])))
        assert tr.graph == mode                                    # (the capture did not fall back)
        runs[mode] = (rec, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    assert runs[False][0] == runs[True][0], (runs[False][0], runs[True][0])
    for k, v in runs[False][1].items():
        assert torch.equal(v, runs[True][1][k]), k
