"""GPU: training on all pairs of a batch (`sampling = 'cartesian'`) and on a pair list (`ReIDNet.match_gallery_train`).

* The cartesian train_step of three configs is pinned to what the REFERENCE's own cartesian branch produced
  (tools/make_cartesian_golden.py -> tests/golden/train_step_cartesian_<tag>_n128.npz), by the rule of
  test_train_step_of_other_configs_matches_the_reference: a gradient within grad_floor of the reference's float32 one,
  or no further from the float64 one than max(grad_floor, twice the reference's own float32 error).  match_loss IS the
  loss here (alpha['match'] = 1, no other loss), so it is held to the loss's bound; the other five logged values are
  counts and an accuracy over 16 slots and must be equal.
* match_gallery_train on the point-cat model is held to oracle/model_oracle.match in float64 with autograd; the yardstick
  is the explicit route (train_graph.match_logits on h[i], h[j]): at most twice its error, floor 1e-5 of scale.
* Padding leaves the live slots alone; sampling = None keeps the paired step; the Trainer trains, eager and captured."""
import json

import numpy as np
import pytest
import torch

import pair_list_ref as PL
from conftest import load_golden
from pcr_amd import testing as T
from test_gpu_config_variants import BASELINE, _pt_mul
from test_gpu_train_variants import STNET, _build

pytestmark = pytest.mark.gpu

F64 = torch.float64
CASES = {"pt": (_pt_mul(1, 64, 8), "pt"), "stnet": (STNET, "pt"), "baseline": (BASELINE, "pt_baseline")}
LOGGED = ("match_acc", "num_preds_0", "num_preds_1", "num_gt_0", "num_gt_1")


def _data(meta, dev="cuda"):
    b = meta["pairs"]
    s1, s2 = T.synthetic_pairs(b, meta["n"], seed=meta["input_seed"], kind="randn")
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    return dict(sparse_1=list(s1.to(dev)), sparse_2=list(s2.to(dev)), dense_1=list(s1.to(dev)), dense_2=list(s2.to(dev)),
                label_1=[zero] * b, label_2=[zero] * b,
                id_1=[torch.tensor([i], device=dev) for i in meta["id_1"]],
                id_2=[torch.tensor([i], device=dev) for i in meta["id_2"]])


@pytest.mark.parametrize("tag", ["pt", "stnet", "baseline"])
def test_cartesian_train_step_matches_the_reference(tag, grad_floor):
    g = load_golden("train_step_cartesian_%s_n128" % tag)
    cfg, manifest = CASES[tag]
    m = _build(cfg, manifest)
    m.sampling = "cartesian"
    m.train()
    out = m.train_step(_data(g["meta"]), None)
    loss = float(out["loss"])
    out["loss"].backward()
    assert out["num_samples"] == g["meta"]["pairs"]
    params = dict(m.named_parameters())
    worst, ref_own, vs64 = {}, {}, {}
    for k in g:
        if k.startswith("grad:"):
            got = params[k[5:]].grad.cpu().numpy()
            scale = max(1e-3, float(np.abs(g[k]).max()))
            g64 = g["grad64:" + k[5:]]
            worst[k[5:]] = float(np.abs(got - g[k]).max()) / scale
            ref_own[k[5:]] = float(np.abs(g[k] - g64).max()) / scale
            vs64[k[5:]] = float(np.abs(got - g64).max()) / scale
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    logged = {k: float(out["log_vars"][k]) for k in LOGGED + ("match_loss",)}
    print(json.dumps(dict(tag=tag, loss=loss, ref_loss=float(g["loss"]), grad_norm=gn, ref_grad_norm=float(g["grad_norm"]),
                          logged=logged, vs_ref32=worst, ref32_vs_ref64=ref_own, vs_ref64=vs64)))
    assert abs(loss - float(g["loss"])) < 1e-4
    assert abs(logged["match_loss"] - float(g["match_loss"])) < 1e-4
    for k in LOGGED:
        assert logged[k] == float(g[k]), (k, logged[k], float(g[k]))
    for k in worst:
        assert worst[k] < grad_floor or vs64[k] < max(grad_floor, 2.0 * ref_own[k]), (k, worst[k], vs64[k], ref_own[k])
    assert gn == pytest.approx(float(g["grad_norm"]), rel=2e-3)
    no_grad = sorted(k for k, p in params.items() if p.grad is None)
    assert no_grad == sorted(json.loads(str(g["no_grad_params"])))


# ------------------------------------------------------------------------------------- match_gallery_train --
M, N, CAP, COUNT = 6, 128, 9, 7
# object 1 in four slots, a self-pair, both orders of (0, 2); the dead slots name object 5, which no live slot does
PAIRS = [[0, 1], [2, 1], [3, 3], [1, 4], [0, 2], [2, 0], [4, 1], [5, 5], [5, 0]]
MATCH = [1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0]
FLOOR = 1e-5


def _matching(params):
    return {k: p for k, p in params if k.startswith(("cross_stage", "match_head"))}


@pytest.fixture(scope="module")
def gallery_runs():
    """the list route (padded and truncated), the explicit route and the float64 oracle on one set of objects, once"""
    import model_oracle as MO
    from pcr_amd import train_graph as TG
    m = _build(_pt_mul(1, 64, 8), "pt").train()
    gen = torch.Generator().manual_seed(17)
    h0 = torch.randn(M, 64, N, generator=gen)
    xyz = torch.randn(M, N, 3, generator=gen)
    pairs = torch.tensor(PAIRS, dtype=torch.int32)
    match = torch.tensor(MATCH)
    i, j = pairs[:COUNT, 0].long(), pairs[:COUNT, 1].long()

    def grads():
        out = {k: p.grad.detach().cpu().clone() for k, p in _matching(m.named_parameters()).items() if p.grad is not None}
        m.zero_grad(set_to_none=True)
        return out

    runs = {}
    for name, (pl, cnt) in dict(padded=(pairs, torch.tensor([COUNT], dtype=torch.int32, device="cuda")),
                                truncated=(pairs[:COUNT], None)).items():
        h = h0.cuda().requires_grad_(True)
        logits = m.match_gallery_train(h, xyz.cuda(), pl.cuda(), cnt)
        loss = TG.list_loss(logits, match[:pl.shape[0]].cuda(), cnt)
        loss.backward()
        runs[name] = dict(logits=logits.detach().cpu(), loss=float(loss), dh=h.grad.cpu(), params=grads())
    # the explicit route: the operands of every live slot gathered by hand, their gradients added per object in f32
    hi, hj = (h0[ix].cuda().requires_grad_(True) for ix in (i, j))
    logits = TG.match_logits(m, hi, xyz[i].cuda(), hj, xyz[j].cuda())[0]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, match[:COUNT].cuda())
    loss.backward()
    dh = sum(PL.index_sum_seq_f32(t.grad.cpu().numpy().reshape(COUNT, -1), ix.numpy(), None, M) for t, ix in ((hi, i), (hj, j)))
    runs["explicit"] = dict(logits=logits.detach().cpu(), loss=float(loss), dh=torch.from_numpy(dh).reshape(M, 64, N),
                            params=grads())
    # float64, autograd through the oracle's composition
    sd = {k: v.detach().cpu().to(F64).requires_grad_(k.startswith(("cross_stage", "match_head")))
          for k, v in m.state_dict().items() if v.is_floating_point()}
    h64 = h0.to(F64).requires_grad_(True)
    x64 = xyz.to(F64)
    logits = MO.match(sd, h64[i], x64[i], h64[j], x64[j])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, match[:COUNT].to(F64))
    loss.backward()
    runs["oracle"] = dict(logits=logits.detach(), loss=float(loss), dh=h64.grad,
                          params={k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None})
    return runs


def _rel(got, want):
    return float((got.to(F64) - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _errors(run, oracle, live):
    e = dict(logits=_rel(run["logits"][:live], oracle["logits"]), dh=_rel(run["dh"], oracle["dh"]))
    assert sorted(run["params"]) == sorted(oracle["params"])
    e.update({k: _rel(run["params"][k], g) for k, g in oracle["params"].items()})
    return e


@pytest.mark.parametrize("route", ["padded", "truncated"])
def test_match_gallery_train_is_no_further_from_float64_than_the_explicit_route(gallery_runs, route):
    oracle = gallery_runs["oracle"]
    assert len(oracle["params"]) >= 20
    new, old = _errors(gallery_runs[route], oracle, COUNT), _errors(gallery_runs["explicit"], oracle, COUNT)
    print(json.dumps(dict(route=route, list_vs_f64=new, explicit_vs_f64=old,
                          loss=[gallery_runs[route]["loss"], gallery_runs["explicit"]["loss"], oracle["loss"]])))
    for k in new:
        assert new[k] <= max(2.0 * old[k], FLOOR), (k, new[k], old[k])
    assert abs(gallery_runs[route]["loss"] - oracle["loss"]) <= max(2.0 * abs(gallery_runs["explicit"]["loss"] - oracle["loss"]),
                                                                     FLOOR * abs(oracle["loss"]))
    # object 5 is named by dead slots only (padded) or by nothing (truncated): its gradient is exactly zero
    assert not gallery_runs[route]["dh"][5].view(torch.int32).any()


def test_padding_leaves_the_live_slots_alone(gallery_runs):
    padded, cut = gallery_runs["padded"], gallery_runs["truncated"]
    assert torch.equal(padded["logits"][:COUNT].view(torch.int32), cut["logits"].view(torch.int32))
    assert not padded["logits"][COUNT:].view(torch.int32).any()          # dead slots: 0.0 exactly


# ------------------------------------------------------------------------------------------------ the switch --
def _batch(b, seed=2):
    return _data(dict(pairs=b, n=128, input_seed=seed, id_1=list(range(b)), id_2=[0, 1, 0, 7, 4, 9][:b]))


def test_without_the_switch_the_paired_step_is_what_it_was():
    runs = []
    for _ in range(2):
        m = _build(_pt_mul(1, 64, 8), "pt").train()
        assert m.sampling is None
        out = m.train_step(_batch(4), None)
        out["loss"].backward()
        lv = out["log_vars"]
        runs.append((out["loss"].detach().cpu(), m.match_head[1].weight.grad.cpu(), lv["num_gt_0"] + lv["num_gt_1"]))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    assert runs[0][2] == 4
    m.zero_grad(set_to_none=True)
    m.sampling = "cartesian"
    lv = m.train_step(_batch(4), None)["log_vars"]
    assert lv["num_gt_0"] + lv["num_gt_1"] == 16


def test_the_trainer_trains_on_cartesian_batches_eager_and_captured():
    from pcr_amd import train
    data = _batch(4)
    rec = {}
    for mode, steps in ((False, 12), (True, 5)):
        m = _build(_pt_mul(1, 64, 8), "pt").train()
        m.sampling = "cartesian"
        tr = train.Trainer(m, max_iters=40, lr=3e-4, grad_clip=1.0, graph=mode)
        outs = [tr.step(data) for _ in range(steps)]
        assert tr.graph == mode                                           # (the capture did not fall back)
        rec[mode] = [(float(o["loss"].detach()), float(o["grad_norm"])) for o in outs]
    losses = [l for l, _ in rec[False]]
    assert all(np.isfinite(losses)) and min(losses[1:]) < losses[0], losses
    # the fourth and fifth step of graph mode are replays of the captured forward + backward
    assert rec[True] == rec[False][:5], (rec[True], rec[False][:5])
