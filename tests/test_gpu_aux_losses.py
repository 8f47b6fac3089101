"""GPU: the auxiliary training losses (include/pcr.h section C2, csrc/aux_loss_kernels.hip, pcr_amd.train_ops KlPairs /
TripletLoss, pcr_amd.train_graph.aux_losses) -- the launches one by one against the float64 restatements of
tests/aux_ref.py, the draw bit for bit against its numpy restatement, the whole train_step against what the REFERENCE's
own train_step produced with the four losses on (tools/make_aux_golden.py -> tests/golden/train_step_aux_n128.npz), the
captured Trainer against the eager one, and the match-only step against itself.

Bound of the op tests (the rule of tests/test_gpu_train_attn_ops.py): max(2e-5 x the tensor's scale, YARD x y32), y32 = the
error of a float32 CPU evaluation of the same closed form (aux_ref on float32 tensors) against the float64 one, computed
here on the CPU -- never a figure read off the kernel.  For kl the scale is that of the two terms that cancel (cross and
lse2 - lse1 for a value; w p1, w p2, w p2 |h2 - h1| and w p2 |cross| for a gradient), not of their difference.  Every
worst value and bound is printed as a JSON line."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import aux_ref as R
from conftest import GOLDEN, load_golden
from pcr_amd import testing as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
BOUND = 2e-5
YARD = 8.0


def _hold(name, got, ref64, ref32, scale=None):
    got, ref64, ref32 = (torch.as_tensor(t).detach().cpu().to(F64) for t in (got, ref64, ref32))
    scale = float(ref64.abs().max()) if scale is None else float(scale)
    y32 = float((ref32 - ref64).abs().max())
    bound = max(BOUND * scale, YARD * y32)
    worst = float((got - ref64).abs().max())
    print(json.dumps(dict(op=name, worst=worst, bound=bound, scale=scale, y32=y32)))
    assert torch.isfinite(got).all(), name
    assert worst <= bound, (name, worst, bound)


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda()


def _info():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------ kl --
# (name, B, D, spread, match).  One workgroup of 256 threads per pair: D = 1 and 63 leave idle threads, 8192 is the training
# shape (C N = 64 x 128), 70 000 is no multiple of 256 nor of the backward's 1024-column chunk; +-30 makes the online
# maximum move while it sums; an all-match batch has an empty group.
KL_CASES = [("d1", 3, 1, 1.0, (1, 0, 1)), ("d63", 4, 63, 1.0, (0, 1, 1, 0)), ("d8192", 8, 8192, 1.0, (1, 1, 0, 1, 0, 0, 1, 0)),
            ("d70000", 2, 70000, 1.0, (1, 0)), ("pm30", 4, 300, 30.0, (1, 0, 0, 1)), ("allmatch", 4, 63, 1.0, (1, 1, 1, 1))]


def _kl_input(B, D, spread, seed=11):
    g = torch.Generator().manual_seed(seed)
    if spread > 1.0:
        h = (torch.rand(2 * B, D, generator=g, dtype=F64) * 2 - 1) * spread
    else:
        h = torch.randn(2 * B, D, generator=g, dtype=F64)
    return h.float()


def _kl_grad_scale(h, match, g):
    B, D = h.shape[0] // 2, h.shape[1]
    _, _, lse, cross, _ = R.kl_pairs(h, match)
    m = torch.as_tensor(match).bool()
    n1 = int(m.sum())
    n = torch.where(m, torch.tensor(float(max(n1, 1)), dtype=F64), torch.tensor(float(max(B - n1, 1)), dtype=F64))
    w = (abs(g) / (n * D))[:, None]
    p = torch.exp(h - lse[:, None])
    return float(torch.stack([(w * p[:B]).max(), (w * p[B:]).max(), (w * p[B:] * (h[B:] - h[:B]).abs()).max(),
                              (w * p[B:] * cross.abs()[:, None]).max()]).max())


@pytest.mark.parametrize("name,B,D,spread,match", KL_CASES)
def test_kl_pairs_forward_and_backward(name, B, D, spread, match):
    from pcr_amd import train_ops as TO
    h32 = _kl_input(B, D, spread)
    h64 = h32.to(F64)
    g = -1.7
    loss64, kl64, lse64, cross64, info64 = R.kl_pairs(h64, match)
    loss32, kl32, _, _, _ = R.kl_pairs(h32, match)
    grad64, grad32 = R.kl_pairs_grad(h64, match, g), R.kl_pairs_grad(h32, match, g)
    runs = []
    for _ in range(2):
        x = h32.cuda().requires_grad_()
        info = _info()
        loss, kl = TO.KlPairs.apply(x, _i32(match), info)
        (loss * g).backward()
        runs.append((loss.detach().clone(), kl.clone(), x.grad.clone(), int(info.item())))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][:3], runs[1][:3])), "kl: not reproducible"
    loss, kl, grad, info = runs[0]
    assert info == info64 == (R.INFO_KL_EMPTY if name == "allmatch" else 0)
    # the two terms that cancel in kl_i: cross_i / D and (lse2 - lse1) / D
    term = float(torch.maximum(cross64.abs(), (lse64[B:] - lse64[:B]).abs()).max()) / D
    _hold("kl[%s].kl" % name, kl, kl64, kl32, scale=term)
    _hold("kl[%s].loss" % name, loss, loss64, loss32, scale=term)
    _hold("kl[%s].dh" % name, grad.reshape(2 * B, D), grad64, grad32, scale=_kl_grad_scale(h64, match, g))
    if name == "d1":
        assert float(kl.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0      # one entry: softmax = 1, exactly


# ------------------------------------------------------------------------------------------------ pair_dist --
def _dist_input(B, R_, D, seed=5):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, D, generator=g, dtype=F64).float()
    h = torch.randn(R_, D, generator=g, dtype=F64).float()
    h[1] = a[0] + 1e-3 * torch.randn(D, generator=g).float() / np.sqrt(D)          # within 1e-3 of its anchor
    h[2] = a[1]                                                                     # exactly its anchor
    return a, h


# (B, R, D): 3 x 6 x 5 is one partial tile and one partial chunk of D; 33 x 66 x 130 is 2 x 3 tiles (the last of each axis
# holding one and two rows) and four chunks of 32 plus a tail of 2
@pytest.mark.parametrize("B,R_,D", [(3, 6, 5), (33, 66, 130)])
def test_pair_dist_forward_and_backward(B, R_, D):
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    a32, h32 = _dist_input(B, R_, D)
    a64, h64 = a32.to(F64), h32.to(F64)
    want, want32 = R.pair_dist(a64, h64), R.pair_dist(a32, h32)
    got = TO.pair_dist(a32.cuda(), h32.cuda())
    assert torch.equal(got, TO.pair_dist(a32.cuda(), h32.cuda()))
    _hold("pair_dist[%d,%d,%d]" % (B, R_, D), got, want, want32)
    assert float(want[0, 1]) < 2e-3
    assert abs(float(got[0, 1]) - float(want[0, 1])) <= max(BOUND * float(want[0, 1]), YARD * abs(float(want32[0, 1] - want[0, 1])))
    assert float(got[1, 2]) == pytest.approx(float(np.float32(1e-6)) * np.sqrt(D), rel=1e-6)     # d = eps sqrt(D)
    # backward: any coefficient matrix (two thirds zeros, as the triplet's is sparse), g = gout alpha / count
    g = torch.Generator().manual_seed(7)
    E32 = (torch.randn(B, R_, generator=g, dtype=F64) * (torch.rand(B, R_, generator=g) < 0.33)).float()
    gout, alpha, count = 0.75, 3.0, 12
    diff = lambda a, h: (a[:, None, :] - h[None, :, :]) + R.EPS                     # noqa: E731
    ref = {}
    for tag, (a, h, E) in (("64", (a64, h64, E32.to(F64))), ("32", (a32, h32, E32))):
        w = E[:, :, None] * diff(a, h) * (gout * alpha / count)
        ref[tag] = (-w.sum(dim=1), w.sum(dim=0))
    dev = lambda t: t.cuda().contiguous()                                           # noqa: E731
    outs = []
    for _ in range(2):
        da, dh = torch.full((B, D), 9e9, device="cuda"), torch.full((R_, D), 9e9, device="cuda")
        L.run.pcr_pair_dist_bwd_f32(dev(a32), dev(h32), dev(E32), dev(torch.tensor([gout])), dev(torch.tensor([0.2, alpha])),
                                    _i32([count]), da, dh, B, R_, D, L.stream_ptr())
        outs.append((da, dh))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _hold("pair_dist_bwd[%d,%d,%d].da" % (B, R_, D), outs[0][0], ref["64"][0], ref["32"][0])
    _hold("pair_dist_bwd[%d,%d,%d].dh" % (B, R_, D), outs[0][1], ref["64"][1], ref["32"][1])
    # count == 0: every gradient is 0
    L.run.pcr_pair_dist_bwd_f32(dev(a32), dev(h32), dev(E32), dev(torch.tensor([gout])), dev(torch.tensor([0.2, alpha])),
                                _i32([0]), da, dh, B, R_, D, L.stream_ptr())
    assert float(da.abs().max()) == 0.0 and float(dh.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the draw --
LAYOUTS = {
    "wide": (list(range(8)) + [0, 1, 2, 3, 104, 105, 106, 107], 4),            # pool >= T
    "narrow": ([5, 5, 5, 5, 9, 8], 4),                                          # pool < T: with replacement
    "empty": ([7, 7, 7, 7], 3),                                                 # no row with another id
    # 150 rows: the pool is built over three 64-lane steps, the last one partial; ids repeat, so pools have holes
    "long": ([i % 40 for i in range(75)] + [(i % 40) if i % 3 else 900 + i for i in range(75)], 128),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_triplet_draw_is_the_numpy_rule_bit_for_bit(name):
    from pcr_amd import train_ops as TO
    ids, Tn = LAYOUTS[name]
    B = len(ids) // 2
    match = [int(ids[i] == ids[B + i]) for i in range(B)]
    got = {}
    for seed in (0, 1, (5 << 32) + 17):
        want, winfo = R.draw(ids, match, Tn, seed=seed)
        info = _info()
        st = torch.full((1,), seed, dtype=torch.int64, device="cuda")
        neg = TO.triplet_draw(_i32(ids), _i32(match), Tn, info, seed=st)
        assert np.array_equal(neg.cpu().numpy(), want), (name, seed)
        assert int(info.item()) == winfo
        assert torch.equal(neg, TO.triplet_draw(_i32(ids), _i32(match), Tn, _info(), seed=st))      # same seed, same bits
        got[seed] = neg
    if name != "empty":
        assert not torch.equal(got[0], got[1])                                  # a seed advanced by one draws afresh
        words = R.words_for(ids, match, got[1].cpu().numpy())
        again = TO.triplet_draw(_i32(ids), _i32(match), Tn, _info(), rand=torch.from_numpy(words).cuda())
        assert torch.equal(again, got[1])                                       # the rand seam
    none = TO.triplet_draw(_i32(ids), _i32(match), Tn, _info())                 # no seed: seed 0
    assert torch.equal(none, got[0])


# ------------------------------------------------------------------------------------------------ the whole op --
def _triplet_torch(h, neg, match, margin):
    B, Tn = h.shape[0] // 2, neg.shape[1]
    idx = [i for i in range(B) if match[i]]
    a = torch.tensor([i for i in idx for _ in range(Tn)])
    n = torch.as_tensor(np.concatenate([neg[i] for i in idx]), dtype=torch.long)
    return torch.nn.TripletMarginLoss(margin=margin, p=2)(anchor=h[:B][a], positive=h[B:][a], negative=h[n])


# (B, D, T): D = 128 is the pooled use_o width; (33, 130) spans 2 x 3 tiles and five chunks of D (66 triplets: more leave
# no margin 1e-3 of the largest distance away from every hinge); (3, 7, 6) draws from a pool of 4 with replacement, so a
# negative counts twice or three times in E; (5, 1, 3): one column
@pytest.mark.parametrize("B,D,Tn", [(6, 128, 4), (33, 130, 3), (3, 7, 6), (5, 1, 3)])
def test_triplet_loss_with_injected_negatives_matches_torch(B, D, Tn):
    from pcr_amd import train_ops as TO
    g = torch.Generator().manual_seed(3)
    h64 = torch.randn(2 * B, D, generator=g, dtype=F64)
    h64[B:] = h64[:B] + 0.3 * torch.randn(B, D, generator=g, dtype=F64)          # a positive is nearer than a negative
    h32 = h64.float()
    h64 = h32.to(F64)
    match = [int(i % 3 != 1) for i in range(B)]
    rng = np.random.default_rng(1)
    neg = np.full((B, Tn), -1, np.int32)
    for i in range(B):
        if match[i]:
            pool = [r for r in range(2 * B) if r not in (i, B + i)]
            neg[i] = rng.choice(pool, Tn, replace=len(pool) < Tn)
    margin = R.median_margin(h64, neg, match)
    gap, dmax = R.hinge_gaps(h64, neg, match, margin)
    assert margin > 0 and gap >= 1e-3 * dmax, (margin, gap, dmax)               # no triplet sits on the hinge
    alpha, up = 2.5, 0.6
    x64 = h64.clone().requires_grad_()
    want = _triplet_torch(x64, neg, match, margin) * alpha
    (want * up).backward()
    x32 = h32.clone().requires_grad_()
    y32 = R.triplet(x32, neg, match, np.float32(margin))[0] * alpha
    (y32 * up).backward()
    runs = []
    for _ in range(2):
        x = h32.cuda().requires_grad_()
        info = _info()
        hyper = torch.tensor([margin, alpha], dtype=torch.float32).cuda()
        loss, dist, count = TO.TripletLoss.apply(x, _i32(neg), _i32(match), hyper, info)
        (loss * up).backward()
        runs.append((loss.detach().clone(), x.grad.clone(), dist.clone()))
        assert int(count.item()) == sum(match) * Tn and int(info.item()) == 0
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "triplet: not reproducible"
    tag = "triplet[%d,%d,%d]" % (B, D, Tn)
    _hold(tag + ".loss", runs[0][0], want, y32, scale=alpha * dmax)              # (a mean of differences of distances)
    _hold(tag + ".dh", runs[0][1], x64.grad, x32.grad)
    # no matching pair: loss 0, gradient 0, the info bit
    x = h32.cuda().requires_grad_()
    info = _info()
    loss, _, count = TO.TripletLoss.apply(x, _i32(np.full((B, Tn), -1)), _i32([0] * B), hyper, info)
    loss.backward()
    assert float(loss.detach()) == 0.0 and int(count.item()) == 0 and float(x.grad.abs().max()) == 0.0
    assert int(info.item()) == R.INFO_TRIPLET_NONE


# ------------------------------------------------------------------------------------------------ the model --
def _head(n_out):
    return [dict(type="LinearRes", n_in=128, n_out=128, norm="GN", ng=16),
            dict(type="Linear", in_features=128, out_features=n_out)]


ON = dict(kl=True, match=True, cls=True, shape=False, fp=True, dense=False, triplet=True)


def _aux_model(margin=0.25, Tn=4, losses=ON, seed=0):
    import bench
    from mmdet3d.models import build_model
    cfg = copy.deepcopy(bench.PT_MODEL)
    cfg.update(cls_head=_head(20), fp_head=_head(1), triplet_sample_num=Tn, triplet_loss=dict(margin=margin, p=2),
               losses_to_use=dict(losses))
    m = build_model(cfg)
    man = T.load_manifest(os.path.join(GOLDEN, "pt_aux_manifest.json"))
    assert T.manifest_of(m) == man
    m.load_state_dict(T.seeded_state_dict(man, seed), strict=True)
    return m.cuda()


def _aux_data(pairs, n, seed, classes=20, dev="cuda"):
    """tools/make_aux_golden.py train_data"""
    s1, s2 = T.synthetic_pairs(pairs, n, seed=seed, kind="randn")
    ids1 = torch.arange(pairs)
    ids2 = torch.where(torch.arange(pairs) < pairs // 2, ids1, ids1 + 100)
    lab1 = (torch.arange(pairs) * 5 + 3) % classes
    lab2 = torch.where(torch.arange(pairs) < pairs // 2, lab1, (lab1 + 7) % classes)
    s1, s2 = s1.to(dev), s2.to(dev)
    return dict(sparse_1=list(s1), sparse_2=list(s2), dense_1=list(s1), dense_2=list(s2),
                label_1=[v.view(1).to(dev) for v in lab1], label_2=[v.view(1).to(dev) for v in lab2],
                id_1=[i.view(1).to(dev) for i in ids1], id_2=[i.view(1).to(dev) for i in ids2])


def test_train_step_with_the_four_losses_matches_the_reference(grad_floor):
    g = load_golden("train_step_aux_n128")
    meta = g["meta"]
    pairs, n = meta["pairs"], meta["n"]
    m = _aux_model(margin=float(g["margin"]), Tn=meta["triplet_sample_num"])
    m.train()
    data = _aux_data(pairs, n, meta["input_seed"], meta["classes"])
    ids = g["ids"]
    match = (ids[:pairs] == ids[pairs:]).astype(np.int32)
    m.triplet_rand = torch.from_numpy(R.words_for(ids.tolist(), match, g["neg"])).cuda()    # the recorded negatives
    out = m.train_step(data, None)
    loss = float(out["loss"])
    out["loss"].backward()
    lv = out["log_vars"]
    params = dict(m.named_parameters())
    worst, ref_own, vs64 = {}, {}, {}
    for k in g:
        if k.startswith("grad:"):
            got = params[k[5:]].grad.cpu().numpy()
            scale = max(1e-3, float(np.abs(g[k]).max()))
            worst[k[5:]] = float(np.abs(got - g[k]).max()) / scale
            g64 = g["grad64:" + k[5:]]
            ref_own[k[5:]] = float(np.abs(g[k] - g64).max()) / scale
            vs64[k[5:]] = float(np.abs(got - g64).max()) / scale
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params.values() if p.grad is not None)))
    bufs = dict(m.named_buffers())
    bw = {k[4:]: float(np.abs(bufs[k[4:]].cpu().numpy() - g[k]).max()) for k in g if k.startswith("buf:")}
    parts = {k: (float(lv[k]), float(g[k])) for k in ("match_loss", "cls_loss", "fp_loss", "kl_loss", "triplet_loss",
                                                        "match_acc", "cls_acc", "fp_acc")}
    print(json.dumps(dict(loss=loss, ref_loss=float(g["loss"]), parts=parts, grad_norm=gn, ref_grad_norm=float(g["grad_norm"]),
                          vs_ref32=worst, ref32_vs_ref64=ref_own, vs_ref64=vs64, running_mean=bw)))
    assert int(train_info(m)) == 0
    assert abs(loss - float(g["loss"])) < 1e-4
    for k in ("match_acc", "cls_acc", "fp_acc"):
        assert abs(parts[k][0] - parts[k][1]) < 1e-6, (k, parts[k])
    for k in ("match_loss", "cls_loss", "fp_loss", "kl_loss", "triplet_loss"):
        assert abs(parts[k][0] - parts[k][1]) < 1e-4, (k, parts[k])
    for k in worst:
        assert worst[k] < grad_floor or vs64[k] < max(grad_floor, 2.0 * ref_own[k]), (k, worst[k], vs64[k], ref_own[k])
    assert gn == pytest.approx(float(g["grad_norm"]), rel=2e-3)
    assert all(v < 1e-5 for v in bw.values()), bw
    no_grad = sorted(k for k, p in params.items() if p.grad is None)
    assert no_grad == sorted(json.loads(str(g["no_grad_params"])))

    # forward_test in eval mode, after the step as the tool recorded it
    m.eval()
    one = lambda v: [torch.full((1,), v, dtype=torch.long, device="cuda")] * pairs      # noqa: E731
    with torch.no_grad():
        res = m(return_loss=False, **dict(data, size_1=one(n), size_2=one(n), vis_1=one(1), vis_2=one(1)))[0]
    dev = {k: float(np.abs(res[k].cpu().numpy() - g[k]).max()) for k in ("val_cls_preds", "val_fp_preds", "val_match_preds")}
    vl = {k: (float(res[k]), float(g[k])) for k in ("val_cls_loss", "val_fp_loss", "val_kl_loss", "val_match_loss")}
    print(json.dumps(dict(forward_test=dev, val_losses=vl)))
    assert res["val_cls_preds"].shape == (2 * pairs, meta["classes"]) and res["val_fp_preds"].shape == (2 * pairs,)
    assert dev["val_cls_preds"] < 1e-4 and dev["val_fp_preds"] < 1e-4
    for k, (a, b) in vl.items():
        assert abs(a - b) < 1e-4, (k, a, b)
    # the public head entry on encoded objects gives the same predictions
    with torch.no_grad():
        xyz1, xyz2, h1, h2 = m.siamese_forward(torch.stack(data["sparse_1"]), torch.stack(data["sparse_2"]))
        heads = m.object_heads(torch.cat([h1, h2], dim=0))
    assert torch.equal(heads["cls"], res["val_cls_preds"]) and torch.equal(heads["fp"], res["val_fp_preds"])


def train_info(m):
    return m.__dict__["_pcr_aux"].info.item()


def _snapshot(m):
    return [p.detach().clone() for p in m.parameters()] + [b.detach().clone() for b in m.buffers()]


def test_twelve_captured_trainer_steps_equal_twelve_eager_ones():
    from pcr_amd import train
    runs = {}
    for graph in (True, False):
        m = _aux_model()
        m.train()
        tr = train.Trainer(m, max_iters=40, lr=3e-4, grad_clip=1.0, graph=graph)
        losses, trip = [], []
        for it in range(12):
            out = tr.step(_aux_data(8, 128, seed=2))
            losses.append(out["loss"].detach().clone())
            trip.append(out["log_vars"]["triplet_loss"])
        if graph:
            assert tr.graph and tr._g is not None, "the iteration was not captured"
        assert int(m.__dict__["_pcr_aux"].seed.item()) == 12                 # one draw per step, replays included
        runs[graph] = (torch.stack(losses), trip, _snapshot(m))
    losses, trip, snap = runs[True]
    assert torch.isfinite(losses).all() and all(np.isfinite(trip))
    assert len(set(trip)) > 1                                                # (a fresh draw per replay: the term moves)
    assert torch.equal(losses, runs[False][0]), (losses, runs[False][0])
    assert trip == runs[False][1]
    assert all(torch.equal(a, b) for a, b in zip(snap, runs[False][2])), "captured and eager training diverged"


def test_switched_off_is_the_same_as_left_out():
    off = dict(kl=False, match=True, cls=False, shape=False, fp=False, dense=False, triplet=False)
    outs = []
    for losses in (off, dict(match=True)):
        m = _aux_model(losses=losses)
        m.train()
        assert not m._aux_on()
        out = m.train_step(_aux_data(8, 128, seed=2), None)
        out["loss"].backward()
        assert "_pcr_aux" not in m.__dict__ and "cls_loss" not in out["log_vars"]          # nothing new was set up
        outs.append((out["loss"].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert torch.equal(outs[0][0], outs[1][0])
    assert sorted(outs[0][1]) == sorted(outs[1][1]) and not any(k.startswith(("cls_head", "fp_head")) for k in outs[0][1])
    assert all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in outs[0][1])


def test_use_o_takes_the_pooled_stage_two_features():
    """use_o: the triplet's rows are get_pooled_feats(o1 / o2), D = 128; the gradient reaches the matching stages only
    through them and the match loss, and the encoder through both"""
    m = _aux_model(losses=dict(match=True, triplet=True))
    m.use_o = True
    m.train()
    out = m.train_step(_aux_data(8, 128, seed=2), None)
    out["loss"].backward()
    assert np.isfinite(float(out["loss"])) and out["log_vars"]["triplet_loss"] >= 0.0
    assert m.cross_stage2.q_proj.weight.grad is not None and torch.isfinite(m.cross_stage2.q_proj.weight.grad).all()
