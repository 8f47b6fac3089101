"""GPU: the PointNet / DGCNN training ops (pcr_amd.train_ops: BnAct, EdgeConvTrain, Bmm, PoolBoth, ChannelMax) one by one
against the float64 references of tests/train_ref.py -- forward value, every gradient, every side effect (running
statistics, saved indices) -- at the shapes where their kernels change plan, and bit-reproducibility of all of it (no
float atomics anywhere).

Bounds (`_rel` = max|a - b| / max|b|): selections, indices and routed copies exact; pooling means and their gradients
1e-6 (PoolPair's bound); BatchNorm-type outputs and gradients, and Bmm, 2e-5 (tnorm's bound) -- the two stressed
inputs included.  The inputs are conditioned (train_ref) so that the float64 reference takes no marginal decision; every
test asserts that on the CPU before it launches.  The case tables below are shared with test_train_ref_cpu.py, which
shows without a device that every input conditions to zero marginal decisions."""
import json
import math

import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 1e-5
BN_BOUND = 2e-5
MEAN_BOUND = 1e-6

# ---------------------------------------------------------------------------------------------- cases --
# BnAct (B, C, L): PointNet's conv shapes; nparts = 2 < B (the strided cloud loop); odd B over two parts; the STN's fully
# connected BatchNorms (clouds as tokens, B = 1); C % 32 != 0 with L < 64; L = 1; L > 256; nparts = B = 70
BN_SHAPES = [(8, 64, 128), (8, 128, 128), (16, 1024, 128), (5, 1024, 9), (1, 512, 8), (1, 256, 8), (4, 100, 33), (3, 7, 1),
             (2, 3, 300), (70, 16, 40)]
BN_ACTS = {"none": (False, 0.0), "relu": (True, 0.0), "leaky": (True, 0.2)}
BN_CASES = [(s, a, False) for s in BN_SHAPES for a in BN_ACTS] + [((8, 64, 128), a, True) for a in BN_ACTS] + \
           [((16, 1024, 128), "relu", True)]
# EdgeConvTrain (B, Co, N, K): DGCNN's own layers; the channel-chunked LDS plan; odd everything; K = N; K = 1.
# Variants: "knn" (neighbours of random features), "repeat" (a neighbour listed twice in a row: exact ties on ONE table
# entry), "dup" (a cloud with duplicated points: exact ties between DIFFERENT entries, so the tie rule decides where the
# gradient goes), "stress" (channel mean = 10 standard deviations: the layer's statistics are uncentred float32 sums)
EDGE_SHAPES = [(4, 64, 128, 20), (2, 128, 256, 20), (2, 256, 128, 20), (2, 64, 1024, 20), (3, 40, 50, 7), (1, 33, 33, 33),
               (2, 32, 64, 1)]
EDGE_CASES = [(s, "knn") for s in EDGE_SHAPES] + [((4, 64, 128, 20), "repeat"), ((3, 40, 50, 7), "repeat"),
                                                  ((4, 64, 128, 20), "dup"), ((3, 40, 50, 7), "dup"),
                                                  ((1, 33, 33, 33), "dup"), ((4, 64, 128, 20), "stress")]
SLOPE = 0.2
# Bmm (B, k, N): k = 3 and 64 are PointNet's transforms; 127 / 128 straddle the 64 KiB of default dynamic LDS
BMM_CASES = [(1, 1, 1), (5, 1, 1000), (1, 3, 128), (5, 3, 128), (5, 3, 63), (1, 17, 65), (5, 17, 1000), (1, 64, 1), (1, 64, 64),
             (5, 64, 128), (1, 127, 63), (5, 127, 65), (1, 128, 65), (5, 128, 128), (1, 128, 1000)]
# PoolBoth (P, C, L)
POOL_CASES = [(7, 1, L) for L in (1, 8, 63, 64, 65, 128, 300)] + [(3, 6, L) for L in (1, 8, 63, 64, 65, 128, 300)] + \
             [(2, 64, L) for L in (1, 63, 64, 65, 300)] + [(2, 1024, 8), (1, 1024, 128), (8, 1024, 1)]
# ChannelMax (B, C, L, W): W in {1, 2, 64, C}
CMAX_CASES = [(1, 1, 1, 1), (3, 6, 63, 1), (3, 6, 8, 6), (2, 6, 300, 2), (2, 64, 128, 64), (2, 64, 65, 2), (2, 64, 300, 1),
              (5, 64, 1, 64), (1, 1024, 8, 64), (2, 1024, 64, 1024), (1, 1024, 128, 2), (2, 1024, 63, 1)]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _affine(C, g):
    """gamma = 1 + 0.3 N(0,1) with channel 0 forced negative and channel 1 exactly zero (z = beta there: kept clear of
    zero, on the slope side of the activation); beta = 0.1 N(0,1)"""
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    gamma[0] = -gamma[0].abs() - 0.1
    gamma[1] = 0.0
    beta[1] = -0.25
    return gamma, beta


def make_bn_input(shape, act, stress):
    """float32 CPU tensors of one BnAct case: y (conditioned when there is an activation), gamma, beta, go"""
    B, C, Ln = shape
    g = _gen(B, C, Ln, len(act), stress)
    y = torch.randn(B, C, Ln, generator=g) * (0.5 + torch.rand(1, C, 1, generator=g)) + torch.randn(1, C, 1, generator=g)
    gamma, beta = _affine(C, g)
    if stress:
        # the first element of a channel -- the offset the forward subtracts before it sums -- 8 standard deviations out
        for c in (2, C - 1):
            y[0, c, 0] = y[:, c].mean() + 8.0 * y[:, c].std()
    moved = 0
    if BN_ACTS[act][0]:
        y, moved = R.condition_signs(y, gamma, beta, EPS)
    return dict(y=y, gamma=gamma, beta=beta, go=torch.randn(B, C, Ln, generator=g), moved=moved)


def make_edge_input(shape, variant, knn):
    """float32 CPU tensors of one EdgeConvTrain case; knn(feat (B,C,N), K) -> idx (B,N,K) int32 on the CPU (the
    device's dgcnn_engine.knn_feat in the GPU tests, train_ref.knn_ref where there is no device)"""
    from pcr_amd import testing as T
    B, Co, N, K = shape
    g = _gen(B, Co, N, K, len(variant))
    if variant == "dup":
        xyz = T.synthetic_clouds(B, N, seed=Co + K, kind="dup")
        feat = xyz.permute(0, 2, 1).contiguous()
        w = torch.randn(2 * Co, 3, generator=g)
        # element-wise products and sums (no blocked matmul): duplicated points get bit-identical table columns
        tab = (w[None, :, 0:1] * feat[:, 0:1] + w[None, :, 1:2] * feat[:, 1:2]) + w[None, :, 2:3] * feat[:, 2:3]
    else:
        feat = torch.randn(B, 16, N, generator=g)
        tab = torch.randn(B, 2 * Co, N, generator=g)
    idx = knn(feat, K)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, N, K)
    if variant == "repeat" and K >= 2:
        idx = idx.clone()
        idx[:, :, K // 2:2 * (K // 2)] = idx[:, :, :K // 2]
    if variant == "stress":
        tab[:, Co:] += 10.0 * math.sqrt(2.0)
    gamma, beta = _affine(Co, g)
    tab, moved = R.condition_edge(tab, idx, gamma, beta, EPS)
    return dict(tab=tab, idx=idx, gamma=gamma, beta=beta, gp=torch.randn(B, Co, N, generator=g), moved=moved)


def _planted(rows, n, g):
    """(rows, n) values with the edges of a first-maximum selection planted row by row (kind = row % 6): all zeros (a
    post-ReLU row); the maximum at index 0; at n - 1; twice, at n // 4 and n - 1 (for n > 64: two lanes, two strides of a
    wave's loop); all negative (for n < 64 the idle lanes of a wave hold -inf); half-integers (ties everywhere)"""
    v = torch.randn(rows, n, generator=g)
    kind = torch.arange(rows) % 6
    top = v.abs().amax(dim=1) + 1.0
    v[kind == 0] = 0.0
    v[kind == 1, 0] = top[kind == 1]
    v[kind == 2, n - 1] = top[kind == 2]
    v[kind == 3, n - 1] = top[kind == 3]
    v[kind == 3, n // 4] = top[kind == 3]
    v[kind == 4] = -v[kind == 4].abs() - 0.5
    v[kind == 5] = torch.round(2.0 * v[kind == 5]) / 2.0
    return v


def make_pool_input(P, C, Ln):
    g = _gen(P, C, Ln, 11)
    o = _planted(P * C, Ln, g).reshape(P, C, Ln).contiguous()
    return dict(o=o, go=torch.randn(P, 2 * C, generator=g))


def make_cmax_input(B, C, Ln, W):
    g = _gen(B, C, Ln, W, 13)
    G = C // W
    x = _planted(B * G * Ln, W, g).reshape(B, G, Ln, W).permute(0, 1, 3, 2).reshape(B, C, Ln).contiguous()
    return dict(x=x, go=torch.randn(B, G, Ln, generator=g))


# -------------------------------------------------------------------------------------------- helpers --
def _rel(a, b):
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def _vs(got, want):
    """_rel of a device float32 tensor against its float64 reference"""
    return _rel(got.detach().cpu().to(F64), want.detach())


def _saved_arg(out, shape):
    """the int32 index tensor the Function saved for its backward (the last one of that shape: EdgeConvTrain saves the
    neighbour lists in front of it)"""
    hits = [t for t in out.grad_fn.saved_tensors if t.dtype == torch.int32 and tuple(t.shape) == tuple(shape)]
    assert hits
    return hits[-1].cpu().long()


def _leaves(*ts):
    return [t.detach().to(F64).requires_grad_(True) for t in ts]


def _report(op, case, worst):
    print(json.dumps(dict(op=op, case=str(case), worst=worst)))


def _bn_layer(cls, C, gamma, beta, momentum, track, g, dtype=torch.float32):
    bn = cls(C, eps=EPS, momentum=momentum, track_running_stats=track)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        if track:        # (not the 0 / 1 defaults: a wrong (1 - momentum) factor must show)
            bn.running_mean.copy_(torch.randn(C, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.to(dtype).train()


def _check_running(bn, ref, worst):
    worst["running_mean"] = _vs(bn.running_mean, ref.running_mean)
    worst["running_var"] = _vs(bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 2


# ---------------------------------------------------------------------------------------------- BnAct --
def _bn_act_twice(inp, act, bn):
    """forward + backward of BnAct twice on the same input (two running-statistics steps) -> the two result lists"""
    from pcr_amd import train_ops as TO
    runs = []
    for _ in range(2):
        y = inp["y"].cuda().requires_grad_(True)
        z = TO.BnAct.apply(y, bn.weight, bn.bias, bn, BN_ACTS[act][0], BN_ACTS[act][1])
        runs.append([z.detach()] + list(torch.autograd.grad(z, [y, bn.weight, bn.bias], inp["go"].cuda())))
    return runs


def _bn_act_want(inp, act):
    y, gamma, beta = _leaves(inp["y"], inp["gamma"], inp["beta"])
    z, mean, unb = R.bn_act_ref(y, gamma, beta, EPS, *BN_ACTS[act])
    return [z.detach()] + list(torch.autograd.grad(z, [y, gamma, beta], inp["go"].to(F64))), mean, unb


def _bn_act_case(shape, act, stress, momentum):
    inp = make_bn_input(shape, act, stress)
    if BN_ACTS[act][0]:
        assert R.marginal_signs(inp["y"], inp["gamma"], inp["beta"], EPS) == 0
    C = shape[1]
    g = _gen(C, 17)
    bn = _bn_layer(torch.nn.BatchNorm1d, C, inp["gamma"], inp["beta"], momentum, True, g).cuda()
    g = _gen(C, 17)
    ref = _bn_layer(torch.nn.BatchNorm1d, C, inp["gamma"], inp["beta"], momentum, True, g, dtype=F64)
    runs = _bn_act_twice(inp, act, bn)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    want, mean, unb = _bn_act_want(inp, act)
    with torch.no_grad():
        for _ in range(2):
            ref(inp["y"].to(F64))
    # the reference's own statistics are what nn.BatchNorm1d tracks (1e-12 on the CPU: test_train_ref_cpu.py)
    worst = {k: _vs(a, b) for k, a, b in zip(("z", "dy", "dgamma", "dbeta"), runs[0], want)}
    _check_running(bn, ref, worst)
    _report("BnAct", (shape, act, "stress" if stress else "", momentum), worst)
    assert max(worst.values()) < BN_BOUND, worst


@pytest.mark.parametrize("shape,act,stress", BN_CASES)
def test_bn_act_matches_float64(shape, act, stress):
    """z, dy, dgamma, dbeta and the running statistics after two steps (against nn.BatchNorm1d in float64) within 2e-5.
    Observed worst _rel on the MI355X: z 5.1e-7, dy 3.5e-7, dgamma 4.2e-7, dbeta 1.4e-7, running mean 9.1e-8, running
    var 4.7e-7; stressed (y[0, c, 0] 8 sigma out): z 1.8e-6, dy 4.5e-7, dgamma 8.5e-7, running var 1.1e-6."""
    _bn_act_case(shape, act, stress, 0.1)


@pytest.mark.parametrize("shape", [(8, 64, 128), (5, 1024, 9), (3, 7, 1)])
def test_bn_act_running_statistics_with_momentum_one_half(shape):
    _bn_act_case(shape, "relu", False, 0.5)


def test_bn_act_without_tracking_leaves_the_buffers_alone():
    from pcr_amd import train_ops as TO
    inp = make_bn_input((4, 100, 33), "leaky", False)
    bn = _bn_layer(torch.nn.BatchNorm1d, 100, inp["gamma"], inp["beta"], 0.1, False, _gen(1)).cuda()
    assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
    runs = _bn_act_twice(inp, "leaky", bn)
    want, _, _ = _bn_act_want(inp, "leaky")
    assert max(_vs(a, b) for a, b in zip(runs[0], want)) < BN_BOUND
    # a layer that tracks, called through a stand-in that says it does not: its buffers must come back bit for bit
    bn = _bn_layer(torch.nn.BatchNorm1d, 100, inp["gamma"], inp["beta"], 0.1, True, _gen(2)).cuda()
    before = [bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]
    bn.track_running_stats = False
    TO.BnAct.apply(inp["y"].cuda(), bn.weight, bn.bias, bn, True, 0.2)
    for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
        assert torch.equal(a, b)


def test_batch_norm_refuses_what_torch_refuses():
    """momentum=None (cumulative average) has no HIP path; one value per channel has no variance: torch's training-mode
    BatchNorm raises "Expected more than 1 value per channel when training", and so do BnAct and EdgeConvTrain --
    before any launch, the running statistics untouched"""
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    g = _gen(3)
    C = 4
    one = torch.zeros(1, 1, 1, dtype=torch.int32, device="cuda")
    calls = {torch.nn.BatchNorm1d: lambda bn, x, idx: TO.BnAct.apply(x, bn.weight, bn.bias, bn, True, 0.0),
             torch.nn.BatchNorm2d: lambda bn, x, idx: TO.EdgeConvTrain.apply(x, idx, bn.weight, bn.bias, bn, SLOPE)}
    for cls, call in calls.items():
        two_d = cls is torch.nn.BatchNorm2d
        bn = _bn_layer(cls, C, torch.ones(C), torch.zeros(C), 0.1, True, g).cuda()
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            bn(torch.randn(*((1, C, 1, 1) if two_d else (1, C, 1)), generator=g).cuda())
        before = [bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]
        with pytest.raises(L.PcrError, match="Expected more than 1 value per channel when training"):
            call(bn, torch.randn(1, 2 * C if two_d else C, 1, generator=g).cuda(), one)
        for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
            assert torch.equal(a, b)
        bn.momentum = None
        with pytest.raises(L.PcrError, match="momentum=None"):
            call(bn, torch.randn(2, 2 * C if two_d else C, 4, generator=g).cuda(), one.expand(2, 4, 1).contiguous())
        for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
            assert torch.equal(a, b)


def _bn_step_caller(name):
    """-> (the BatchNorm modules whose statistics the Function tracks, a function that runs ONE training-mode forward):
    the three callers of train_ops._bn_batch_step at the smallest shapes their own tests use"""
    from pcr_amd import train_ops as TO
    g = _gen(29, len(name))
    if name == "BnAct":
        B, C, Ln = 3, 7, 1
        bn = _bn_layer(torch.nn.BatchNorm1d, C, *_affine(C, g), 0.1, True, g).cuda()
        y = torch.randn(B, C, Ln, generator=g).cuda()
        return [bn], lambda: TO.BnAct.apply(y, bn.weight, bn.bias, bn, True, 0.0)
    if name == "EdgeConvTrain":
        B, Co, N, K = 2, 32, 64, 1
        bn = _bn_layer(torch.nn.BatchNorm2d, Co, *_affine(Co, g), 0.1, True, g).cuda()
        tab = torch.randn(B, 2 * Co, N, generator=g).cuda()
        idx = torch.randint(0, N, (B, N, K), generator=g).to(torch.int32).cuda()
        return [bn], lambda: TO.EdgeConvTrain.apply(tab, idx, bn.weight, bn.bias, bn, SLOPE)
    from mmdet3d.models.pointnet2_utils import PointNetSetAbstractionEdgeSA
    from pcr_amd import engine
    from pcr_amd import testing as T
    B, N, S, K = 3, 128, 128, 32
    sa = PointNetSetAbstractionEdgeSA(npoint=None, radius=0.3, nsample=K, mlp=[0, 32, 32, 32], sampling="RANDOM",
                                      use_xyz=True, use_knn=True)
    sa.load_state_dict(T.seeded_state_dict(T.manifest_of(sa), 5))
    sa = sa.cuda().train()
    xyz = T.synthetic_clouds(B, N, seed=3, kind="randn").cuda()
    idx = engine.knn_prefix(xyz, S, K)
    return list(sa.mlp_bns), lambda: TO.sa_edge_train(sa, xyz, None, idx)


def _bn_state(bns):
    return [(t._version, t.clone()) for bn in bns for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]


def _same_state(before, bns):
    return all(v == w and torch.equal(a, b) for (v, a), (w, b) in zip(before, _bn_state(bns)))


@pytest.mark.parametrize("name", ["SaEdgeTrain", "BnAct", "EdgeConvTrain"])
def test_the_batch_statistics_step_keeps_the_modules_books(name):
    """one training-mode forward of each Function that normalises by batch statistics: the running buffers -- written
    through raw pointers by the finalize launch -- show it in Tensor._version (what the caches are keyed by) and
    num_batches_tracked counts exactly one batch; a module that does not track is left alone, buffers and counter, bit
    for bit; momentum=None (on the LAST of the modules) is refused before any module's statistics have moved"""
    from pcr_amd import _lib as L
    bns, forward = _bn_step_caller(name)
    assert all(bn.training and bn.track_running_stats and bn.num_batches_tracked is not None for bn in bns)
    before = _bn_state(bns)
    forward()
    for bn, i in zip(bns, range(0, len(before), 3)):
        assert bn.running_mean._version > before[i][0] and bn.running_var._version > before[i + 1][0]
        assert not torch.equal(bn.running_mean, before[i][1]) and not torch.equal(bn.running_var, before[i + 1][1])
        assert int(bn.num_batches_tracked) == int(before[i + 2][1]) + 1
    before = _bn_state(bns)
    for bn in bns:
        bn.track_running_stats = False
    forward()
    assert _same_state(before, bns)
    for bn in bns:
        bn.track_running_stats = True
    bns[-1].momentum = None
    with pytest.raises(L.PcrError, match="momentum=None"):
        forward()
    assert _same_state(before, bns)


# -------------------------------------------------------------------------------------- EdgeConvTrain --
def _device_knn(feat, K):
    from pcr_amd import dgcnn_engine
    return dgcnn_engine.knn_feat(feat.cuda(), K).cpu()


@pytest.mark.parametrize("shape,variant", EDGE_CASES)
def test_edge_conv_train_matches_float64(shape, variant):
    """pooled, dtab, dgamma, dbeta and BatchNorm2d's running statistics within 2e-5; the saved arg exactly the first k.
    Observed worst _rel on the MI355X: pooled 1.2e-7, dtab 3.1e-7, dgamma 1.4e-7, dbeta 1.1e-7, running mean 8.5e-8,
    running var 7.6e-8; stressed (channel mean 10 sigma): pooled 3.9e-6, dtab 3.8e-6, dgamma 4.2e-6, running var 3.2e-6."""
    from pcr_amd import train_ops as TO
    B, Co, N, K = shape
    inp = make_edge_input(shape, variant, _device_knn)
    idx = inp["idx"]
    if variant != "dup":                                     # the point itself is in its list
        assert bool((idx.long() == torch.arange(N).view(1, N, 1)).any(dim=2).all())
    assert R.edge_marginals(inp["tab"], idx, inp["gamma"], inp["beta"], EPS) == (0, 0)
    bn = _bn_layer(torch.nn.BatchNorm2d, Co, inp["gamma"], inp["beta"], 0.1, True, _gen(Co, 19)).cuda()
    ref = _bn_layer(torch.nn.BatchNorm2d, Co, inp["gamma"], inp["beta"], 0.1, True, _gen(Co, 19), dtype=F64)
    runs, args = [], []
    for _ in range(2):
        tab = inp["tab"].cuda().requires_grad_(True)
        pooled = TO.EdgeConvTrain.apply(tab, idx.cuda(), bn.weight, bn.bias, bn, SLOPE)
        args.append(_saved_arg(pooled, (B, Co, N)))
        runs.append([pooled.detach()] + list(torch.autograd.grad(pooled, [tab, bn.weight, bn.bias], inp["gp"].cuda())))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    tab64, gamma, beta = _leaves(inp["tab"], inp["gamma"], inp["beta"])
    pooled64, arg64, _, _ = R.edge_conv_ref(tab64, idx, gamma, beta, EPS, SLOPE)
    want = [pooled64.detach()] + list(torch.autograd.grad(pooled64, [tab64, gamma, beta], inp["gp"].to(F64)))
    with torch.no_grad():
        for _ in range(2):
            ref(R.edge_pre(inp["tab"].to(F64), idx))
    assert torch.equal(args[0], arg64) and torch.equal(args[1], arg64)
    if variant in ("repeat", "dup") and K > 1:
        z = R.edge_pre(inp["tab"].to(F64), idx)
        top = z.topk(2, dim=3).values
        low = (-z).topk(2, dim=3).values
        assert int((top[..., 0] == top[..., 1]).sum()) + int((low[..., 0] == low[..., 1]).sum()) > 0    # ties are there
    worst = {k: _vs(a, b) for k, a, b in zip(("pooled", "dtab", "dgamma", "dbeta"), runs[0], want)}
    _check_running(bn, ref, worst)
    _report("EdgeConvTrain", (shape, variant), worst)
    assert max(worst.values()) < BN_BOUND, worst


# ------------------------------------------------------------------------------------------------ Bmm --
def _bmm_input(B, k, N):
    g = _gen(B, k, N, 23)
    x, T = torch.randn(B, k, N, generator=g), torch.randn(B, k, k, generator=g) / math.sqrt(k)
    if k > 1:
        assert not torch.equal(T, T.transpose(1, 2))       # (a swapped transpose flag must not pass)
    return x, T, torch.randn(B, k, N, generator=g)


@pytest.mark.parametrize("B,k,N", BMM_CASES)
def test_bmm_matches_float64(B, k, N):
    """y, dx, dT within 2e-5.  Observed worst _rel on the MI355X: y 6.2e-7, dx 5.1e-7, dT 1.4e-7."""
    from pcr_amd import train_ops as TO
    x0, T0, go = _bmm_input(B, k, N)
    runs = []
    for _ in range(2):
        x, T = x0.cuda().requires_grad_(True), T0.cuda().requires_grad_(True)
        y = TO.Bmm.apply(x, T)
        runs.append([y.detach()] + list(torch.autograd.grad(y, [x, T], go.cuda())))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    x64, T64, g64 = x0.to(F64), T0.to(F64), go.to(F64)
    want = [R.bmm_ref(x64, T64)] + list(R.bmm_bwd_ref(x64, T64, g64))
    worst = {k_: _vs(a, b) for k_, a, b in zip(("y", "dx", "dT"), runs[0], want)}
    _report("Bmm", (B, k, N), worst)
    assert max(worst.values()) < BN_BOUND, worst


@pytest.mark.parametrize("B,k,N", [(5, 3, 128), (1, 64, 65), (1, 128, 65)])
@pytest.mark.parametrize("need_x,need_T", [(True, False), (False, True), (True, True)])
def test_bmm_backward_computes_only_what_is_asked(B, k, N, need_x, need_T):
    from pcr_amd import train_ops as TO
    x0, T0, go = _bmm_input(B, k, N)
    x, T = x0.cuda().requires_grad_(need_x), T0.cuda().requires_grad_(need_T)
    (TO.Bmm.apply(x, T) * go.cuda()).sum().backward()
    dx, dT = R.bmm_bwd_ref(x0.to(F64), T0.to(F64), go.to(F64))
    assert (x.grad is not None) == need_x and (T.grad is not None) == need_T
    if need_x:
        assert _vs(x.grad, dx) < BN_BOUND
    if need_T:
        assert _vs(T.grad, dT) < BN_BOUND


# ------------------------------------------------------------------------------ PoolBoth, ChannelMax --
@pytest.mark.parametrize("P,C,Ln", POOL_CASES)
def test_pool_both_matches_float64(P, C, Ln):
    """maxima and arg exact; means and the full backward within 1e-6; the backward of the max half alone (the mean half
    given a zero gradient) is a routed copy: exact.  (The kernel compares float32 values as they are: no decision is
    marginal, nothing to condition.)  Observed worst _rel on the MI355X: mean 1.0e-7, backward 5.1e-8."""
    from pcr_amd import train_ops as TO
    inp = make_pool_input(P, C, Ln)
    go_max = inp["go"].clone()
    go_max[:, C:] = 0.0
    want, arg64 = R.pool_both_ref(inp["o"].to(F64))
    runs = []
    for _ in range(2):
        o = inp["o"].cuda().requires_grad_(True)
        pooled = TO.PoolBoth.apply(o)
        assert torch.equal(_saved_arg(pooled, (P, C)), arg64)
        runs.append([pooled.detach(), torch.autograd.grad(pooled, o, inp["go"].cuda(), retain_graph=True)[0],
                     torch.autograd.grad(pooled, o, go_max.cuda())[0]])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    pooled, dout, dout_max = (t.cpu() for t in runs[0])
    assert torch.equal(pooled[:, :C].to(F64), want[:, :C])
    assert torch.equal(dout_max.to(F64), R.pool_both_bwd_ref(go_max.to(F64), arg64, Ln))
    worst = dict(mean=_rel(pooled[:, C:].to(F64), want[:, C:]),
                 dout=_rel(dout.to(F64), R.pool_both_bwd_ref(inp["go"].to(F64), arg64, Ln)))
    _report("PoolBoth", (P, C, Ln), worst)
    assert max(worst.values()) < MEAN_BOUND, worst


def test_pool_both_as_the_transform_nets_use_it():
    """the STN's max over the points: PoolBoth.apply(h)[:, :C] -- the slice hands the mean half a zero gradient"""
    from pcr_amd import train_ops as TO
    P, C, Ln = 8, 1024, 128
    inp = make_pool_input(P, C, Ln)
    want, arg64 = R.pool_both_ref(inp["o"].to(F64))
    h = inp["o"].cuda().requires_grad_(True)
    got = TO.PoolBoth.apply(h)[:, :C]
    go = inp["go"][:, :C].contiguous()
    dh, = torch.autograd.grad(got, h, go.cuda())
    assert torch.equal(got.detach().cpu().to(F64), want[:, :C])
    full = torch.cat([go, torch.zeros_like(go)], dim=1).to(F64)
    assert torch.equal(dh.cpu().to(F64), R.pool_both_bwd_ref(full, arg64, Ln))


@pytest.mark.parametrize("B,C,Ln,W", CMAX_CASES)
def test_channel_max_matches_float64(B, C, Ln, W):
    """values, the winning channel and the routed gradient: all exact"""
    from pcr_amd import train_ops as TO
    inp = make_cmax_input(B, C, Ln, W)
    want, arg64 = R.channel_max_ref(inp["x"].to(F64), W)
    runs = []
    for _ in range(2):
        x = inp["x"].cuda().requires_grad_(True)
        y = TO.ChannelMax.apply(x, W)
        assert torch.equal(_saved_arg(y, (B, C // W, Ln)), arg64)
        runs.append([y.detach(), torch.autograd.grad(y, x, inp["go"].cuda())[0]])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][0].cpu().to(F64), want)
    assert torch.equal(runs[0][1].cpu().to(F64), R.channel_max_bwd_ref(inp["go"].to(F64), arg64, C))


def test_pooling_of_no_clouds_returns_empty_tensors():
    from pcr_amd import train_ops as TO
    o = torch.empty(0, 64, 128, device="cuda").requires_grad_(True)
    pooled = TO.PoolBoth.apply(o)
    assert tuple(pooled.shape) == (0, 128) and pooled.dtype == torch.float32
    assert tuple(torch.autograd.grad(pooled, o, torch.empty(0, 128, device="cuda"))[0].shape) == (0, 64, 128)
    x = torch.empty(0, 64, 128, device="cuda").requires_grad_(True)
    y = TO.ChannelMax.apply(x, 2)
    assert tuple(y.shape) == (0, 32, 128) and y.dtype == torch.float32
    assert tuple(torch.autograd.grad(y, x, torch.empty(0, 32, 128, device="cuda"))[0].shape) == (0, 64, 128)
