"""float64 restatement of one ball-query scale of a PointSAModule in TRAINING mode (pcr_amd.train_ops.SaGroupTrain), of the
two first-layer launches it adds (pcr_sa_l1c_fwd_f32 / pcr_sa_l1c_bwd_f32) and of a whole PointNet2SSG train_step; the
case tables and input builders the CPU and GPU tests share; planted faults; the conditioning of the module cases.
Plain torch on the CPU; nothing here imports pcr_amd.  Selections, BatchNorm and the conditioning rules are train_ref's.

The scale, as mmdet3d's QueryAndGroup(use_xyz) + three ConvModules + max do it: rows [xyz_i - xyz_centre, f_i] for the K
indices of every centre (rows k >= cnt are the ball query's copies of row 0), conv / BatchNorm2d with batch statistics
over ALL B S K rows / ReLU three times, max over K.  The max is a gather at the FIRST index attaining it, written out --
copies tie exactly, and torch.max's backward is free to pick any of them.

Conditioning.  The inputs of the module are the cloud, the point features and the weights; an activation element cannot
be edited on its own.  A marginal decision of the float64 graph (train_ref's rule: a ReLU argument z within delta =
REL_DELTA max|z| of zero, or a winner of the max that leads the next DISTINCT value by less than delta while positive) is
removed by moving the row's own point: the smallest change of its features (of its coordinates where there are no
features, all exact copies of the point together, so a duplicate stays a duplicate) that puts z at +- 2 delta, by the
row's Jacobian with the batch statistics held.  That disturbs the other rows of the point a little, hence passes until
the float64 graph has none left.  Only DISTINCT rows k < cnt are looked at: a copy repeats its row 0's decision, and a tie
between copies of one row is not marginal -- parameter and table gradients do not depend on which copy wins."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import train_ref as R

F64 = torch.float64
EPS = 1e-5
MOMENTUM = 0.1
REL_DELTA = R.REL_DELTA
MOVE_CAP = 1e-3                    # conditioning may move this fraction of a case's elements, no more
PROD_BOUND = 1e-5                  # the launches (test_gpu_train_sa_ops.py)
BN_BOUND = 2e-5                    # BatchNorm compositions
BF_BOUND = 3e-5                    # where TRAIN_PRECISION puts the 128 x 128 backward on split bf16

# ---------------------------------------------------------------------------------------------- cases --
# the launches (B, N, S, K, c1): centre a permutation with every centre index >= S somewhere; odd everything; one live
# channel in the second chunk; N = 1100 (channel chunk 4: eight channels of 1100 floats are past the 32 KiB slice); K
# larger than the 64-row tile; K = 1.  Channel chunks these take: 32, 16 and 4.
L1C_SHAPES = [(3, 128, 64, 32, 32), (3, 100, 37, 20, 20), (2, 50, 7, 5, 33), (1, 1100, 32, 8, 6), (2, 40, 8, 96, 16),
              (2, 64, 64, 1, 32)]
# index sets: "ball" = D-FPS + ball query on `dup` clouds, "hot" = one point gathered by every row, "random"
# the other chunks (random and hot sets): chunk 8 at the shape of config 2's first scale (N = 1024), chunk 2 with one live
# channel in the second chunk, chunk 1
L1C_CHUNK_SHAPES = [(1, 1024, 32, 8, 12), (1, 2100, 16, 4, 3), (1, 4100, 8, 4, 2)]
L1C_VARIANTS = ((True, True), (True, False), (False, True), (False, False))        # (with tab, with bias)
L1C_CASES = [(s, "random", t, b) for s in L1C_SHAPES for t, b in L1C_VARIANTS] + \
            [(s, v, True, False) for s in L1C_SHAPES for v in ("ball", "hot")] + [(L1C_SHAPES[0], "ball", False, False)] + \
            [(s, "random", t, b) for s in L1C_CHUNK_SHAPES for t, b in ((True, True), (False, False))] + \
            [(s, "hot", True, False) for s in L1C_CHUNK_SHAPES]
BALL_RADIUS = 0.3                  # every shape then has centres with cnt < K, with cnt = 1 and (N = 1100) with cnt = K
# the module: MLP widths (mlp[0] = point features), N, S, radius, K, B, cloud kind
MODULE_CASES = [dict(mlp=[0, 16, 32, 64], N=300, S=96, r=0.5, K=16, B=3, kind="dup"),
                dict(mlp=[6, 32, 32, 64], N=300, S=96, r=0.5, K=16, B=3, kind="dup"),
                dict(mlp=[64, 128, 128, 256], N=128, S=32, r=0.8, K=64, B=2, kind="box"),
                # layers 2 and 3 on the wave-autonomous kernels (the GPU test lowers their block threshold), layer 3 taking
                # the max over K inside its launch: 32 / 64 channels, K >= 32, clouds of whole 32-token blocks
                dict(mlp=[6, 32, 32, 64], N=128, S=32, r=0.8, K=32, B=2, kind="dup", stream=True)]
# the model of the step test
MODEL_BACKBONE = dict(type="PointNet2SSG", num_points=(128, 64), radii=(0.4, 0.8), num_samples=(8, 32),
                      sa_channels=((16, 16, 32), (32, 32, 64)), trainable=True)
MODEL_PAIRS, MODEL_N = 4, 256
FAULTS = ("centre_is_s", "stats_without_copies", "dtab_without_copies", "route_to_every_copy")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ------------------------------------------------------------------------------------------- indexing --
def genuine_count(idx):
    """(B,S,K) ball-query indices -> (B,S) genuine hits: the query fills all K slots with the first hit and then writes
    the hits, distinct points, in order -- slots k >= cnt still hold slot 0's index"""
    return 1 + (idx[..., 1:] != idx[..., :1]).sum(dim=-1)


def copy_mask(idx):
    """(B,S,K) bool: slot k is a copy of slot 0 (k >= cnt)"""
    K = idx.shape[-1]
    return torch.arange(K).view(1, 1, K) >= genuine_count(idx).unsqueeze(-1)


def gather_cols(t, idx):
    """t (B,C,N), idx (B,S,K) -> (B,C,S,K)"""
    B, C, _ = t.shape
    _, S, K = idx.shape
    return torch.gather(t, 2, idx.long().reshape(B, 1, S * K).expand(B, C, S * K)).view(B, C, S, K)


def dxyz(xyz, idx, centre):
    """(B,3,S,K): xyz[idx] - xyz[centre]"""
    xt = xyz.transpose(1, 2)
    c = torch.gather(xt, 2, centre.long().unsqueeze(1).expand(-1, 3, -1))
    return gather_cols(xt, idx) - c.unsqueeze(3)


def group_rows(xyz, feats, idx, centre):
    """the gathered input of the grouped MLP, [dxyz, f_i]: (B, 3 + D, S, K)"""
    d = dxyz(xyz, idx, centre)
    return d if feats is None else torch.cat([d, gather_cols(feats, idx)], dim=1)


def sa_l1c_ref(xyz, idx, centre, tab, wa, bias):
    """pcr_sa_l1c_fwd_f32 as include/pcr.h states it: y[b,c,s K + k] = wa[c] . (xyz[idx] - xyz[centre[b,s]]) + tab[b,c,idx]
    (+ bias[c]): (B,c1,S K)"""
    B, S, K = idx.shape
    y = torch.einsum("cj,bjsk->bcsk", wa, dxyz(xyz, idx, centre))
    if tab is not None:
        y = y + gather_cols(tab, idx)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y.reshape(B, wa.shape[0], S * K)


# ------------------------------------------------------------------------------------------ the scale --
def _bn_batch(y, gamma, beta, w=None):
    """BatchNorm over (B,S,K) with batch statistics -> (z, mean, unbiased variance, scale); w (B,1,S,K) 0/1: the
    statistics over the rows with w = 1 only (a planted fault)"""
    if w is None:
        z, mean, var, scale = R._bn(y, gamma, beta, EPS, (0, 2, 3))
        n = y.shape[0] * y.shape[2] * y.shape[3]
        return z, mean.detach(), R._unbiased(var.detach(), n), scale
    n = w.sum()
    mean = (y * w).sum(dim=(0, 2, 3), keepdim=True) / n
    var = (((y - mean) ** 2) * w).sum(dim=(0, 2, 3), keepdim=True) / n
    scale = gamma.view(1, -1, 1, 1) / torch.sqrt(var + EPS)
    return scale * (y - mean) + beta.view(1, -1, 1, 1), mean.flatten().detach(), R._unbiased(var.flatten().detach(), n), scale


def scale_ref(layers, xyz, feats, idx, centre, running=False, fault=None):
    """layers: three dicts W (cout,cin), b (cout) or None, gamma, beta (and mean, var for `running`).  -> dict(out
    (B,c3,S), arg (B,c3,S) the first winning k, stats [(batch mean, unbiased variance)] x 3, z [(B,c,S,K)] x 3 the ReLU
    arguments, scale [(1,c,1,1)] x 3).  fault: one of FAULTS, the planted wrong readings."""
    B, S, K = idx.shape
    copies = copy_mask(idx).unsqueeze(1)                                   # (B,1,S,K)
    if fault == "centre_is_s":
        centre = torch.arange(S, dtype=centre.dtype).view(1, S).expand(B, S)
    h = group_rows(xyz, feats, idx, centre)
    if fault == "dtab_without_copies":
        h = torch.where(copies, h.detach(), h)                             # the copies' rows carry nothing back to the table
    stats, zs, scales = [], [], []
    for p in layers:
        y = torch.einsum("oc,bcsk->bosk", p["W"], h)
        if p.get("b") is not None:
            y = y + p["b"].view(1, -1, 1, 1)
        if running:
            scale = (p["gamma"] / torch.sqrt(p["var"] + EPS)).view(1, -1, 1, 1)
            z = scale * (y - p["mean"].view(1, -1, 1, 1)) + p["beta"].view(1, -1, 1, 1)
        else:
            w = (~copies).to(y.dtype) if fault == "stats_without_copies" else None
            z, mean, unb, scale = _bn_batch(y, p["gamma"], p["beta"], w)
            stats.append((mean, unb))
        zs.append(z)
        scales.append(scale.detach())
        h = torch.relu(z)
    # the first index attaining the maximum, among the DISTINCT rows: a copy holds its row 0's value exactly and comes
    # after it, so it never wins -- stated here, because the batched float64 products of this restatement may round a copy's
    # value one unit away from its row 0's (seen: 1.2696046259484979 against ...972), which is no property of the graph
    arg = R.first_argmax(torch.where(copies, torch.full_like(h, -float("inf")), h).detach(), 3)
    out = torch.gather(h, 3, arg.unsqueeze(3)).squeeze(3)
    if fault == "route_to_every_copy":
        # the value is the maximum; its gradient goes to every slot that holds the winner's point
        won = torch.gather(idx.long().unsqueeze(1).expand(-1, h.shape[1], -1, -1), 3, arg.unsqueeze(3))
        tie = (idx.long().unsqueeze(1) == won).to(h.dtype)
        out = (h * tie).sum(dim=3) - (tie.sum(dim=3) - 1.0) * out.detach()
    return dict(out=out, arg=arg, stats=stats, z=zs, scale=scales)


def layers_of(sd, prefix="mlps.0.", dtype=F64, grad=False):
    """the three layers of a state dict (conv weights as matrices) in `dtype`, as leaves when `grad`"""
    def t(k):
        v = sd.get(prefix + k)
        if v is None:
            return None
        v = v.detach().cpu().to(dtype)
        return v.requires_grad_(True) if grad else v
    out = []
    for j in range(3):
        W = t("layer%d.conv.weight" % j)
        p = dict(W4=W, W=W.view(W.shape[0], -1), b=t("layer%d.conv.bias" % j), gamma=t("layer%d.bn.weight" % j),
                 beta=t("layer%d.bn.bias" % j))
        p["mean"] = sd[prefix + "layer%d.bn.running_mean" % j].detach().cpu().to(dtype)
        p["var"] = sd[prefix + "layer%d.bn.running_var" % j].detach().cpu().to(dtype)
        out.append(p)
    return out


def scale_outputs(sd, xyz, feats, idx, centre, w, fault=None, dtype=F64):
    """everything the module test compares, in `dtype`: out, arg, running statistics after ONE step from sd's, the
    gradient of sum(out w) for every conv / BatchNorm parameter (state-dict names, mlps.0. dropped) and `feats`"""
    layers = layers_of(sd, dtype=dtype, grad=True)
    f = None if feats is None else feats.to(dtype).requires_grad_(True)
    r = scale_ref(layers, xyz.to(dtype), f, idx, centre, fault=fault)
    names, leaves = [], []
    for j, p in enumerate(layers):
        for key, n in (("W4", "conv.weight"), ("b", "conv.bias"), ("gamma", "bn.weight"), ("beta", "bn.bias")):
            if p[key] is not None:
                names.append("grad:layer%d.%s" % (j, n))
                leaves.append(p[key])
    if f is not None:
        names.append("grad:feats")
        leaves.append(f)
    grads = torch.autograd.grad((r["out"] * w.to(dtype)).sum(), leaves)
    res = dict(out=r["out"].detach(), arg=r["arg"])
    for j, (p, (mean, unb)) in enumerate(zip(layers, r["stats"])):
        res["layer%d.bn.running_mean" % j] = R.running_update(p["mean"], mean, MOMENTUM)
        res["layer%d.bn.running_var" % j] = R.running_update(p["var"], unb, MOMENTUM)
    res.update(zip(names, grads))
    return res


# ------------------------------------------------------------------------------------ conditioning --
def _decisions(layers, xyz, feats, idx, centre, rel=REL_DELTA, own_side=True):
    """the marginal decisions of the float64 graph on these float32 inputs, among the distinct rows:
    -> (entries [(layer l, b, c, s, k, wanted change of z_l[b,c,s,k])] as tensors per layer, forward record)"""
    r = scale_ref(layers, xyz.to(F64), None if feats is None else feats.to(F64), idx, centre)
    distinct = ~copy_mask(idx).unsqueeze(1)
    out = []
    for l, (z, scale) in enumerate(zip(r["z"], r["scale"])):
        delta = rel * float(z.abs().max())
        marg = (z.abs() < delta) & distinct & (scale != 0)
        b, c, s, k = torch.nonzero(marg, as_tuple=True)
        zz = z[b, c, s, k]
        ent = [(b, c, s, k, 2.0 * delta * (R._sign(zz) if own_side else 1.0) - zz)]
        if l == 2:
            # the winner against the next DISTINCT VALUE among the distinct rows (rows of bit-equal points tie exactly:
            # the first-index rule's case, left alone and raised together)
            zd = torch.where(distinct, z, torch.full_like(z, -float("inf")))
            mx = zd.amax(dim=3, keepdim=True)
            second = torch.where(zd < mx, zd, torch.full_like(zd, -float("inf"))).amax(dim=3, keepdim=True)
            near = (mx - second < delta) & (mx > 0) & (scale != 0)
            b, c, s, k = torch.nonzero(near & (zd == mx), as_tuple=True)
            ent.append((b, c, s, k, 2.0 * delta - (mx - second).expand_as(z)[b, c, s, k]))
        out.append(ent)
    return out, r


def count_marginals(layers, xyz, feats, idx, centre):
    ent, _ = _decisions(layers, xyz, feats, idx, centre)
    return sum(int(e[0].numel()) for per in ent for e in per)


def _row_jacobian(layers, r, l, b, c, s, k):
    """(E, 3 + D): d z_l[b,c,s,k] / d (the row's input), batch statistics held"""
    v = r["scale"][l].flatten()[c].unsqueeze(1) * layers[l]["W"][c]
    for j in range(l - 1, -1, -1):
        open_ = (r["z"][j][b, :, s, k] > 0).to(v.dtype)
        v = (v * open_ * r["scale"][j].flatten().unsqueeze(0)) @ layers[j]["W"]
    return v


def _coord_groups(xyz):
    """(B,N) int64: points of a cloud with bit-equal coordinates share a number"""
    out = []
    for cloud in xyz:
        _, inv = torch.unique(cloud, dim=0, return_inverse=True)
        out.append(inv)
    return torch.stack(out)


def condition_scale(layers, xyz, feats, query, max_passes=R.MAX_PASSES):
    """float32 xyz (B,N,3), feats (B,D,N) or None, query(xyz) -> (centre (B,S) int32, idx (B,S,K) int32)
    -> (xyz', feats', centre, idx, decisions moved, elements looked at).  See the module docstring."""
    moved = 0
    for pass_ in range(max_passes):
        centre, idx = query(xyz)
        # (two rows of one point whose z differ by less than 2 delta in a channel cannot both go to their own side: what is
        # still marginal after four passes goes to the positive side)
        ent, r = _decisions(layers, xyz, feats, idx, centre, own_side=pass_ < 4)
        n = sum(int(e[0].numel()) for per in ent for e in per)
        total = int((~copy_mask(idx)).sum()) * sum(p["W"].shape[0] for p in layers)
        if n == 0:
            return xyz, feats, centre, idx, moved, total
        moved += n
        B, N, _ = xyz.shape
        step = torch.zeros(B, N, 3 if feats is None else feats.shape[1], dtype=F64)
        for l, per in enumerate(ent):
            for b, c, s, k, dz in per:
                if not b.numel():
                    continue
                jac = _row_jacobian(layers, r, l, b, c, s, k)
                jac = jac[:, :3] if feats is None else jac[:, 3:]
                nrm = (jac * jac).sum(dim=1, keepdim=True)
                assert bool((nrm > 0).all()), "a marginal row that its point cannot move (the centre's own row)"
                step.index_put_((b, idx[b, s, k].long()), dz.unsqueeze(1) * jac / nrm, accumulate=True)
        if feats is None:
            gid = _coord_groups(xyz)
            per_group = torch.zeros(B, N, 3, dtype=F64).scatter_add_(1, gid.unsqueeze(2).expand(-1, -1, 3), step)
            xyz = (xyz.to(F64) + torch.gather(per_group, 1, gid.unsqueeze(2).expand(-1, -1, 3))).to(torch.float32)
        else:
            feats = (feats.to(F64) + step.transpose(1, 2)).to(torch.float32)
    raise AssertionError("conditioning did not settle")


# ----------------------------------------------------------------------------------- input builders --
def clouds(B, N, seed, kind):
    """pcr_amd.testing.synthetic_clouds' `box` and `dup` clouds, restated (this file imports nothing of the product)"""
    g = np.random.default_rng([0x5EED, seed])
    a = g.uniform(-0.5, 0.5, (B, N, 3)) * np.array([4.0, 2.0, 1.5])
    if kind == "dup":
        half = N // 2
        for c in range(B):
            src = g.integers(0, half, N - half)
            a[c, half:] = a[c, src]
            a[c] = a[c, g.permutation(N)]
    return torch.from_numpy(a.astype(np.float32))


def oracle_query(S, radius, K):
    """query(xyz) by the C oracle's D-FPS and ball query (the device ops are pinned to it bit for bit)"""
    import point_ops as P

    def query(xyz):
        x = xyz.numpy()
        centre = P.fps(x, S)
        new_xyz = np.take_along_axis(x, centre[..., None].astype(np.int64).repeat(3, -1), 1)
        return torch.from_numpy(centre), torch.from_numpy(P.ball_query(0.0, radius, K, x, new_xyz))
    return query


def make_l1c_input(shape, index_set, with_tab, with_bias, query=None):
    """float32 CPU tensors of one launch case; query(xyz) serves the "ball" set"""
    B, N, S, K, c1 = shape
    g = _gen("l1c", shape, index_set, with_tab, with_bias)
    if index_set == "ball":
        xyz = clouds(B, N, 7, "dup")
        centre, idx = query(xyz)
    else:
        xyz = torch.randn(B, N, 3, generator=g)
        if S <= N:          # a permutation's head; cloud 0 takes the LAST S points, so every centre index is >= S when 2 S <= N
            centre = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)]).to(torch.int32)
            centre[0] = torch.arange(N - S, N, dtype=torch.int32)[torch.randperm(S, generator=g)]
        else:
            centre = torch.randint(0, N, (B, S), generator=g, dtype=torch.int32)
        idx = torch.full((B, S, K), N - 1, dtype=torch.int32) if index_set == "hot" else \
            torch.randint(0, N, (B, S, K), generator=g, dtype=torch.int32)
    Ln = S * K
    return dict(xyz=xyz, idx=idx.contiguous(), centre=centre.contiguous(),
                tab=torch.randn(B, c1, N, generator=g) if with_tab else None,
                wa=torch.randn(c1, 3, generator=g), bias=torch.randn(c1, generator=g) if with_bias else None,
                g=torch.randn(B, c1, Ln, generator=g), y=torch.randn(B, c1, Ln, generator=g),
                ka=torch.rand(c1, generator=g) + 0.5, kb=torch.randn(c1, generator=g) * 0.05,
                kc=torch.randn(c1, generator=g) * 0.05)


def l1c_want(inp):
    """-> (y, {dwa, dbias, dtab}) in float64: the forward on the inputs, the backward of dy = ka g + kb y + kc with the
    GIVEN y (the launches are two independent linear maps)"""
    d = lambda t: None if t is None else t.to(F64)                                    # noqa: E731
    wa = d(inp["wa"]).requires_grad_(True)
    bias = torch.zeros(wa.shape[0], dtype=F64, requires_grad=True)                    # (d bias is produced with or without one)
    tab = None if inp["tab"] is None else d(inp["tab"]).requires_grad_(True)
    y0 = sa_l1c_ref(d(inp["xyz"]), inp["idx"], inp["centre"], tab, wa, bias)
    dy = R.tdense_dy(1, d(inp["g"]), d(inp["y"]), {n: d(inp[n]) for n in ("ka", "kb", "kc")})
    grads = torch.autograd.grad(y0, [wa, bias] + ([tab] if tab is not None else []), dy)
    y64 = y0.detach() + (d(inp["bias"]).view(1, -1, 1) if inp["bias"] is not None else 0.0)
    return y64, dict(dwa=grads[0], dbias=grads[1], dtab=grads[2] if tab is not None else None)


def seeded_mlp_sd(mlp, seed):
    """state dict of PointSAModule(mlp_channels=mlp).mlps[0] -- names, shapes and value rules of
    pcr_amd.testing.seeded_state_dict (conv weights uniform in +- sqrt(3 / fan_in), BatchNorm gains 1 + 0.1 n, biases
    0.05 n, running mean 0.1 n, running variance in [0.5, 1.5]) from this file's own generator"""
    g = _gen("mlp", tuple(mlp), seed)
    sd, cin = {}, mlp[0] + 3
    for j, co in enumerate(mlp[1:]):
        p = "mlps.0.layer%d." % j
        bound = (3.0 / cin) ** 0.5
        sd[p + "conv.weight"] = (torch.rand(co, cin, 1, 1, generator=g) * 2 - 1) * bound
        sd[p + "bn.weight"] = 1.0 + 0.1 * torch.randn(co, generator=g)
        sd[p + "bn.bias"] = 0.05 * torch.randn(co, generator=g)
        sd[p + "bn.running_mean"] = 0.1 * torch.randn(co, generator=g)
        sd[p + "bn.running_var"] = torch.rand(co, generator=g) + 0.5
        sd[p + "bn.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
        cin = co
    return sd


@functools.lru_cache(maxsize=None)
def module_case(i):
    """the conditioned inputs of MODULE_CASES[i], built once: dict(sd, xyz, feats, centre, idx, w, moved, total, raw_xyz,
    raw_feats)"""
    c = MODULE_CASES[i]
    D = c["mlp"][0]
    g = _gen("module", i)
    sd = seeded_mlp_sd(c["mlp"], 5)
    xyz = clouds(c["B"], c["N"], (31, 12, 13, 14)[i], c["kind"])      # (seeds whose conditioning settles well inside MOVE_CAP)
    feats = torch.randn(c["B"], D, c["N"], generator=g) if D else None
    layers = layers_of(sd)
    cx, cf, centre, idx, moved, total = condition_scale(layers, xyz, feats, oracle_query(c["S"], c["r"], c["K"]))
    w = torch.randn(c["B"], c["mlp"][-1], c["S"], generator=g)
    return dict(sd=sd, xyz=cx, feats=cf, centre=centre, idx=idx, w=w, moved=moved, total=total, raw_xyz=xyz, raw_feats=feats)


# ------------------------------------------------------------------------------------ the whole step --
def backbone_train_ref(sd, pc, cfg, query_of, dtype=F64):
    """PointNet2SSG.forward in training mode on a state dict of leaves (prefix backbone.): -> (xyz, h (B,conv_out,M),
    [(batch mean, unbiased variance)] per BatchNorm in order)"""
    xyz, feats, stats = pc[..., :3].to(dtype), None, []
    for i, (S, r, K) in enumerate(zip(cfg["num_points"], cfg["radii"], cfg["num_samples"])):
        centre, idx = query_of(S, r, K)(xyz.to(torch.float32))
        p = "backbone.SA_modules.%d.mlps.0." % i
        layers = []
        for j in range(3):
            W = sd[p + "layer%d.conv.weight" % j]
            layers.append(dict(W=W.view(W.shape[0], -1), b=sd.get(p + "layer%d.conv.bias" % j),
                               gamma=sd[p + "layer%d.bn.weight" % j], beta=sd[p + "layer%d.bn.bias" % j]))
        res = scale_ref(layers, xyz, feats, idx, centre)
        stats += res["stats"]
        feats = res["out"]
        xyz = torch.gather(xyz, 1, centre.long().unsqueeze(2).expand(-1, -1, 3))
    return xyz, F.conv1d(feats, sd["backbone.cov_final.weight"], sd["backbone.cov_final.bias"]), stats


def step_ref(sd, s1, s2, match, cfg, query_of, dtype=F64):
    """one match-only train_step of a ReIDNet with the PointNet2SSG backbone in `dtype`: encoder with batch statistics,
    the matching head as model_oracle.match states it (LayerNorm / GroupNorm only: the same in train and eval mode),
    BCE-with-logits against `match`.  -> (loss, {name: gradient}, logits, BatchNorm batch statistics)"""
    import model_oracle as MO
    leaves = {k: (v.detach().cpu().to(dtype).requires_grad_(True) if v.is_floating_point() and "running_" not in k else v)
              for k, v in sd.items()}
    b = s1.shape[0]
    xyz, h, stats = backbone_train_ref(leaves, torch.cat([s1, s2], 0).to(dtype), cfg, query_of, dtype)
    xyz = xyz.detach()
    logits = MO.match(leaves, h[:b], xyz[:b], h[b:], xyz[b:])
    loss = F.binary_cross_entropy_with_logits(logits, match.to(dtype))
    names = [k for k, v in leaves.items() if torch.is_tensor(v) and v.requires_grad]
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return loss.detach(), {k: g for k, g in zip(names, grads) if g is not None}, logits.detach(), stats
