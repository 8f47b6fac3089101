"""GPU: the bookkeeping of the wave-autonomous K-row SA kernel (sa_stream_kernel), item shape by item shape.  A work item
is lcm(32, K) rows of one cloud, at most three 32-row blocks: K = 16 / 32 / 48 / 64 / 96 give 6 / 3 / 2 / 1 / 1 centres per
item.  The centre of a 16-row group is derived on the scalar unit, the group maxima fold into a running maximum per centre
in registers and leave from there, and every per-block load goes through a buffer resource with a 32-bit lane offset.  None
of that may move a bit: held here for every item shape, with a partial last item and with whole items only, for the five
width instantiations, without features, with in-launch layer 1, with tables that carry the coordinate term and with given
centres -- channel-major against point-major output, launch against launch, a cloud alone against the cloud in its batch,
claimed against dealt items -- and against a float64 restatement of the layer (models/pointnet2_utils.py:242-288, 333-360)
on the same indices, which a maximum over the wrong centre's groups must fail."""
import pytest
import torch
import torch.nn as nn

from pcr_amd import _lib as L
from pcr_amd import engine

pytestmark = pytest.mark.gpu

B, N, D = 11, 64, 32           # more clouds than XCD slots and no multiple of them: uneven shares for every slot
# (K, S): blocks per item / centres per item = 3/6, 3/3, 3/3, 3/2, 3/2, 2/1, 3/1; S with a partial last item, S in whole items
SHAPES = [(16, 8), (32, 7), (32, 9), (48, 5), (48, 6), (64, 3), (96, 2)]
WIDTHS = [(32, 32, 32), (64, 64, 64), (128, 128, 128), (32, 32, 64), (64, 64, 128)]
VARIANTS = ["no_features", "in_launch", "xyz_tables", "centre_idx"]
# the bound tests/test_gpu_sa_xyz_tables.py holds the K-row kernel to against plain torch (split bf16, of the result's scale)
BOUND = 2e-5

_plans = {}


def _layer(D, widths):
    key = (D, widths)
    if key not in _plans:
        g = torch.Generator().manual_seed(17 + D + sum(widths))
        torch.manual_seed(17 + D + sum(widths))  # (the convolutions' default initialisation draws from the global generator)
        cin = 3 + 2 * D
        convs = [nn.Conv2d(a, b, 1) for a, b in zip((cin,) + widths[:2], widths)]
        bns = [nn.BatchNorm2d(c) for c in widths]
        for bn, c in zip(bns, widths):
            bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            bn.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            bn.bias.data.copy_(torch.randn(c, generator=g) * 0.1)
            bn.eval()
        _plans[key] = (convs, bns, engine.SaPlan(convs, bns, torch.device("cuda"), 0))
    return _plans[key]


def _reference(convs, bns, xyz, feat, idx, cidx=None, regroup=None):
    """gather, three 1x1 convolutions with the BatchNorm folded in, ReLU, max over K -- float64 on the host.
    regroup (planted fault): the 16-row groups of consecutive centre pairs are dealt {0,1} / {2,..} instead of by centre"""
    nb, S, K = idx.shape
    li = idx.long().cpu()
    x64 = xyz.cpu().double()
    bidx = torch.arange(nb).view(nb, 1, 1)
    ci = (torch.arange(S).view(1, S).expand(nb, S) if cidx is None else cidx.long().cpu()).unsqueeze(2)   # (nb,S,1)
    parts = [x64[bidx, li] - x64[bidx, ci]]
    if feat is not None:
        f_pm = feat.cpu().double().transpose(1, 2)
        c_f = f_pm[bidx, ci].expand(-1, -1, K, -1)
        parts += [c_f, f_pm[bidx, li] - c_f]
    x = torch.cat(parts, dim=-1)                                        # (nb,S,K,cin)
    for conv, bn in zip(convs, bns):
        w = conv.weight.detach().double().reshape(conv.weight.shape[0], -1)
        sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        sh = (conv.bias.detach().double() - bn.running_mean.double()) * sc + bn.bias.detach().double()
        x = torch.relu(x @ (w * sc.unsqueeze(1)).t() + sh)
    if regroup is None:
        return x.max(dim=2)[0].transpose(1, 2)                          # (nb,c3,S)
    gpc = K // 16
    grp = x.reshape(nb, S // 2, 2 * gpc, 16, -1).max(dim=3)[0]         # the group maxima of an item of two centres
    out = torch.stack([grp[:, :, :regroup].max(dim=2)[0], grp[:, :, regroup:].max(dim=2)[0]], dim=2)
    return out.reshape(nb, S, -1).transpose(1, 2)


def _inputs(K, S, n=N, seed=0):
    g = torch.Generator().manual_seed(1000 * K + S + seed)
    xyz = torch.randn(B, n, 3, generator=g)
    feat = torch.randn(B, D, n, generator=g)
    idx = torch.randint(0, n, (B, S, K), generator=g, dtype=torch.int32)    # (a max over K does not ask for neighbours)
    cidx = torch.stack([torch.randperm(n, generator=g)[:S] for _ in range(B)]).to(torch.int32)
    return xyz.cuda(), feat.cuda(), idx.cuda(), cidx.cuda()


def _cases():
    for K, S in SHAPES:
        for w in WIDTHS:
            for v in VARIANTS:
                if v == "xyz_tables" and w[2] != w[1]:
                    continue            # (the dispatcher takes such tables for equal widths only: asserted below)
                yield pytest.param(K, S, w, v, id="K%d-S%d-%d_%d_%d-%s" % ((K, S) + w + (v,)))


def test_which_shapes_take_tables_with_the_coordinate_term():
    lib = L.load()
    bf = engine.PRECISIONS["bf16x3"]
    for K, _ in SHAPES:
        for w in WIDTHS:
            assert lib.pcr_sa_tables_take_xyz(0, D, w[0], w[1], w[2], K, bf) == (1 if w[2] == w[1] else 0)


@pytest.mark.parametrize("K,S,widths,variant", list(_cases()))
def test_every_item_shape_keeps_its_bits_and_its_value(K, S, widths, variant, monkeypatch):
    xyz, feat, idx, cidx = _inputs(K, S)
    if variant == "no_features":
        feat = None
    convs, bns, plan = _layer(0 if feat is None else D, widths)
    kw = dict(centre_idx=cidx) if variant == "centre_idx" else {}
    monkeypatch.setattr(engine, "SA_XYZ_TABLES", variant in ("xyz_tables", "centre_idx"))
    with engine.precision("bf16x3"), torch.no_grad():
        cm = plan.run(xyz, feat, idx, **kw)
        cm2 = plan.run(xyz, feat, idx, **kw)
        pm = plan.run(xyz, feat, idx, out_point_major=True, **kw)
        alone = {}
        for b in (0, B - 1):
            kb = dict(centre_idx=cidx[b:b + 1].contiguous()) if kw else {}
            alone[b] = plan.run(xyz[b:b + 1].contiguous(), None if feat is None else feat[b:b + 1].contiguous(),
                                idx[b:b + 1].contiguous(), **kb)
    assert cm.shape == (B, widths[2], S) and torch.isfinite(cm).all()
    assert torch.equal(cm, cm2), "two launches differ"
    assert pm.transpose(1, 2).is_contiguous() and torch.equal(cm, pm), "channel-major and point-major output differ"
    for b, o in alone.items():
        assert torch.equal(o[0], cm[b]), "cloud %d alone differs from the cloud in its batch" % b
    want = _reference(convs, bns, xyz, feat, idx, cidx if kw else None)
    err, scale = float((cm.cpu().double() - want).abs().max()), float(want.abs().max())
    print("K=%d S=%d %s %s: max |kernel - float64| = %.3g of scale %.3g (%.3g of the bound)" % (
        K, S, widths, variant, err, scale, err / (BOUND * scale)))
    assert err <= BOUND * scale


@pytest.mark.parametrize("widths", [(32, 32, 32), (64, 64, 64)])    # (the library claims items for equal widths <= 64 only)
@pytest.mark.parametrize("with_feat", [False, True])
def test_claimed_and_dealt_walks_give_the_same_bits(widths, with_feat, monkeypatch):
    n, S, K = 1024, 6, 48
    lib = L.load()
    assert lib.pcr_sa_claim_ws_ints(widths[0], widths[1], widths[2], K, n, engine.PRECISIONS["bf16x3"]) > 0
    xyz, feat, idx, _ = _inputs(K, S, n=n, seed=1)
    convs, bns, plan = _layer(D if with_feat else 0, widths)
    feat = feat if with_feat else None
    with engine.precision("bf16x3"), torch.no_grad():
        monkeypatch.setattr(engine, "SA_CLAIMS", True)
        a = plan.run(xyz, feat, idx)
        a_pm = plan.run(xyz, feat, idx, out_point_major=True)
        monkeypatch.setattr(engine, "SA_CLAIMS", False)
        d = plan.run(xyz, feat, idx)
    assert torch.isfinite(a).all() and torch.equal(a, d) and torch.equal(a, a_pm)
    want = _reference(convs, bns, xyz, feat, idx)
    assert float((a.cpu().double() - want).abs().max()) <= BOUND * float(want.abs().max())


@pytest.mark.parametrize("widths", [(32, 32, 32), (64, 64, 128)])
def test_a_maximum_over_the_wrong_centres_groups_exceeds_the_bound(widths):
    """K = 48: the two centres of an item own the groups {0,1,2} and {3,4,5} of its three blocks.  A reference that deals them
    {0,1} and {2,..,5} is what a kernel with an off-by-one in that bookkeeping would compute: the bound must tell the two apart"""
    K, S = 48, 6
    xyz, feat, idx, _ = _inputs(K, S)
    convs, bns, plan = _layer(D, widths)
    with engine.precision("bf16x3"), torch.no_grad():
        got = plan.run(xyz, feat, idx).cpu().double()
    want = _reference(convs, bns, xyz, feat, idx)
    same = _reference(convs, bns, xyz, feat, idx, regroup=3)
    wrong = _reference(convs, bns, xyz, feat, idx, regroup=2)
    scale = float(want.abs().max())
    assert torch.equal(same, want)                                      # (the regrouping itself restates the reference)
    assert float((got - want).abs().max()) <= BOUND * scale
    err = float((got - wrong).abs().max())
    print("planted fault %s: %.3g of the scale, %.3g of the bound" % (widths, err / scale, err / (BOUND * scale)))
    assert err > BOUND * scale
