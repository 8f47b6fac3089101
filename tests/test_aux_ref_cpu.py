"""CPU: the float64 restatements of the cls / fp / kl / triplet losses (tests/aux_ref.py) against torch's own losses
composed as the reference composes them (ReIDNet.py:348-384, 467-482, 538-582), values and autograd gradients to 1e-12;
three planted faults are each seen; the draw rule of pcr.h has the properties the reference's torch.multinomial call has;
the new entry points are exported and refuse bad arguments without a device; shape / dense still raise."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import aux_ref as R

TOL = 1e-12


def _kl_torch(h, match):
    """get_kl_loss as the reference writes it (alpha = 1)"""
    B = h.shape[0] // 2
    kl = nn.KLDivLoss(log_target=True, reduction="none")
    lsmx = nn.LogSoftmax(dim=1)
    v = kl(lsmx(h[:B]), lsmx(h[B:])).mean(dim=1)
    no = torch.where(match == 0)
    v[no] = v[no] * -1
    return v[match == 0].mean() + v[match == 1].mean()


def _triplet_torch(h, neg, match, margin):
    """get_triplet_loss as the reference writes it, with the negatives given (alpha = 1)"""
    B, T = h.shape[0] // 2, neg.shape[1]
    idx = torch.where(match == 1)[0]
    a = torch.cat([torch.full((T,), int(i)) for i in idx])
    n = torch.cat([torch.as_tensor(neg[int(i)], dtype=torch.long) for i in idx])
    return nn.TripletMarginLoss(margin=margin, p=2)(anchor=h[:B][a], positive=h[B:][a], negative=h[n])


def _case(B=6, D=37, seed=0, scale=1.0, near=None):
    """near: the second half is the first plus noise of that size (a positive is closer than a negative, so the median
    margin is positive -- torch's triplet loss refuses any other)"""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(2 * B, D, generator=g, dtype=torch.float64) * scale
    if near is not None:
        h[B:] = h[:B] + near * torch.randn(B, D, generator=g, dtype=torch.float64)
    match = (torch.arange(B) % 3 != 1).float()
    return h.requires_grad_(), match


def _negatives(B, T, match, seed=1):
    rng = np.random.default_rng(seed)
    neg = np.full((B, T), -1, np.int64)
    for i in range(B):
        if match[i]:
            pool = [r for r in range(2 * B) if r not in (i, B + i)]
            neg[i] = rng.choice(pool, T, replace=len(pool) < T)
    return neg


@pytest.mark.parametrize("B,D,scale", [(3, 1, 1.0), (6, 37, 1.0), (5, 300, 30.0)])
def test_kl_restatement_matches_torch(B, D, scale):
    h, match = _case(B, D, scale=scale)
    want = _kl_torch(h, match)
    gw, = torch.autograd.grad(want, h)
    got, kl, _, _, info = R.kl_pairs(h, match)
    gg, = torch.autograd.grad(got, h)
    assert info == 0
    assert abs(float((got - want).detach())) < TOL
    assert float((gg - gw).abs().max()) < TOL
    assert float((R.kl_pairs_grad(h.detach(), match, g=1.0) - gw).abs().max()) < TOL
    assert float((R.kl_pairs_grad(h.detach(), match, g=-2.5) + 2.5 * gw).abs().max()) < 3 * TOL


def test_kl_empty_group_counts_as_zero():
    h, _ = _case()
    match = torch.ones(6)
    loss, kl, _, _, info = R.kl_pairs(h, match)
    assert info == R.INFO_KL_EMPTY and abs(float((loss - kl.mean()).detach())) < TOL
    assert torch.isnan(_kl_torch(h, match))                       # (what the reference gives: the documented deviation)


@pytest.mark.parametrize("B,D,T", [(6, 37, 4), (4, 5, 9), (5, 128, 3)])
def test_triplet_restatement_matches_torch(B, D, T):
    h, match = _case(B, D, seed=3, near=0.3)
    neg = _negatives(B, T, match)
    margin = R.median_margin(h.detach(), neg, match)
    gap, dmax = R.hinge_gaps(h.detach(), neg, match, margin)
    assert gap > 1e-9 * dmax
    want = _triplet_torch(h, neg, match, margin)
    gw, = torch.autograd.grad(want, h)
    got, dist, E, count, info = R.triplet(h, neg, match, margin)
    gg, = torch.autograd.grad(got, h)
    assert info == 0 and count == int(match.sum()) * T
    d = dist.detach()
    active = sum(float(d[i, B + i] - d[i, int(r)] + margin) > 0 for i in range(B) if match[i] for r in neg[i])
    assert 0 < active < count                                     # (active and inactive triplets both occur)
    assert abs(float((got - want).detach())) < TOL
    assert float((gg - gw).abs().max()) < TOL
    assert float((R.triplet_grad(h.detach(), E, count) - gw).abs().max()) < TOL
    # torch's own distance: pairwise_distance adds eps to the difference
    assert float((d[0] - nn.functional.pairwise_distance(h[:1].expand(2 * B, D), h).detach()).abs().max()) < TOL


def test_triplet_without_a_match_is_zero_and_flagged():
    h, _ = _case()
    loss, _, E, count, info = R.triplet(h, np.full((6, 4), -1), torch.zeros(6), 0.2)
    assert float(loss) == 0.0 and count == 0 and info == R.INFO_TRIPLET_NONE and not E.any()


def test_cls_and_fp_restatements_match_torch():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(12, 20, generator=g, dtype=torch.float64, requires_grad=True)
    labels = torch.arange(12) * 5 % 20
    want = nn.functional.cross_entropy(logits, labels)
    gw, = torch.autograd.grad(want, logits)
    got, grad = R.cross_entropy(logits.detach(), labels)
    assert abs(float((got - want).detach())) < TOL and float((grad - gw).abs().max()) < TOL
    x = (torch.randn(12, generator=g, dtype=torch.float64) * 4).requires_grad_()
    t = (labels > 9).double()
    want = nn.BCEWithLogitsLoss()(x, t)
    gw, = torch.autograd.grad(want, x)
    got, grad = R.bce_logits(x.detach(), t)
    assert abs(float((got - want).detach())) < TOL and float((grad - gw).abs().max()) < TOL


def test_object_head_accuracies_follow_the_reference_lines():
    """metrics.evaluate over forward_test outputs: val_cls_acc / val_fp_acc when the predictions are there
    (reidentification_base.py:150, :156), no entry when a head is off (forward_test returns None for it)"""
    from pcr_amd import metrics
    g = torch.Generator().manual_seed(9)
    batches = []
    for b in (3, 5):
        labels = torch.randint(0, 20, (2 * b,), generator=g)
        cls = torch.randn(2 * b, 20, generator=g)
        fp = torch.randn(2 * b, generator=g)
        batches.append(dict(val_match_preds=torch.randn(b, generator=g), val_match_gt=torch.randint(0, 2, (b,), generator=g).float(),
                            val_cls_preds=cls, val_cls_gt=labels, val_fp_preds=fp, val_fp_gt=(labels > 9).float()))
    out = metrics.evaluate(batches)
    r = metrics.accumulate(batches)
    assert out["val_cls_acc"] == r["val_cls_preds"].argmax(dim=1).eq(r["val_cls_gt"]).float().mean().item()
    assert out["val_fp_acc"] == (nn.Sigmoid()(r["val_fp_preds"]) > 0.5).float().eq(r["val_fp_gt"]).float().mean().item()
    off = metrics.evaluate([dict(b, val_cls_preds=None, val_fp_preds=None) for b in batches])
    assert "val_cls_acc" not in off and "val_fp_acc" not in off and off["val_match_acc"] == out["val_match_acc"]


def test_evaluate_model_gathers_the_object_heads(tmp_path):
    """evaluate_model keeps forward_test's per-object predictions per pair, so they shard and gather like the logits: the
    accuracies do not depend on the batch size and equal the two lines applied to one batch of everything"""
    import test_evaluate as TE
    from pcr_amd import evaluate as EV
    root = str(tmp_path / "crops")
    TE.write_toy_crops(root)
    ds, _ = EV.build_val_set(TE.VAL_CFG, root)

    class WithHeads(TE.Stub):
        losses_to_use = dict(match=True, cls=True, fp=True)

        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.cls_head = nn.Sequential(nn.Identity(), nn.Linear(3, 4))
            self.seen = []

        def forward(self, return_loss=True, **kw):
            (res,) = super().forward(return_loss, **kw)
            feats = torch.cat([torch.stack(kw["sparse_1"]), torch.stack(kw["sparse_2"])]).mean(dim=1)      # (2b, 3)
            labels = torch.cat(kw["label_1"] + kw["label_2"])
            res.update(val_cls_preds=self.cls_head(feats) * 50, val_cls_gt=labels % 4,
                       val_fp_preds=feats[:, 0] * 50, val_fp_gt=(feats[:, 1] > 0).float())
            self.seen.append(res)
            return [res]

    n = len(ds)
    whole = WithHeads()
    want = EV.evaluate_model(whole, ds, n, seed=5, device="cpu", rank=0, world=1)
    (res,) = whole.seen
    assert want["val_cls_acc"] == res["val_cls_preds"].argmax(dim=1).eq(res["val_cls_gt"]).float().mean().item()
    assert want["val_fp_acc"] == (torch.sigmoid(res["val_fp_preds"]) > 0.5).float().eq(res["val_fp_gt"]).float().mean().item()
    assert 0.0 < want["val_fp_acc"] < 1.0
    for bs in (16, 7):
        got = EV.evaluate_model(WithHeads(), ds, bs, seed=5, device="cpu", rank=0, world=1)
        assert got["val_cls_acc"] == want["val_cls_acc"] and got["val_fp_acc"] == want["val_fp_acc"]
    plain = EV.evaluate_model(TE.Stub(), ds, 16, seed=5, device="cpu", rank=0, world=1)
    assert "val_cls_acc" not in plain and "val_fp_acc" not in plain


def test_planted_faults_are_detected():
    h, match = _case(6, 37, seed=7, near=0.3)
    h = h.detach()
    want = float(_kl_torch(h, match))
    assert abs(float(R.kl_pairs(h, match, flip=False)[0]) - want) > 1e-6          # no sign flip for the non-matches
    B, T = 6, 4
    neg = _negatives(B, T, match)
    margin = R.median_margin(h.detach(), neg, match)
    want = float(_triplet_torch(h, neg, match, margin))
    assert abs(float(R.triplet(h, neg, match, margin)[0]) - want) < TOL
    assert abs(float(R.triplet(h, neg, match, margin, mean="all")[0]) - want) > 1e-6      # a mean over B T
    # eps dropped: invisible at distances of order ten, so look where the issue says it matters -- a positive ON its anchor
    hz = h.detach().clone()
    hz[B:] = hz[:B]
    want = float(_triplet_torch(hz, neg, match, 50.0))
    assert abs(float(R.triplet(hz, neg, match, 50.0)[0]) - want) < TOL
    assert abs(float(R.triplet(hz, neg, match, 50.0, eps=0.0)[0]) - want) > 1e-7
    assert float(R.pair_dist(hz[:1], hz[B:B + 1])) == pytest.approx(1e-6 * np.sqrt(37), rel=1e-12)


LAYOUTS = {
    # pool >= T: eight pairs, the first four match, every id its own
    "wide": (list(range(8)) + [0, 1, 2, 3, 104, 105, 106, 107], 4),
    # pool < T: one matching pair of an object seen four times, two strangers
    "narrow": ([5, 5, 5, 5, 9, 8], 4),
    # an empty pool: every row carries the same id
    "empty": ([7, 7, 7, 7], 3),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_draw_rule_properties(name):
    ids, T = LAYOUTS[name]
    B = len(ids) // 2
    match = [int(ids[i] == ids[B + i]) for i in range(B)]
    for seed in (0, 1, 1 << 40):
        neg, info = R.draw(ids, match, T, seed=seed)
        for i in range(B):
            pool = R.pool_of(ids, i)
            if not match[i] or not pool:
                assert (neg[i] == -1).all()
                continue
            assert all(ids[r] != ids[i] for r in neg[i])                       # no negative shares the anchor's id
            if len(pool) >= T:
                assert len(set(neg[i].tolist())) == T                         # distinct: without replacement
        assert bool(info & R.INFO_TRIPLET_POOL) == (name == "empty")
        assert (R.draw(ids, match, T, seed=seed)[0] == neg).all()
        if name != "empty":
            assert (R.draw(ids, match, T, rand=R.words_for(ids, match, neg))[0] == neg).all()     # the rand seam
    if name == "wide":
        assert (R.draw(ids, match, T, seed=0)[0] != R.draw(ids, match, T, seed=1)[0]).any()
        # every pool row is drawn about equally often over many seeds
        hits = np.zeros(2 * B)
        for seed in range(400):
            for r in R.draw(ids, match, T, seed=seed)[0][0]:
                hits[r] += 1
        assert hits[0] == hits[B] == 0 and hits[hits > 0].min() > 0.6 * 400 * T / (2 * B - 2)


NEW = ("pcr_kl_pairs_fwd_f32", "pcr_kl_pairs_bwd_f32", "pcr_triplet_ok", "pcr_triplet_draw_i32", "pcr_pair_dist_f32",
       "pcr_triplet_select_f32", "pcr_pair_dist_bwd_f32")


def test_new_symbols_are_exported_and_refuse_bad_arguments():
    from pcr_amd import _lib, abi, build
    build.build()
    lib = _lib.load()
    assert lib.pcr_abi_version() == 17
    for name in NEW:
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    n = None
    assert lib.pcr_kl_pairs_fwd_f32(n, n, n, n, n, n, n, n, 4, 8, n) == 1
    assert lib.pcr_kl_pairs_bwd_f32(n, n, n, n, n, n, n, 4, 8, n) == 1
    assert lib.pcr_triplet_draw_i32(n, n, n, n, n, n, 4, 8, n) == 1
    assert lib.pcr_pair_dist_f32(n, n, n, 4, 8, 16, n) == 1
    assert lib.pcr_triplet_select_f32(n, n, n, n, n, n, n, n, n, 4, 8, n) == 1
    assert lib.pcr_pair_dist_bwd_f32(n, n, n, n, n, n, n, n, 4, 8, 16, n) == 1
    assert lib.pcr_triplet_ok(256, 128) == 1 and lib.pcr_triplet_ok(4096, 128) == 1
    assert lib.pcr_triplet_ok(4097, 1) == 0 and lib.pcr_triplet_ok(0, 4) == 0 and lib.pcr_triplet_ok(4, 0) == 0
    # sizes are checked before pointers are looked at: a host address is never read
    buf = (abi.ctypes.c_int * 4)()
    p = abi.ctypes.cast(buf, abi.ctypes.c_void_p)
    assert lib.pcr_triplet_draw_i32(p, p, None, None, p, p, 5000, 4, None) == 1
    assert lib.pcr_kl_pairs_fwd_f32(p, p, p, p, p, p, p, p, 0, 8, None) == 1
    assert lib.pcr_pair_dist_f32(p, p, p, 4, 8, 0, None) == 1


def _cfg(**losses):
    import bench
    cfg = copy.deepcopy(bench.PT_MODEL)
    cfg["losses_to_use"] = dict(kl=False, match=True, cls=False, shape=False, fp=False, triplet=False, **losses)
    return cfg


@pytest.mark.parametrize("name", ["shape", "dense"])
def test_shape_and_dense_still_raise(name):
    from mmdet3d.models import build_model
    cfg = _cfg()
    cfg["losses_to_use"][name] = True
    m = build_model(cfg)
    with pytest.raises(NotImplementedError, match=name):
        m._check_losses()
    data = dict.fromkeys(("sparse_1", "sparse_2", "dense_1", "dense_2", "label_1", "label_2", "id_1", "id_2"), [])
    with pytest.raises(NotImplementedError, match=name):
        m.train().forward_train(**data)


def test_the_four_losses_pass_the_check_and_p_must_be_two():
    from mmdet3d.models import build_model
    from pcr_amd._lib import PcrError
    cfg = _cfg()
    cfg["losses_to_use"].update(kl=True, cls=True, fp=True, triplet=True)
    m = build_model(copy.deepcopy(cfg))
    m._check_losses()
    assert m._aux_on() and not build_model(_cfg())._aux_on()
    cfg["triplet_loss"] = dict(margin=10, p=1)
    with pytest.raises(PcrError, match="p = 1"):
        build_model(cfg)._check_losses()
    # no head built: a PcrError that names it, not an AttributeError
    m.losses_to_use.update(kl=False, triplet=False, fp=False)
    with pytest.raises(PcrError, match="cls_head must be"):
        m._object_head("cls", torch.zeros(2, 128))
