"""GPU: ReIDNet.match_gallery for the three one-way matching heads of the reference's baseline configs -- `concat`
(reid_pts_point-transformer_baseline.py), `xcorr-baseline` (..._baseline_stnet.py) and `xcorr` (..._baseline_orig.py) --
against the goldens recorded from the imported reference and against match_forward_inference on the gathered tensors.
Pair (i, j) means match_forward_inference(h[i:i+1], h[j:j+1], xyz[i:i+1], xyz[j:j+1]), i the search side.
The model dicts restate the config files' `model` entries, as tests/test_gpu_config_variants.py / test_gpu_dgcnn.py /
test_gpu_train_variants.py do."""
import copy
import os

import numpy as np
import pytest
import torch

import rank_ref
from conftest import GOLDEN, load_golden
from pcr_amd import testing as T

pytestmark = pytest.mark.gpu
TOL = 1e-4            # the project's parity bound against the imported reference
BOUND = 2e-6          # bound (1) of tests/test_gpu_dense_forms.py: max|a - b| / max|b| of one f32 launch form

BASELINE = dict(
    type="ReIDNet", hidden_size=128, combine="cat", match_type="concat", output_sequence_size=64,
    backbone=dict(type="Pointnet_Backbone", input_channels=0, use_xyz=True, conv_out=64),
    backbone_list=[128, 64, 32], pool_type="max", downsample=None, cls_head=None, fp_head=None,
    match_head=[dict(type="LinearRes", n_in=256, n_out=256, norm="GN", ng=32),
                dict(type="Linear", in_features=256, out_features=1)],
    shape_head=None, cross_stage1=None, cross_stage2=None, local_stage1=None, local_stage2=None)

PT = dict(
    type="ReIDNet", hidden_size=128, combine="point-cat", match_type="xcorr_eff", pool_type="both",
    backbone_list=[128, 64, 32], output_sequence_size=64,
    backbone=dict(type="Pointnet_Backbone", input_channels=0, use_xyz=True, conv_out=64),
    match_head=[dict(type="LinearRes", n_in=128, n_out=128, norm="GN", ng=8),
                dict(type="Linear", in_features=128, out_features=1)],
    downsample=None, cls_head=None, fp_head=None, shape_head=None,
    cross_stage1=dict(type="corss_attention", d_model=64, nhead=2, attention="linear"),
    cross_stage2=dict(type="corss_attention", d_model=64, nhead=2, attention="linear"),
    local_stage1=dict(), local_stage2=dict())
LOCAL = dict(type="local_self_attention", d_model=64, nhead=2, attention="linear", knum=48, pos_size=64)
STNET = dict(copy.deepcopy(PT), match_type="xcorr-baseline")
ORIG = dict(copy.deepcopy(PT), match_type="xcorr", local_stage1=dict(LOCAL), local_stage2=dict(LOCAL))

HEADS = {"concat": (BASELINE, "pt_baseline"), "xcorr-baseline": (STNET, "pt"), "xcorr": (ORIG, "pt_xcorr")}
_MODELS = {}


def model_of(head):
    if head not in _MODELS:
        from mmdet3d.models import build_model
        cfg, manifest = HEADS[head]
        m = build_model(copy.deepcopy(cfg))
        man = T.load_manifest(os.path.join(GOLDEN, manifest + "_manifest.json"))
        assert T.manifest_of(m) == man, "state_dict names/shapes differ from the reference's"
        m.load_state_dict(T.seeded_state_dict(man, 0), strict=True)
        _MODELS[head] = m.cuda().eval()
    return _MODELS[head]


def golden_gallery(m, name):
    """the golden's pairs as a gallery [h1 ; h2] with the pair list (p, P + p)"""
    g = load_golden(name)
    meta = g["meta"]
    s1, s2 = T.synthetic_pairs(meta["pairs"], meta["n"], meta["input_seed"], meta["kind"])
    with torch.no_grad():
        xyz1, xyz2, h1, h2 = m.siamese_forward(s1.cuda(), s2.cuda())
    P = meta["pairs"]
    pairs = torch.stack([torch.arange(P), torch.arange(P) + P], dim=1).to(torch.int32).cuda()
    return g, torch.cat([h1, h2]).contiguous(), torch.cat([xyz1, xyz2]).contiguous(), pairs


def gathered(m, h, xyz, pairs):
    i, j = pairs[:, 0].long(), pairs[:, 1].long()
    return m.match_forward_inference(h[i].contiguous(), h[j].contiguous(), xyz[i].contiguous(), xyz[j].contiguous())


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


MIXED = [(0, 4), (4, 0), (1, 5), (1, 5), (2, 2), (7, 3), (3, 7), (6, 1), (0, 4)]     # repeats, (i, j) with (j, i), i == j


def test_concat_gallery_matches_the_reference_golden():
    from pcr_amd import engine
    m = model_of("concat")
    g, h, xyz, pairs = golden_gallery(m, "pt_baseline_n128_randn")
    with torch.no_grad():
        got = m.match_gallery(h, xyz, pairs)
        emb = m.embed(h)
        via_emb = m.match_embeddings(emb, pairs)
        with engine.precision("f32"):
            direct = gathered(m, h, xyz, pairs)
        mixed = torch.tensor(MIXED, dtype=torch.int32, device="cuda")
        got_mixed = m.match_gallery(h, xyz, mixed)
        with engine.precision("f32"):
            direct_mixed = gathered(m, h, xyz, mixed)
    d_gold = float(np.abs(got.cpu().numpy() - g["logits"]).max())
    print("concat: |gallery - golden| %.3g, gallery vs match_forward_inference(f32) %.3g / %.3g of scale"
          % (d_gold, rel(got, direct), rel(got_mixed, direct_mixed)))
    assert d_gold < TOL
    assert rel(got, direct) <= BOUND and rel(got_mixed, direct_mixed) <= BOUND
    assert emb.shape == (2 * g["meta"]["pairs"], 128)
    assert float(np.abs(emb[:g["meta"]["pairs"]].cpu().numpy() - g["pooled1"]).max()) < TOL
    assert torch.equal(via_emb, got)
    assert not torch.equal(got_mixed[0], got_mixed[1])                   # (0, 4) against (4, 0): the head is one-way
    from pcr_amd._lib import PcrError
    with pytest.raises(PcrError):                                        # a 3-D pool
        m.embed(torch.zeros(2, 130, 128, device="cuda"))


def test_xcorr_gallery_matches_the_reference_golden_and_the_pairwise_entry():
    from pcr_amd import engine
    m = model_of("xcorr")
    g, h, xyz, pairs = golden_gallery(m, "pt_xcorr_n128_randn")
    mixed = torch.tensor(MIXED, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        got = m.match_gallery(h, xyz, pairs)
        got_mixed = m.match_gallery(h, xyz, mixed)
        with engine.precision("f32"):
            f32_gallery = m.match_gallery(h, xyz, pairs)
            f32_mixed = m.match_gallery(h, xyz, mixed)
            f32_direct = gathered(m, h, xyz, mixed)
    print("xcorr: |gallery - golden| %.3g, default vs f32 %.3g"
          % (float(np.abs(got.cpu().numpy() - g["logits"]).max()), float((got_mixed - f32_mixed).abs().max())))
    assert float(np.abs(got.cpu().numpy() - g["logits"]).max()) < TOL
    assert float(np.abs(f32_gallery.cpu().numpy() - g["logits"]).max()) < TOL
    assert torch.equal(f32_mixed, f32_direct)
    assert float((got_mixed - f32_mixed).abs().max()) <= TOL


def test_xcorr_baseline_gallery_equals_the_pairwise_entry():
    from pcr_amd import engine
    m = model_of("xcorr-baseline")
    s1, s2 = T.synthetic_pairs(4, 128, 1, "randn")
    with torch.no_grad():
        xyz1, xyz2, h1, h2 = m.siamese_forward(s1.cuda(), s2.cuda())
    h, xyz = torch.cat([h1, h2]).contiguous(), torch.cat([xyz1, xyz2]).contiguous()
    mixed = torch.tensor(MIXED, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        got = m.match_gallery(h, xyz, mixed)
        with engine.precision("f32"):
            f32_gallery = m.match_gallery(h, xyz, mixed)
            f32_direct = gathered(m, h, xyz, mixed)
    print("xcorr-baseline: default vs f32 %.3g" % float((got - f32_gallery).abs().max()))
    assert torch.equal(f32_gallery, f32_direct)
    assert float((got - f32_gallery).abs().max()) <= TOL
    assert not torch.equal(f32_gallery[0], f32_gallery[1])               # logits(0, 4) != logits(4, 0)


@pytest.mark.parametrize("head,chunk", [pytest.param(h, c, id=h if c is None else "%s-chunk%d" % (h, c))
                                        for c in (None, 5) for h in ("concat", "xcorr-baseline", "xcorr")])
def test_count_gates_the_list(head, chunk, monkeypatch):
    m = model_of(head)
    clouds = T.synthetic_clouds(7, 128, seed=21, kind="randn").cuda()
    with torch.no_grad():
        xyz, h = m.forward_inference(clouds)
    xyz, h = xyz.contiguous(), h.contiguous()
    g = torch.Generator().manual_seed(4)
    live = torch.randint(0, 6, (7, 2), generator=g, dtype=torch.int32)           # the live pairs never name object 6 ...
    pad = torch.full((13, 2), 6, dtype=torch.int32)                              # ... which the padding does
    pairs = torch.cat([live, pad]).cuda()
    count = torch.tensor([7], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        full = m.match_gallery(h, xyz, pairs)
        if chunk is not None:        # four passes over the 20 slots: the count falls inside the second, two are wholly dead
            monkeypatch.setattr(type(m), "GALLERY_CHUNK", chunk)
        gated = m.match_gallery(h, xyz, pairs, count=count, dead_value=-3.25)
        # the padded object's features poisoned: NaN where the gate reads nothing of a dead pair; for 'xcorr', whose
        # local stages run on every pair, other finite features (its dead logits are replaced, not skipped)
        h2 = h.clone()
        h2[6] = (h[6] * 100.0 + 5.0) if head == "xcorr" else float("nan")
        poisoned = m.match_gallery(h2, xyz, pairs, count=count, dead_value=-3.25)
    assert torch.equal(gated[:7], full[:7])
    assert bool((gated[7:] == -3.25).all())
    assert torch.equal(poisoned, gated)
    from pcr_amd._lib import PcrError
    with pytest.raises(PcrError):
        m.match_gallery(h, xyz, pairs, count=torch.tensor([7], device="cuda"))   # int64


def test_concat_retrieve_and_associate_end_to_end():
    m = model_of("concat")
    Q, G = 6, 9
    clouds = T.synthetic_clouds(Q + G, 128, seed=33, kind="randn").cuda()
    with torch.no_grad():
        xyz, h = m.forward_inference(clouds)
    xyz, h = xyz.contiguous(), h.contiguous()
    q_labels = torch.tensor([0, 1, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
    g_labels = torch.tensor([0, 0, 1, 1, 0, 1, 0, 1, 1], dtype=torch.int32, device="cuda")
    q_ids = torch.tensor([3, 4, 5, 6, 4, 3], dtype=torch.int32, device="cuda")
    g_ids = torch.tensor([3, 5, 4, 6, 3, 4, 9, 9, 6], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        out = m.retrieve(h[:Q], xyz[:Q], q_labels, None, h[Q:], xyz[Q:], g_labels, None, query_ids=q_ids, gallery_ids=g_ids,
                         topk=4, num_classes=2)
        c = int(out["count"])
        pairs = out["pairs"]
        want_logits = m.match_gallery(h, xyz, torch.stack([pairs[:, 0], pairs[:, 1] + Q], dim=1))
    assert c == 3 * 4 + 3 * 5
    assert torch.equal(out["logits"], want_logits)
    scores = rank_ref.score_matrix(want_logits.cpu().numpy(), pairs.cpu().numpy(), c, Q, G)
    assert np.array_equal(rank_ref.bits(out["scores"].cpu().numpy()), rank_ref.bits(scores))
    want = rank_ref.rank_gallery(scores, q_ids.cpu().numpy(), g_ids.cpu().numpy(), 4)
    for k, v in want.items():
        assert np.array_equal(rank_ref.bits(out[k].cpu().numpy()), rank_ref.bits(v)), k
    # the tracker's association over the same head: scoring the live pairs only decides the same
    # (a miss / a birth costs 50: dearer than any pair, so that the assignment has matches to decide)
    cost = dict(track_miss=torch.full((Q,), 50.0, device="cuda"), det_new=torch.full((G,), 50.0, device="cuda"))
    with torch.no_grad():
        a = m.associate(h[:Q], xyz[:Q], q_labels, None, h[Q:], xyz[Q:], g_labels, None, num_classes=2, live_only=False,
                        **cost)
        b = m.associate(h[:Q], xyz[:Q], q_labels, None, h[Q:], xyz[Q:], g_labels, None, num_classes=2, live_only=True,
                        **cost)
    assert int(a["info"]) == 0 and int(b["info"]) == 0
    assert torch.equal(a["track_to_det"], b["track_to_det"]) and torch.equal(a["det_to_track"], b["det_to_track"])
    assert bool((a["track_to_det"] >= 0).any())
