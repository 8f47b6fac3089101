#!/usr/bin/env python3
"""Writes tests/golden/train_step_aux_n128.npz and pt_aux_manifest.json: the reference's own train_step
(mmdet3d/models/ReIDNet.py:586-634) with the match, cls, fp, kl and triplet losses on, and its forward_test in eval mode.

Model: the point-cat Point-Transformer (configs_reid/_base_/reidentifiers/reid_pts_point-transformer_point-cat.py) with the
two heads its commented config lines give -- LinearRes(128, 128, 'GN', ng=16) + Linear(128, 20) for cls, + Linear(128, 1)
for fp -- triplet_sample_num = 4, backbone_list [128, 64, 32], seeded weights (pcr_amd.testing).  Input: 8 pairs of 128
points, the first half matching, labels spread over 0..19 (some above 9: false positives).

The reference is imported through oracle/ref_loader.build_ref_reidnet; nothing of its text is written anywhere.
`torch.multinomial` is wrapped for the duration of a step: the first (float32) step records what the reference drew, the
float64 step is handed the same draws.  Recorded, as oracle/make_golden.py gen_train_variants records: loss, the logged
values, a spread of `grad:` tensors with their float64 twins `grad64:`, `no_grad_params`, the gradient norm, running
means; plus `neg` (B, T) int32 (rows of cat(h1, h2); -1 for a non-matching pair), `margin`, and the eval-mode
`val_cls_preds` / `val_fp_preds` / `val_match_preds` and val losses.

Margin: the float64 midpoint of the two central values of d_an - d_ap over the drawn triplets (their median), so that
active and inactive triplets both occur.  The tool refuses to write unless, in float64,
  * the margin is positive (torch's TripletMarginLoss takes no other),
  * every triplet's |d_ap - d_an + margin| is at least 1e-3 of the largest distance, and
  * every row's top-two cls logit gap exceeds 1e-3 (training mode and eval mode),
and tries the next input seed when they fail.

    PCR_REFERENCE_ROOT=/path/to/reference python tools/make_aux_golden.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import aux_ref  # noqa: E402
import make_golden as MG  # noqa: E402
import ref_loader  # noqa: E402
from pcr_amd import testing as T  # noqa: E402

PAIRS, N, TRIPLETS, CLASSES = 8, 128, 4, 20
LOSSES = dict(kl=True, match=True, cls=True, shape=False, fp=True, dense=False, triplet=True)


def head(n_out):
    return [dict(type="LinearRes", n_in=128, n_out=128, norm="GN", ng=16),
            dict(type="Linear", in_features=128, out_features=n_out)]


def build(dtype):
    model, manifest = MG.build(MG.PT_CFG, seed=0, losses_to_use=dict(LOSSES), cls_head=head(CLASSES), fp_head=head(1),
                               triplet_sample_num=TRIPLETS, backbone_list=[128, 64, 32])
    return model.to(dtype), manifest


def train_data(seed, dtype=torch.float32):
    s1, s2 = T.synthetic_pairs(PAIRS, N, seed=seed, kind="randn")
    s1, s2 = s1.to(dtype), s2.to(dtype)
    ids1 = torch.arange(PAIRS)
    ids2 = torch.where(torch.arange(PAIRS) < PAIRS // 2, ids1, ids1 + 100)
    lab1 = (torch.arange(PAIRS) * 5 + 3) % CLASSES                      # 3, 8, 13, 18, 3, ...: both sides of 9
    lab2 = torch.where(torch.arange(PAIRS) < PAIRS // 2, lab1, (lab1 + 7) % CLASSES)
    return dict(sparse_1=list(s1), sparse_2=list(s2), dense_1=list(s1), dense_2=list(s2),
                label_1=[v.view(1) for v in lab1], label_2=[v.view(1) for v in lab2],
                id_1=[i.view(1) for i in ids1], id_2=[i.view(1) for i in ids2])


class Draws:
    """torch.multinomial for the duration of a step: records every call's result, or replays a recorded list"""

    def __init__(self, replay=None):
        self.calls, self.replay = [], None if replay is None else list(replay)

    def __enter__(self):
        self.orig = torch.multinomial

        def spy(*a, **k):
            out = self.orig(*a, **k) if self.replay is None else self.replay[len(self.calls)].clone()
            self.calls.append(out.clone())
            return out
        torch.multinomial = spy
        return self

    def __exit__(self, *exc):
        torch.multinomial = self.orig
        return False


def negatives(data, draws):
    """the rows of cat(h1, h2) the reference gathered (ReIDNet.py:551-555): pool[draw] per matching pair"""
    ids = torch.cat(data["id_1"] + data["id_2"])
    neg = np.full((PAIRS, TRIPLETS), -1, np.int32)
    matching = [i for i in range(PAIRS) if int(ids[i]) == int(ids[PAIRS + i])]
    assert len(matching) == len(draws)
    for i, d in zip(matching, draws):
        pool = torch.where(ids != ids[i])[0]
        neg[i] = pool[d].numpy()
    return neg, ids.numpy()


def step(model, data, draws=None):
    seen = {}
    orig = model.cls_forward

    def cls_spy(*a, **k):
        preds, loss = orig(*a, **k)
        seen["cls"] = preds.detach().clone()
        return preds, loss
    model.cls_forward = cls_spy
    with Draws(draws) as d, contextlib.redirect_stdout(io.StringIO()):
        out = model.train_step(data, None)
    model.cls_forward = orig
    out["loss"].backward()
    return out, d.calls, seen["cls"]


def top_two_gap(logits):
    top = logits.double().topk(2, dim=1)[0]
    return float((top[:, 0] - top[:, 1]).min())


def attempt(seed):
    data = train_data(seed)
    data64 = train_data(seed, torch.float64)
    # the margin: the float64 encodings under the draws of a probe step (the draws do not depend on the margin)
    probe, _ = build(torch.float64)
    probe.train()
    torch.manual_seed(seed)
    with Draws() as d, contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        s1, s2 = torch.stack(data64["sparse_1"]), torch.stack(data64["sparse_2"])
        _, _, h1, h2 = probe.siamese_forward(s1, s2)
        ids1, ids2 = torch.cat(data64["id_1"]), torch.cat(data64["id_2"])
        probe.get_triplet_loss(h1, h2, ids1, ids2, (ids1 == ids2).float(), None, s1.device)
    neg, ids = negatives(data, d.calls)
    draws = d.calls
    h = torch.cat([h1, h2]).reshape(2 * PAIRS, -1)
    match = (ids[:PAIRS] == ids[PAIRS:]).astype(np.int32)
    margin = aux_ref.median_margin(h, neg, match)
    gap, dmax = aux_ref.hinge_gaps(h, neg, match, margin)
    if not (margin > 0 and gap >= 1e-3 * dmax):
        return None, "margin %.4g, hinge gap %.3g of %.3g" % (margin, gap, dmax)

    model, manifest = build(torch.float32)
    model.triplet_loss = nn.TripletMarginLoss(margin=margin, p=2)
    model.train()
    out, calls, cls_train = step(model, data, draws)
    assert all(torch.equal(a, b) for a, b in zip(calls, draws))
    model64, _ = build(torch.float64)
    model64.triplet_loss = nn.TripletMarginLoss(margin=margin, p=2)
    model64.train()
    out64, _, cls_train64 = step(model64, data64, draws)

    # forward_test in eval mode (after the step: the running statistics moved, as they would in training)
    model.eval()
    one = lambda v: [torch.full((1,), v, dtype=torch.long)] * PAIRS          # noqa: E731
    test = dict(data, size_1=one(N), size_2=one(N), vis_1=one(1), vis_2=one(1))
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        res = model(return_loss=False, **test)[0]
    gaps = (top_two_gap(cls_train64), top_two_gap(cls_train), top_two_gap(res["val_cls_preds"]))
    if min(gaps) <= 1e-3:
        return None, "cls top-two gaps %s" % (gaps,)

    params = dict(model.named_parameters())
    p64 = dict(model64.named_parameters())
    lv = out["log_vars"]
    rec = dict(loss=np.float32(out["loss"].item()), loss64=np.float64(out64["loss"].item()), margin=np.float64(margin),
               neg=neg, ids=ids.astype(np.int64))
    for k in ("match_loss", "match_acc", "cls_loss", "cls_acc", "fp_loss", "fp_acc", "kl_loss", "triplet_loss"):
        rec[k] = np.float32(lv[k])
        rec[k + "64"] = np.float64(out64["log_vars"][k])
    with_grad = [k for k, p in params.items() if p.grad is not None]
    pick = sorted(set(with_grad[:3] + with_grad[-3:] + with_grad[::10] +
                      [k for k in with_grad if k.startswith(("cls_head", "fp_head"))]))
    for k in pick:
        if params[k].grad.numel() <= 40000:
            rec["grad:" + k] = MG._np(params[k].grad)
            rec["grad64:" + k] = p64[k].grad.numpy().astype(np.float32)          # (the exact value rounded once)
    rec["no_grad_params"] = np.array(json.dumps([k for k, p in params.items() if p.grad is None]))
    rec["grad_norm"] = np.float32(float(torch.sqrt(sum((params[k].grad.double() ** 2).sum() for k in with_grad))))
    bn = [(k, b) for k, b in model.named_buffers() if k.endswith("running_mean")]
    for k, b in bn[:2] + bn[-1:]:
        rec["buf:" + k] = MG._np(b)
    for k in ("val_cls_preds", "val_fp_preds", "val_match_preds"):
        rec[k] = MG._np(res[k]).astype(np.float32)
    for k in ("val_cls_loss", "val_fp_loss", "val_kl_loss", "val_match_loss"):
        rec[k] = np.float32(float(res[k]))
    rec["meta"] = np.array(json.dumps(dict(pairs=PAIRS, n=N, input_seed=seed, weight_seed=0, triplet_sample_num=TRIPLETS,
                                           classes=CLASSES, cfg=MG.PT_CFG, hinge_gap=gap, max_dist=dmax,
                                           cls_gaps=list(gaps))))
    return (rec, manifest), None


def main():
    ref = ref_loader.load_reference()
    ref.attention.torch = MG._CpuTorch()
    for seed in range(2, 40):
        got, why = attempt(seed)
        if got is None:
            print("input seed", seed, "refused:", why)
            continue
        rec, manifest = got
        np.savez_compressed(os.path.join(MG.GOLD, "train_step_aux_n%d.npz" % N), **rec)
        with open(os.path.join(MG.GOLD, "pt_aux_manifest.json"), "w") as f:
            json.dump(manifest, f)
        print("input seed", seed, "loss", rec["loss"], "loss64", rec["loss64"], "margin", rec["margin"],
              {k: float(rec[k]) for k in ("match_loss", "cls_loss", "fp_loss", "kl_loss", "triplet_loss", "cls_acc", "fp_acc")},
              "grads recorded", sum(1 for k in rec if k.startswith("grad:")))
        print("neg", rec["neg"].tolist())
        return 0
    print("no input seed in 2..39 meets the conditions")
    return 1


if __name__ == "__main__":
    sys.exit(main())
