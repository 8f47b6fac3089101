#!/usr/bin/env python3
"""Times a training step (forward + backward of ReIDNet.train_step, no optimizer) of the point-cat Point-Transformer at the
training configs' shape -- 256 pairs of 128 points, triplet_sample_num = 128, margin 10 -- three ways:

  M  match only (every ReID config's setting so far)
  A  match + cls + fp + kl + triplet through the HIP launches (train_graph.aux_losses: the two heads through the dense and
     token-norm launches, pcr_kl_pairs, pcr_triplet_draw + pcr_pair_dist + pcr_triplet_select + pcr_pair_dist_bwd)
  R  match through the same HIP graph + a torch restatement of the same four losses ON THE DEVICE, as the reference writes
     them (ReIDNet.py:348-384, 467-482, 538-582): nn.KLDivLoss over two log-softmaxes, torch.multinomial on the host
     generator per matching pair, anchor / positive / negative gathered as three (n_match T, 64 N) tensors for
     nn.TripletMarginLoss, the heads as torch modules on the pooled features.  R is the yardstick: A - M against R - M is
     what the launches cost against what the restatement costs.

Device events around windows of >= --window seconds after a warm-up, --repeats windows each, the three alternating in one
process; eager, and A and M replayed from a captured graph (R reads the host generator in every step and cannot be
captured).  Fails without a GPU.

    python tools/bench_aux_losses.py [--out profiles/<record>.json]      (default: profiles/aux_losses_bench.json)
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

PAIRS, N, TRIPLETS, MARGIN, CLASSES = 256, 128, 128, 10.0, 20
ON = dict(kl=True, match=True, cls=True, shape=False, fp=True, dense=False, triplet=True)
OFF = dict(kl=False, match=True, cls=False, shape=False, fp=False, dense=False, triplet=False)


def window(fn, seconds):
    """ms per call over a window of at least `seconds` (device events; the call count is fixed from a pilot)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    calls = max(3, int(np.ceil(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def head(n_out):
    return [dict(type="LinearRes", n_in=128, n_out=128, norm="GN", ng=16),
            dict(type="Linear", in_features=128, out_features=n_out)]


def build(losses):
    import bench
    from mmdet3d.models import build_model
    from pcr_amd import testing as T
    cfg = copy.deepcopy(bench.PT_MODEL)
    cfg.update(cls_head=head(CLASSES), fp_head=head(1), triplet_sample_num=TRIPLETS,
               triplet_loss=dict(margin=MARGIN, p=2), losses_to_use=dict(losses))
    m = build_model(cfg)
    m.load_state_dict(T.seeded_state_dict(T.load_manifest(os.path.join(ROOT, "tests", "golden", "pt_aux_manifest.json")), 0),
                      strict=True)
    return m.cuda().train()


def batch():
    from pcr_amd import testing as T
    s1, s2 = T.synthetic_pairs(PAIRS, N, seed=2, kind="randn")
    ids1 = torch.arange(PAIRS)
    ids2 = torch.where(torch.arange(PAIRS) % 2 == 0, ids1, ids1 + 1000)          # half of the pairs match
    lab1 = (torch.arange(PAIRS) * 7 + 3) % CLASSES
    lab2 = torch.where(torch.arange(PAIRS) % 2 == 0, lab1, (lab1 + 7) % CLASSES)
    s1, s2 = s1.cuda(), s2.cuda()
    return dict(sparse_1=list(s1), sparse_2=list(s2), dense_1=list(s1), dense_2=list(s2),
                label_1=[v.view(1).cuda() for v in lab1], label_2=[v.view(1).cuda() for v in lab2],
                id_1=[i.view(1).cuda() for i in ids1], id_2=[i.view(1).cuda() for i in ids2])


class TorchAux:
    """the four losses as the reference writes them, on the device, over the HIP graph's encodings"""

    def __init__(self, model):
        self.m = model
        self.kl = nn.KLDivLoss(log_target=True, reduction="none")
        self.lsmx = nn.LogSoftmax(dim=1)
        self.ce = nn.CrossEntropyLoss()
        self.triplet = nn.TripletMarginLoss(margin=MARGIN, p=2)

    @staticmethod
    def head(seq, x):
        """[LinearRes, Linear] in torch ops (lanegcn_nets.py:228-241; the package's LinearRes.forward is a HIP launch
        without a backward)"""
        r = seq[0]
        out = torch.relu(r.norm1(r.linear1(x)))
        out = r.norm2(r.linear2(out))
        short = x if r.transform is None else r.transform[1](r.transform[0](x))
        return seq[1](torch.relu(out + short))

    def __call__(self, h1, h2, labels, id1, id2, match):
        m = self.m
        h_cat = torch.cat([h1, h2], dim=0)
        pooled = torch.cat([h_cat.max(dim=2)[0], h_cat.mean(dim=2)], dim=1)
        cls = self.ce(self.head(m.cls_head, pooled), labels)
        fp = m.bce(self.head(m.fp_head, pooled).squeeze(1), (labels > 9).float())
        kl = self.kl(self.lsmx(h1.reshape(h1.size(0), -1)), self.lsmx(h2.reshape(h2.size(0), -1))).mean(dim=1)
        no = torch.where(match == 0)
        kl[no] = kl[no] * -1
        kl = kl[match == 0].mean() + kl[match == 1].mean()
        idx = torch.where(match == 1)[0]
        ids = torch.cat([id1, id2], dim=0)
        a, n = [], []
        for i in idx:
            pool = torch.where(ids != id1[i])[0]
            pick = torch.multinomial(torch.ones(pool.size(0)), TRIPLETS, replacement=len(pool) < TRIPLETS).to(h1.device)
            a.append(torch.full((TRIPLETS,), int(i), device=h1.device))
            n.append(pool[pick])
        a, n = torch.cat(a), torch.cat(n)
        trip = self.triplet(anchor=h1.reshape(h1.size(0), -1)[a], positive=h2.reshape(h1.size(0), -1)[a],
                            negative=h_cat.reshape(h_cat.size(0), -1)[n])
        return cls + kl + fp + trip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_losses_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_aux_losses: no GPU (this tool measures on the device only)")
    from pcr_amd import train_ops
    data = batch()
    m_off, m_on, m_ref = build(OFF), build(ON), build(OFF)
    ref_aux = TorchAux(m_ref)

    def step(model):
        def run():
            for p in model.parameters():
                p.grad = None
            train_ops.prepack(model)
            model.train_step(data, None)["loss"].backward()
        return run

    def step_ref():
        m = m_ref
        for p in m.parameters():
            p.grad = None
        train_ops.prepack(m)
        s1, s2, _, _, l1, l2, i1, i2 = m.preprocess_inputs(*(data[k] for k in (
            "sparse_1", "sparse_2", "dense_1", "dense_2", "label_1", "label_2", "id_1", "id_2")))
        xyz1, xyz2, h1, h2 = m.siamese_forward(s1, s2)
        match = (i1 == i2).float()
        _, loss, _ = m.match_forward(h1, h2, xyz1, xyz2, match, None, s1.device)
        (loss + ref_aux(h1, h2, torch.cat([l1, l2]), i1, i2, match)).backward()

    sides = {"M_match_only": step(m_off), "A_hip_aux": step(m_on), "R_torch_aux": step_ref}
    for f in sides.values():
        for _ in range(3):
            f()
    graphs = {}
    for name in ("M_match_only", "A_hip_aux"):
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            sides[name]()
            with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
                sides[name]()
        torch.cuda.current_stream().wait_stream(s)
        graphs[name + "_replayed"] = g.replay
    sides.update(graphs)
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, f in sides.items():
            times[k].append(window(f, args.window))
    row = {k: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
           for k, t in times.items()}
    print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_aux_losses.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "pairs": PAIRS, "points": N, "triplet_sample_num": TRIPLETS,
           "note": "forward + backward of one training step, ms per step, median / min / max of the repeated windows, the "
                   "sides alternating in one process.  M = match only; A = match + cls + fp + kl + triplet through the HIP "
                   "launches; R = match + a torch restatement of the same four losses on the device (the yardstick: it "
                   "gathers anchor, positive and negative as (n_match T, 64 N) tensors and draws on the host generator, "
                   "so it cannot be captured).  A - M against R - M is the cost of the four losses either way",
           "ms": row}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
