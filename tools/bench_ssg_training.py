#!/usr/bin/env python3
"""Times a Trainer step (forward + backward + the HIP AdamW update) of the PointNet++ SSG ReIDNet in training mode at
BASELINE config 2's shape: 1024-point box clouds, SA(512, 0.2, 32, [64, 64, 128]) -> SA(128, 0.4, 64, [128, 128, 256]) ->
Conv1d 64, 256 pairs per GPU (the reference's samples_per_gpu), eager and with Trainer(graph=True).

The yardstick is a torch-on-device restatement of the same step in the same process, alternated with it: the encoder as
gather + conv2d + BatchNorm2d + max over the (B,C,S,K) tensor (sampling and ball query by the same device ops, cov_final
as nn.Conv1d), the matching through the existing training graph, the same Trainer.  (The parent of this feature cannot
run the step at all, so it cannot be the yardstick.)

Recorded besides: the per-launch table of one eager HIP step (the engine's profiling hooks: name, launches, ms, share) and
the saved-activation bytes of the two encoders, computed from the shapes.

Host clock around windows of >= --window seconds that end in a device synchronise, --repeats windows each after a warm-up
that includes the graph capture.  Fails without a GPU.

    python tools/bench_ssg_training.py [--out profiles/ssg_training_bench.json] [--pairs 256]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N = 1024
LOSSES = dict(kl=False, match=True, cls=False, shape=False, fp=False, dense=False, triplet=False)


class TorchSSG(torch.nn.Module):
    """PointNet2SSG.forward in training mode, restated with torch ops on the grouped (B,C,S,K) tensor; same sub-module
    names, so a state dict fits both"""

    def __init__(self, ssg):
        super().__init__()
        self.SA_modules, self.cov_final = ssg.SA_modules, ssg.cov_final

    def forward(self, pointcloud, numpoints=None):
        from mmdet3d import ops
        xyz, feats = pointcloud[..., 0:3].detach().contiguous(), None
        for sa in self.SA_modules:
            g = sa.groupers[0]
            with torch.no_grad():
                centre = ops.furthest_point_sample(xyz, sa.num_point[0]).long()
                new_xyz = torch.gather(xyz, 1, centre.unsqueeze(2).expand(-1, -1, 3)).contiguous()
                idx = ops.ball_query(0.0, g.max_radius, g.sample_num, xyz, new_xyz).long()
            B, S, K = idx.shape
            flat = idx.reshape(B, 1, S * K)
            h = torch.gather(xyz.transpose(1, 2), 2, flat.expand(-1, 3, -1)).view(B, 3, S, K) - new_xyz.transpose(1, 2).unsqueeze(3)
            if feats is not None:
                h = torch.cat([h, torch.gather(feats, 2, flat.expand(-1, feats.shape[1], -1)).view(B, -1, S, K)], dim=1)
            for layer in sa.mlps[0].children():
                h = F.relu(layer.bn(layer.conv(h)))
            xyz, feats = new_xyz, h.max(dim=3)[0]
        return xyz, self.cov_final(feats)


def build(torch_encoder):
    import bench
    from mmdet3d.models import build_model
    from pcr_amd import testing as T
    cfg = copy.deepcopy(bench.SSG_MODEL)
    cfg["backbone"]["trainable"] = True
    cfg["losses_to_use"] = dict(LOSSES)
    m = build_model(cfg)
    m.load_state_dict(T.seeded_state_dict(T.manifest_of(m), 0), strict=True)
    if torch_encoder:
        m.backbone = TorchSSG(m.backbone)
    return m.cuda().train()


def batch(pairs):
    from pcr_amd import testing as T
    s1, s2 = T.synthetic_pairs(pairs, N, seed=1234, kind="box")
    s1, s2 = s1.cuda(), s2.cuda()
    ids1 = torch.arange(pairs)
    ids2 = torch.where(torch.arange(pairs) % 2 == 0, ids1, ids1 + 10 ** 6)
    zero = torch.zeros(1, dtype=torch.long, device="cuda")
    return dict(sparse_1=list(s1), sparse_2=list(s2), dense_1=list(s1), dense_2=list(s2), label_1=[zero] * pairs,
                label_2=[zero] * pairs, id_1=[i.view(1).cuda() for i in ids1], id_2=[i.view(1).cuda() for i in ids2])


def window(fn, seconds):
    """ms per call over a window of at least `seconds` that ends in a synchronise (the call count comes from a pilot)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(3, int(np.ceil(seconds / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def saved_bytes(model, clouds):
    """saved-activation bytes of the two encoders for `clouds` clouds, from the shapes: HIP = what SaGroupTrain keeps (the
    three raw layer outputs, pooled / argmax / winning raw value, the cloud, the index list, the centre indices; the point
    features its table layer keeps are the previous scale's pooled output, counted there); torch = the grouped input, every
    conv output (kept by BatchNorm) and every ReLU output (kept by F.relu and by the next conv; BatchNorm's own output is
    not kept), the max's int64 indices and the gather's int64 index list"""
    hip = tor = 0
    n, d = N, 0
    for sa in model.backbone.SA_modules:
        S, K = sa.num_point[0], sa.groupers[0].sample_num
        cs = [l.conv.weight.shape[0] for l in sa.mlps[0].children()]
        rows = clouds * S * K
        hip += 4 * rows * sum(cs) + 12 * clouds * cs[2] * S + 4 * rows + 4 * clouds * (3 * n + S)
        tor += 4 * rows * (3 + d) + 4 * rows * 2 * sum(cs) + 8 * clouds * cs[2] * S + 8 * rows
        n, d = S, cs[2]
    return dict(hip=hip, torch=tor)


def launch_table(tr, data):
    """one eager HIP step under the engine's profiling hooks: [name, launches, ms, share] by descending time, and the share
    of the step's device time the hooks cover"""
    from pcr_amd import engine
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    engine.PROFILE = []
    try:
        e0.record()
        tr.step(data)
        e1.record()
        torch.cuda.synchronize()
        agg = {}
        for name, a, b, *_ in engine.PROFILE:
            n, ms = agg.get(name, (0, 0.0))
            agg[name] = (n + 1, ms + a.elapsed_time(b))
    finally:
        engine.PROFILE = None
    total = e0.elapsed_time(e1)
    rows = sorted(([k, n, round(ms, 3), round(ms / total, 4)] for k, (n, ms) in agg.items()), key=lambda r: -r[2])
    return dict(step_ms=round(total, 3), hooked_share=round(sum(r[2] for r in rows) / total, 4), launches=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssg_training_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssg_training: no GPU (this tool measures on the device only)")
    from pcr_amd import train
    data = batch(args.pairs)
    sides, trainers = {}, {}
    for graph in (False, True):
        for name, torch_encoder in (("hip", False), ("torch", True)):
            tr = train.Trainer(build(torch_encoder), max_iters=10 ** 6, lr=1e-5, grad_clip=1.0, graph=graph)
            for _ in range(tr.graph_warmup + 2):                  # eager warm-up, the capture, one replay
                tr.step(data)
            assert tr.graph == graph, "graph capture fell back"
            key = "%s_%s" % (name, "graph" if graph else "eager")
            sides[key] = (lambda tr=tr: tr.step(data))
            trainers[key] = tr
    times, peak = {k: [] for k in sides}, {}
    for _ in range(args.repeats):
        for k, f in sides.items():
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            times[k].append(window(f, args.window))
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated() - base)
    ms = {k: {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3),
              "peak_mib_above_resident": round(peak[k] / 2.0 ** 20, 1)} for k, t in times.items()}
    rec = {"tool": "tools/bench_ssg_training.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "points": N, "pairs": args.pairs,
           "model": "SA(512, 0.2, 32, [64, 64, 128]) -> SA(128, 0.4, 64, [128, 128, 256]) -> Conv1d 64, match head of bench.SSG_MODEL",
           "note": "ms per Trainer step (forward + backward + AdamW), median / min / max of the repeated windows, the sides "
                   "alternating in one process.  hip = PointNet2SSG(trainable=True); torch = the same step with the encoder "
                   "restated as gather + conv2d + BatchNorm2d + max (the yardstick); both match through the HIP training "
                   "graph.  peak_mib_above_resident: allocator high-water mark above what was resident before the window "
                   "(graph mode: the captured pool is resident, read the eager rows)",
           "ms": ms, "pairs_per_s": {k: round(args.pairs / (v["median"] * 1e-3), 1) for k, v in ms.items()},
           "hip_over_torch": {g: round(ms["hip_" + g]["median"] / ms["torch_" + g]["median"], 3) for g in ("eager", "graph")},
           "saved_activation_bytes": saved_bytes(trainers["hip_eager"].model, 2 * args.pairs),
           "launch_table": launch_table(trainers["hip_eager"], data)}
    print(json.dumps({k: rec[k] for k in ("ms", "pairs_per_s", "hip_over_torch", "saved_activation_bytes")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
