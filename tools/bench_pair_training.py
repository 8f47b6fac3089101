#!/usr/bin/env python3
"""Times a Trainer step (forward + backward + the HIP AdamW update) of the point-cat Point-Transformer at N = 128 points
for b in {16, 64}, four ways, eager and with Trainer(graph=True):

  a  the paired step: b pairs, 2b clouds encoded
  b  b^2 explicit pairs through the ordinary train_step: 2 b^2 clouds encoded -- the only route to the cartesian
     supervision before `sampling = 'cartesian'`, and the yardstick
  c  sampling = 'cartesian': 2b clouds encoded once, the b^2 slots matched through train_graph.match_logits_list with
     stage 1 once per object (train_ops.LinAttnPairs)
  d  as c with the amortised stage 1 switched off (train_graph.PAIR_AMORTISED = False): every slot's operands gathered,
     stage 1 per slot.  c against d is the share of the indexed attention core.

Host clock around windows of >= --window seconds that end in a device synchronise, --repeats windows each after a warm-up
that includes the graph capture, the sides alternating in one process.  Peak device memory of a step (allocator high-water
mark over the timed windows) is reported per live pair.  Fails without a GPU.

    python tools/bench_pair_training.py [--out profiles/<record>.json]      (default: profiles/pair_training_bench.json)
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N = 128
LOSSES = dict(kl=False, match=True, cls=False, shape=False, fp=False, dense=False, triplet=False)


def build(sampling):
    import bench
    from mmdet3d.models import build_model
    from pcr_amd import testing as T
    cfg = copy.deepcopy(bench.PT_MODEL)
    cfg.update(losses_to_use=dict(LOSSES), sampling=sampling)
    m = build_model(cfg)
    m.load_state_dict(T.seeded_state_dict(T.load_manifest(os.path.join(ROOT, "tests", "golden", "pt_manifest.json")), 0),
                      strict=True)
    return m.cuda().train()


def batch(b, expand):
    """b pairs, a quarter of them matching; expand: the b^2 explicit pairs in cartesian order"""
    from pcr_amd import testing as T
    s1, s2 = T.synthetic_pairs(b, N, seed=2, kind="randn")
    ids1 = torch.arange(b)
    ids2 = torch.where(torch.arange(b) % 4 == 0, ids1, ids1 + 1000)
    if expand:
        cp = torch.cartesian_prod(torch.arange(b), torch.arange(b))
        s1, s2, ids1, ids2 = s1[cp[:, 0]], s2[cp[:, 1]], ids1[cp[:, 0]], ids2[cp[:, 1]]
    s1, s2 = s1.cuda(), s2.cuda()
    zero = torch.zeros(1, dtype=torch.long, device="cuda")
    n = s1.shape[0]
    return dict(sparse_1=list(s1), sparse_2=list(s2), dense_1=list(s1), dense_2=list(s2), label_1=[zero] * n,
                label_2=[zero] * n, id_1=[i.view(1).cuda() for i in ids1], id_2=[i.view(1).cuda() for i in ids2])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_training_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_training: no GPU (this tool measures on the device only)")
    from pcr_amd import train, train_graph
    rows = {}
    for b in args.batches:
        sides = {}
        for graph in (False, True):
            for name, sampling, expand, amortised in (("a_paired", None, False, True), ("b_explicit", None, True, True),
                                                      ("c_cartesian", "cartesian", False, True),
                                                      ("d_gathered", "cartesian", False, False)):
                tr = train.Trainer(build(sampling), max_iters=10 ** 6, lr=1e-5, grad_clip=1.0, graph=graph)
                data = batch(b, expand)

                def run(tr=tr, data=data, amortised=amortised):
                    train_graph.PAIR_AMORTISED = amortised        # (read while the step is built or captured)
                    tr.step(data)
                for _ in range(tr.graph_warmup + 2):              # eager warm-up, the capture, one replay
                    run()
                assert tr.graph == graph, "graph capture fell back"
                live = b if name == "a_paired" else b * b
                sides["%s_%s" % (name, "graph" if graph else "eager")] = (run, live)
        times, peak = {k: [] for k in sides}, {}
        for _ in range(args.repeats):
            for k, (f, live) in sides.items():
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                times[k].append(window(f, args.window))
                peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated() - base)
        train_graph.PAIR_AMORTISED = True
        rows["b=%d" % b] = {k: {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                "live_pairs": sides[k][1], "peak_kib_per_live_pair": round(peak[k] / 1024.0 / sides[k][1], 1)}
                            for k, t in times.items()}
        print(json.dumps({"b=%d" % b: rows["b=%d" % b]}), flush=True)
        del sides
        torch.cuda.empty_cache()
    rec = {"tool": "tools/bench_pair_training.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "points": N,
           "note": "ms per Trainer step (forward + backward + AdamW), median / min / max of the repeated windows, the sides "
                   "alternating in one process; a = b pairs, b = b^2 explicit pairs (2 b^2 clouds encoded; the yardstick), "
                   "c = sampling 'cartesian' (2b clouds encoded, b^2 slots, stage 1 once per object), d = c with every "
                   "slot's stage-1 operands gathered.  peak_kib_per_live_pair: the allocator's high-water mark above what "
                   "was resident before the window (graph mode: the captured pool is resident, so the figure is the "
                   "eager rows')",
           "ms": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
