#!/usr/bin/env python3
"""Times one frame's association behind the matching logits -- the cost matrix, the assignment and the decode -- with the
assignment solved as ONE problem (linear_assignment, the existing route and the yardstick) and class by class, one wave per
class (association_blocks + linear_assignment_blocks, what by_class=True runs), on the same inputs in one process:

  (dd, td) = (1, 1), (2, 0), (2, 1) with the margin kind and (2, 0) with the softmax kind; <name>_full / <name>_blocks
  scenes   tools/bench_decisions.py's two -- capacity 40 with 30 detections and 200 with 100, 3 classes, every slot active
           (tests/decisions_ref.py's generator) -- and a sparse one at 200 / 100: 8 classes, about half of the slots free and
           a third of the detections padding (label -1: they share the rest block)

Each one eager (E) and replayed from a captured graph (G).  ms per frame from device events around windows of >= --window
seconds; all series alternate in one process, --repeats windows each; min, median and max of the windows are reported.
Before timing, every decoded output of the two routes is compared and must be equal.  The block ids are made from the labels
inside the timed step, as a tracker frame makes them.  What it does NOT measure: the match that produces the logits.
Fails without a GPU.

    python tools/bench_assign_blocks.py [--out profiles/<record>.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NUM_CLASSES = 8                   # the model's default: G = 9 blocks, the classes a scene does not use stay empty
CONFIGS = ((1, 1, "margin"), (2, 0, "margin"), (2, 1, "margin"), (2, 0, "softmax"))


def dense_scene(T, D):
    """bench_decisions.py's scene: 3 classes, every object labelled -> (name, labels, logits, pairs, count)"""
    import assoc_ref
    import decisions_ref as R
    logits, pairs, count, _, _ = R.random_case(T, D, 0, 0, seed=[T, D])
    g = np.random.default_rng([T, D])                     # the generator's first two draws are the labels
    tl, dl = g.integers(0, 3, T), g.integers(0, 3, D)
    assert np.array_equal(assoc_ref.compare_pairs(tl, dl, num_classes=3)[0], pairs)
    return "dense", tl, dl, logits, pairs, count


def sparse_scene(T, D):
    """8 classes, about half of the slots free and a third of the detections padding"""
    import assoc_ref
    g = np.random.default_rng([T, D, 8])
    tl, dl = g.integers(0, 8, T), g.integers(0, 8, D)
    tl[g.random(T) < 0.5] = -1
    dl[D - D // 3:] = -1                                  # padding follows the frame's detections
    pairs, count = assoc_ref.compare_pairs(tl, dl, num_classes=8)
    return "sparse", tl, dl, (g.standard_normal(len(pairs)) * 4.0).astype(np.float32), pairs, count


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assign_blocks: no GPU (this tool measures on the device only)")
    from pcr_amd import associate as A
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda t: t.detach().cpu().numpy()
    rows = []
    for T, D, scene in ((40, 30, dense_scene), (200, 100, dense_scene), (200, 100, sparse_scene)):
        name, tl, dl, logits, pairs, count = scene(T, D)
        g = np.random.default_rng([D, T])
        det, trk = g.standard_normal((2, D)).astype(np.float32), g.standard_normal((1, T)).astype(np.float32)
        d_logits, d_pairs, d_count, d_det, d_trk = dev(logits), dev(pairs), dev(np.array([count], np.int32)), dev(det), dev(trk)
        d_tl, d_dl = dev(tl.astype(np.int32)), dev(dl.astype(np.int32))
        series = {}

        def make(dd, td, kind, by_class):
            dv, tv = (d_det[:dd].contiguous() if dd else None), (d_trk[:td].contiguous() if td else None)

            def step():
                cost = A.association_cost_multi(d_logits, d_pairs, d_count, T, D, dv, tv, kind=kind)
                if by_class:
                    row_block, col_block, G = A.association_blocks(d_tl, d_dl, T, D, dd, td, num_classes=NUM_CLASSES)
                    col4row, row4col, block_info = A.linear_assignment_blocks(cost, row_block, col_block, G)
                    assignment = (col4row, row4col, block_info.amax(dim=0, keepdim=True))
                else:
                    assignment = A.linear_assignment(cost)
                return A.decode_assignment(cost, assignment, T, D, dd, td, born_decision=dd - 1, kill_decision=td - 1)
            return step

        for dd, td, kind in CONFIGS:
            key = "%d_%d_%s" % (dd, td, kind)
            full, blocks = make(dd, td, kind, False), make(dd, td, kind, True)
            series[key + "_full"], series[key + "_blocks"] = full, blocks
            a, b = full(), blocks()                       # (the warm-up, and the check of one route against the other)
            for k in a:
                assert np.array_equal(host(a[k]), host(b[k])), "%s %s: %s differs between the two routes" % (name, key, k)
        torch.cuda.synchronize()
        graphs = {}
        for key, fn in series.items():
            graphs[key] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[key]):
                fn()
        times = {(key, mode): [] for key in series for mode in "EG"}
        for _ in range(args.repeats):
            for key, fn in series.items():
                times[(key, "E")].append(window(fn, args.window))
                times[(key, "G")].append(window(graphs[key].replay, args.window))
        row = {"scene": name, "capacity": T, "detections": D, "listed_pairs": int(count),
               "active_slots": int((tl >= 0).sum()), "real_detections": int((dl >= 0).sum())}
        for (key, mode), t in times.items():
            row["%s_%s_ms" % (key, mode)] = {"min": round(min(t), 4), "median": round(float(np.median(t)), 4),
                                             "max": round(max(t), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_assign_blocks.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "num_classes": NUM_CLASSES,
           "note": "<dd>_<td>_<kind>_full = association_cost_multi + linear_assignment + decode_assignment for one frame (the "
                   "existing route, the yardstick); _blocks = the same with association_blocks + linear_assignment_blocks + "
                   "the maximum over the blocks' info in place of linear_assignment (by_class=True).  _E_ eager, _G_ replayed "
                   "from a captured graph.  ms per frame (device events), min / median / max of the repeated windows, all "
                   "series alternating in one process; the decoded outputs of the two routes were compared equal before "
                   "timing.  The match that produces the logits is not part of any series",
           "shapes": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
