#!/usr/bin/env python3
"""Times one frame's association behind the matching logits -- the cost matrix, the assignment and the decode -- for several
sets of decisions (pcr_amd/associate.py: association_cost_multi + linear_assignment + decode_assignment), at a capacity of
40 tracks with 30 detections and of 200 with 100 (tests/decisions_ref.py's generator: 3 classes, logits ~ N(0, 4^2) on the
class-gated pairs, N(0, 1) decision values):

  (dd, td) = (1, 1), (2, 0), (2, 1), each with the margin and the softmax kind; (2, 0) also with reduce
  B        the existing route on the same inputs: association_cost + linear_assignment (one decision per side, no decode)

Each one eager (E) and replayed from a captured graph (G).  ms per frame from device events around windows of >= --window
seconds; all series alternate in one process, --repeats windows each; min, median and max of the windows are reported.
Before timing, every configuration's decode is compared with the restatement's on the device's own matrix and assignment.
What it does NOT measure: the match that produces the logits.  Fails without a GPU.

    python tools/bench_decisions.py [--out profiles/<record>.json]
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

SIZES = ((40, 30), (200, 100))    # (capacity, detections per frame)
CONFIGS = ((1, 1, "margin", False), (1, 1, "softmax", False), (2, 0, "margin", False), (2, 0, "softmax", False),
           (2, 0, "margin", True), (2, 1, "margin", False), (2, 1, "softmax", False))


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
        raise SystemExit("bench_decisions: no GPU (this tool measures on the device only)")
    import decisions_ref as R
    from pcr_amd import associate as A
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda t: t.detach().cpu().numpy()
    rows = []
    for T, D in SIZES:
        logits, pairs, count, _, _ = R.random_case(T, D, 0, 0, seed=[T, D])
        g = np.random.default_rng([D, T])
        det, trk = g.standard_normal((2, D)).astype(np.float32), g.standard_normal((1, T)).astype(np.float32)
        d_logits, d_pairs, d_count, d_det, d_trk = dev(logits), dev(pairs), dev(np.array([count], np.int32)), dev(det), dev(trk)
        series = {}

        def baseline():
            cost = A.association_cost(d_logits, d_pairs, d_count, T, D, track_miss=d_trk[0], det_new=d_det[0])
            return A.linear_assignment(cost)

        def make(dd, td, kind, reduce):
            dv, tv = (d_det[:dd].contiguous() if dd else None), (d_trk[:td].contiguous() if td else None)

            def step():
                out = A.association_cost_multi(d_logits, d_pairs, d_count, T, D, dv, tv, kind=kind, reduce=reduce)
                cost, choices = (out[0], out[1:]) if reduce else (out, None)
                assignment = A.linear_assignment(cost)
                return cost, assignment, choices, A.decode_assignment(cost, assignment, T, D, dd, td, choices=choices,
                                                                      born_decision=dd - 1, kill_decision=td - 1)
            return step

        series["B"] = baseline
        for dd, td, kind, reduce in CONFIGS:
            name = "%d_%d_%s%s" % (dd, td, kind, "_reduce" if reduce else "")
            step = series[name] = make(dd, td, kind, reduce)
            cost, assignment, choices, got = step()                  # (the warm-up, and the check against the restatement)
            h = None if choices is None else tuple(host(c) for c in choices)
            want = R.decode(host(cost), host(assignment[0]), host(assignment[1]), T, D, dd, td, choices=h, born_dec=dd - 1,
                            kill_dec=td - 1, solver_info=int(assignment[2][0]))
            for k in want:
                assert np.array_equal(host(got[k]), want[k]), "%s: the device's %s differs from the restatement's" % (name, k)
        baseline()
        torch.cuda.synchronize()
        graphs = {}
        for name, fn in series.items():
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                fn()
        times = {(name, mode): [] for name in series for mode in "EG"}
        for _ in range(args.repeats):
            for name, fn in series.items():
                times[(name, "E")].append(window(fn, args.window))
                times[(name, "G")].append(window(graphs[name].replay, args.window))
        row = {"capacity": T, "detections": D, "listed_pairs": int(count)}
        for (name, mode), t in times.items():
            row["%s_%s_ms" % (name, mode)] = {"min": round(min(t), 4), "median": round(float(np.median(t)), 4),
                                              "max": round(max(t), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_decisions.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0),
           "note": "<dd>_<td>_<kind>[_reduce] = association_cost_multi + linear_assignment + decode_assignment for one frame; "
                   "B = association_cost + linear_assignment on the same inputs (no decode).  _E_ eager, _G_ replayed from a "
                   "captured graph.  ms per frame (device events), min / median / max of the repeated windows, all series "
                   "alternating in one process.  The match that produces the logits is not part of any series",
           "shapes": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
