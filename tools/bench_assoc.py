#!/usr/bin/env python3
"""Times the association step behind match_gallery on reference-shaped frames (tests/assoc_ref.py's generator: T = D
objects in 8 classes, logits ~ N(0, 4^2), N(0, 1) miss / new costs, fill 10000):

  A  compare_pairs + association_cost + linear_assignment (pcr_amd/associate.py: fixed-shape launches, no host read)
  L  pcr_lsa_f32 alone on the same matrix
  H  the host route of the reference for the same matrix: cost.cpu().numpy() + scipy.optimize.linear_sum_assignment
     when scipy is importable, otherwise the numpy restatement (tests/assoc_ref.py::lsa) -- the record says which

Device events around windows of >= --window seconds after a warm-up for A and L, a host clock around H (it ends in the
solver's return, after the device-to-host copy); A, L and H alternate in one process, --repeats windows each; the spread
is reported next to the median.  Fails without a GPU.

    python tools/bench_assoc.py [--out profiles/<record>.json]
"""
import argparse
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

SIZES = (50, 100, 200)            # T = D
CLASSES = 8


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


def host_window(fn, seconds):
    """ms per call of a host routine that returns only when its result is on the host"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    calls = max(3, int(np.ceil(seconds / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assoc: no GPU (this tool measures on the device only)")
    import assoc_ref as R
    from pcr_amd import associate as A
    try:
        from scipy.optimize import linear_sum_assignment
        host_solver = "scipy.optimize.linear_sum_assignment (float64)"
    except ImportError:
        linear_sum_assignment = None
        host_solver = "tests/assoc_ref.py::lsa (numpy restatement; scipy is not importable here)"
    rows = []
    for n in SIZES:
        T = D = n
        cost_h, logits_h, _, count, miss_h, new_h, (tl_h, dl_h) = R.reference_case(T, D, seed=n, classes=CLASSES)
        steps = R.lsa(cost_h, count_steps=True)[-1]
        tl, dl = torch.from_numpy(tl_h.astype(np.int32)).cuda(), torch.from_numpy(dl_h.astype(np.int32)).cuda()
        logits, miss, new = (torch.from_numpy(x).cuda() for x in (logits_h, miss_h, new_h))
        N = T + D
        out_p = (torch.empty((T * D, 2), dtype=torch.int32, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"))
        out_c = torch.empty((N, N), device="cuda")
        out_l = (torch.empty((1, N), dtype=torch.int32, device="cuda"), torch.empty((1, N), dtype=torch.int32, device="cuda"),
                 torch.empty((1,), dtype=torch.int32, device="cuda"))

        def fa():
            pairs, cnt = A.compare_pairs(tl, dl, num_classes=CLASSES, out=out_p)
            A.association_cost(logits, pairs, cnt, T, D, track_miss=miss, det_new=new, out=out_c)
            A.linear_assignment(out_c, out=out_l)

        def fl():
            A.linear_assignment(out_c, out=out_l)

        def fh():
            c = out_c.cpu().numpy()
            if linear_sum_assignment is not None:
                return linear_sum_assignment(c.astype(np.float64))
            return R.lsa(c)

        fa()
        torch.cuda.synchronize()
        assert np.array_equal(out_c.cpu().numpy().view(np.uint32), cost_h.view(np.uint32)), "the device's matrix differs"
        want = R.lsa(cost_h)
        assert int(out_l[2]) == 0 and np.array_equal(out_l[0][0].cpu().numpy(), want[0]), "the device's assignment differs"
        if linear_sum_assignment is not None:
            assert np.array_equal(fh()[1], want[0]), "scipy's assignment differs from the restatement's"
        for f in (fa, fl, fh):
            for _ in range(3):
                f()
        ta, tl_, th = [], [], []
        for _ in range(args.repeats):
            ta.append(window(fa, args.window))
            tl_.append(window(fl, args.window))
            th.append(host_window(fh, args.window))
        row = {"T": T, "D": D, "classes": CLASSES, "matrix": [N, N], "listed_pairs": int(count), "search_steps": int(steps)}
        for k, t in (("A_three_launches_ms", ta), ("L_pcr_lsa_f32_ms", tl_), ("H_host_route_ms", th)):
            row[k] = {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_assoc.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "host_solver": host_solver,
           "note": "A = compare_pairs + association_cost + linear_assignment into caller-owned buffers (device events); "
                   "L = pcr_lsa_f32 alone on the same matrix (device events); H = the reference's host route for that "
                   "matrix, cost.cpu().numpy() + the host solver named above (host clock, ends with the result on the "
                   "host).  ms per call, median / min / max of the repeated windows, A, L and H alternating in one "
                   "process.  search_steps: column selections the restatement counts for the matrix",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
