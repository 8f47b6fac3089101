#!/usr/bin/env python3
"""Times the crop step in front of forward_inference on seeded scenes (tests/crops_ref.py's generator):

  A  pcr_amd.crops.crops_from_boxes (one launch, no host read)
  B  the reference's METHOD restated with torch ops on the device -- broadcast membership (P, M), one nonzero per box
     (a host sync each), torch.randint on the host per box, gather (trackers/deprecated/pc_utils.py:31-96).  It is written
     here, not shipped: the reference's own code needs pytorch3d and its CUDA extension, which cannot be built for this
     device, so it cannot be the baseline itself.
  C  ReIDNet.forward_inference on the same M crops (Point-Transformer for n = 128, PointNet++ SSG for n = 1024), for scale.

Device events around windows of >= --window seconds after a warm-up, A and B alternating in one process, --repeats
windows each; the spread of the repeats is reported next to the median.  Fails without a GPU.

    python tools/bench_crops.py [--out profiles/<record>.json]
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

SHAPES = ((30000, 100, 128), (250000, 200, 128), (250000, 200, 1024))      # (background points, boxes, n)


def method_b(points, boxes, n):
    """interpolate_per_frame + get_input_batch with torch ops: (M, n, 3) box-frame crops, (M,) lengths"""
    xyz = points[:, :3]
    cz = boxes[:, 2] + boxes[:, 5] / 2
    rot = boxes[:, 6] + np.pi / 2
    c, s = torch.cos(rot), torch.sin(rot)
    sx, sy = xyz[:, None, 0] - boxes[None, :, 0], xyz[:, None, 1] - boxes[None, :, 1]
    lx, ly = sx * c - sy * s, sx * s + sy * c
    dz = xyz[:, None, 2] - cz[None]
    inside = (dz.abs() <= boxes[None, :, 5] / 2) & (lx.abs() < boxes[None, :, 4] / 2) & (ly.abs() < boxes[None, :, 3] / 2)
    out = torch.zeros((boxes.shape[0], n, 3), device=points.device)
    lengths = []
    for m in range(boxes.shape[0]):
        idx = inside[:, m].nonzero()[:, 0]                 # a host sync per box, as the reference's boolean indexing
        ln = idx.numel()
        lengths.append(ln)
        if ln:
            pick = idx[torch.randint(high=ln, size=(n,)).to(points.device)]
            out[m] = torch.stack([lx[pick, m], ly[pick, m], dz[pick, m]], dim=1)
    return out, torch.tensor(lengths, device=points.device)


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
    return e0.elapsed_time(e1) / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crops: no GPU (this tool measures on the device only)")
    import bench
    import crops_ref as R
    from pcr_amd import crops
    models = {128: bench.build_pt_model([128, 64, 32])[0], 1024: bench.build_model("ssg", None)[0]}
    rows = []
    for nbg, M, n in SHAPES:
        pts, boxes = R.make_scene(nbg, M, seed=1 if nbg == 30000 else 2)
        dp, db = torch.from_numpy(pts).cuda(), torch.from_numpy(boxes).cuda()
        seed = torch.zeros(1, dtype=torch.int64, device="cuda")
        out = (torch.empty((M, n, 3), device="cuda"), torch.empty((M,), dtype=torch.int32, device="cuda"))
        model = models[n]

        def fa():
            seed.add_(1)
            crops.crops_from_boxes(dp, db, n, seed=seed, out=out)

        def fb():
            method_b(dp, db, n)

        with torch.no_grad():
            crops.crops_from_boxes(dp, db, n, seed=seed, out=out)
            lb = method_b(dp, db, n)[1]
            # (B rotates with torch's own cos / sin and contraction: a point on a face may fall the other way)
            assert int((lb.int() - out[1]).abs().sum()) <= 8, "the two methods disagree on the point counts"
            model.calibrate_precision(out[0][:M // 2], out[0][M // 2:])

            def fc():
                model.forward_inference(out[0])
            for f in (fa, fb, fc):                          # warm-up of every shape the windows use
                for _ in range(3):
                    f()
            ta, tb, tc = [], [], []
            for _ in range(args.repeats):                   # A and B alternate; C rides along
                ta.append(window(fa, args.window)[0])
                tb.append(window(fb, args.window)[0])
                tc.append(window(fc, args.window)[0])
        row = {"points": int(pts.shape[0]), "boxes": M, "n": n}
        for k, t in (("A_crops_from_boxes_ms", ta), ("B_torch_restatement_ms", tb), ("C_forward_inference_ms", tc)):
            row[k] = {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_crops.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0),
           "note": "A = the fused HIP crop (seed bumped on the device before each call); B = the reference's method restated "
                   "with torch ops (membership matrix, per-box nonzero + host randint + gather), NOT the reference's own code "
                   "(pytorch3d + its CUDA extension cannot be built for this device); C = forward_inference of the same M "
                   "crops (Point-Transformer at n = 128, PointNet++ SSG at n = 1024).  ms per call, median / min / max of the "
                   "repeated windows, A and B alternating in one process",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
