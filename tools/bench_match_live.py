#!/usr/bin/env python3
"""Times what a tracker frame pays for scoring the padding of its fixed-shape pair list, and what the gated launches
(ReIDNet.match_gallery(count=), include/pcr.h pcr_live) save: a bank of C slots and D detections with (64, 128) features
from the toy Point-Transformer, the full C x D pair list (cap rows, as compare_pairs makes it).

  U  match_gallery(pairs): every row of the list is scored -- what the un-gated route costs whatever the count
  L  match_gallery(pairs, count=t) with t = 0, 5 %, 20 % and 100 % of cap; the 100 % row is the cost of the gate itself
  each eager and replayed from one captured graph (ONE graph for all four counts: only the device count changes)
  F  whole track_step frames of a scripted scene (D objects in 3 classes that drive on; the bank fills with D tracks), with
     live_only off and on, eager; `live_share` is the frame's count / cap

Device events around windows of >= --window seconds after a warm-up; the variants of a shape alternate in one process,
--repeats windows each; median / min / max.  Fails without a GPU.

    python tools/bench_match_live.py [--out profiles/<record>.json]
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
N, W, FRAMES = 128, 9, 4
SHARES = (0.0, 0.05, 0.2, 1.0)


def window(fn, seconds, per=1):
    """ms per call (per frame) over a window of at least `seconds` (device events; the call count is fixed from a pilot)"""
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
    return e0.elapsed_time(e1) / calls / per


def stats(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def scene(D, n_pts, seed):
    """FRAMES frames of D box-shaped objects in 3 classes on a grid, driving along x: (sweep, boxes, labels, scores)"""
    import crops_ref as CR
    from pcr_amd import testing as PT
    g = np.random.default_rng(seed)
    objs = PT.synthetic_clouds(D, n_pts, seed=seed, kind="box").numpy()
    centre = np.stack([np.array([12.0 * (m % 10) - 54.0, 9.0 * (m // 10) - 40.0, 0.0]) + g.uniform(-1, 1, 3) for m in range(D)])
    rz = g.uniform(-np.pi, np.pi, D)
    labels = (np.arange(D) % 3).astype(np.int32)
    out = []
    for f in range(FRAMES):
        c = centre + f * np.array([0.5, 0.0, 0.0])
        boxes = np.zeros((D, W), np.float32)
        boxes[:, :3] = c - np.array([0, 0, 0.5 * 1.5 * 1.01])
        boxes[:, 3:6] = np.array([2.0, 4.0, 1.5]) * 1.01
        boxes[:, 6] = rz
        pts = np.concatenate([CR.to_sensor(objs[m].astype(np.float64), c[m], rz[m]) for m in range(D)])
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
                         (pts[g.permutation(len(pts))].astype(np.float32), boxes, labels, g.uniform(0.3, 1.0, D).astype(np.float32))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match_live: no GPU (this tool measures on the device only)")
    import bench
    from pcr_amd import testing as PT
    from pcr_amd import tracks as TR
    model, _ = bench.build_pt_model([N, 64, 32])
    rows = []
    with torch.no_grad():
        cal = PT.synthetic_clouds(16, N, seed=1, kind="box").cuda()
        model.calibrate_precision(cal[:8], cal[8:])
        for C, D in SIZES:
            cap = C * D
            xyz, h = model.forward_inference(PT.synthetic_clouds(C + D, N, seed=C, kind="box").cuda())[:2]
            h, xyz = h.contiguous(), xyz.contiguous()
            t_idx, d_idx = torch.meshgrid(torch.arange(C), torch.arange(D), indexing="ij")
            pairs = torch.stack([t_idx.reshape(-1), d_idx.reshape(-1) + C], dim=1).to(torch.int32).cuda()
            count = torch.zeros((1,), dtype=torch.int32, device="cuda")
            counts = [int(round(s * cap)) for s in SHARES]
            ref = model.match_gallery(h, xyz, pairs)                     # warm, and the values the gated route must give
            for c in counts:
                count.fill_(c)
                got = model.match_gallery(h, xyz, pairs, count=count)
                assert torch.equal(got[:c], ref[:c]) and bool((got[c:] == 0).all()), "gated logits differ at count %d" % c
            torch.cuda.synchronize()
            g_un, g_live = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_un):
                model.match_gallery(h, xyz, pairs)
            with torch.cuda.graph(g_live):
                model.match_gallery(h, xyz, pairs, count=count)
            variants = [("U_ungated", None, lambda: model.match_gallery(h, xyz, pairs), g_un.replay)]
            for s, c in zip(SHARES, counts):
                variants.append(("L_count_%d" % c, c, lambda: model.match_gallery(h, xyz, pairs, count=count), g_live.replay))
            times = {name: ([], []) for name, _, _, _ in variants}
            for _ in range(args.repeats):
                for name, c, eager, replay in variants:
                    if c is not None:
                        count.fill_(c)
                    times[name][0].append(window(eager, args.window))
                    times[name][1].append(window(replay, args.window))
            row = {"capacity": C, "detections": D, "cap_pairs": cap, "points": N, "match_ms": {}}
            for name, c, _, _ in variants:
                row["match_ms"][name] = {"count": cap if c is None else c, "eager": stats(times[name][0]),
                                         "graph": stats(times[name][1])}
            # whole frames
            frames = scene(D, N + 20, seed=D)
            banks = {lo: TR.TrackBank(C, D, feat_shape=(64, N), box_width=W) for lo in (False, True)}
            shares = []

            def run(lo, record=False):
                bank = banks[lo]
                bank.reset()
                for f, (pts, boxes, labels, scores) in enumerate(frames):
                    out = model.track_step(bank, pts, boxes, labels, scores, crop_args=dict(seed=5 + f), live_only=lo)
                    if record:
                        shares.append(round(int(out["count"][0]) / cap, 4))
                return out

            a, b = run(False, record=True), run(True)
            for k in ("track_to_det", "det_to_track", "cost", "det_id"):
                assert torch.equal(a[k], b[k]), "live_only changes %s" % k
            tf = {False: [], True: []}
            for _ in range(args.repeats):
                for lo in (False, True):
                    tf[lo].append(window(lambda: run(lo), args.window, FRAMES))
            row["frame_ms"] = {"live_share_per_frame": shares, "live_only_off": stats(tf[False]), "live_only_on": stats(tf[True])}
            rows.append(row)
            print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_match_live.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "precision": model.precision_level(),
           "note": "match_ms: ReIDNet.match_gallery over the full capacity x detections pair list of 128-point features; "
                   "U = un-gated (every row scored: the cost of the route without count=, whatever the count), L = "
                   "count= with the device count at 0 / 5 % / 20 % / 100 % of the list (100 % = the cost of the gate "
                   "itself); eager = the Python call, graph = one captured graph replayed (the same graph for every "
                   "count).  frame_ms: whole ReIDNet.track_step frames (crops, encoder, pair list, match, cost, "
                   "assignment, bank update, track NMS) of a scripted scene from an empty bank, eager, ms per frame; "
                   "live_share_per_frame = count / cap of each frame.  linear_assignment still runs over capacity + "
                   "detections on both sides.  ms, median / min / max of the repeated windows (device events), the "
                   "variants of a shape alternating in one process",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
