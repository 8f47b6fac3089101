#!/usr/bin/env python3
"""Times duplicate suppression on street-shaped frames (tests/nms_ref.py's generators: clusters of near copies, N boxes):

  G  pcr_amd.nms.nms, kind "rotated" and "axis" (rank + ballot mask + one-wave sweep: fixed-shape launches, no host read)
  T  pcr_amd.nms.suppress_tracks (nearest_bev + the pairwise rule)
  Hn the reference's host route for the same NMS, restated in torch: sort on the device, the thresholded IoU matrix on the
     device (pcr_amd.nms.iou_bev, so both sides pay the same overlap arithmetic), packed to 64-bit words, copied to the
     host, the greedy sweep of iou3d.cpp:128-143 in a host loop over the words, the kept indices copied back
  Ht the reference's track NMS in torch ops (virtual_tracker.py:232-259): class mask, triu, torch.where (a host sync),
     the score compare and the suppressed index lists on the host

Device events around windows of >= --window seconds after a warm-up for G and T, a host clock around Hn and Ht (they end
with their result on the host); the sides alternate in one process, --repeats windows each; the spread is reported next
to the median.  Fails without a GPU.

    python tools/bench_nms.py [--out profiles/<record>.json]      (default: profiles/nms_bench.json)
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

SIZES = (200, 1000, 4096)


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


def host_nms(M, boxes, scores, thresh, kind):
    """the reference's route: everything up to the mask on the device, the sweep on the host"""
    order = scores.sort(0, descending=True)[1]
    b = boxes[order].contiguous()
    n = b.shape[0]
    nb = (n + 63) // 64
    over = torch.triu(M.iou_bev(b, b, kind=kind) > thresh, diagonal=1)
    pad = torch.zeros((n, nb * 64), dtype=torch.int64, device=b.device)
    pad[:, :n] = over
    words = (pad.view(n, nb, 64) << torch.arange(64, device=b.device)).sum(-1)       # bit 63 wraps into the sign: same bits
    mask = words.cpu().numpy().view(np.uint64)
    remv = np.zeros(nb, np.uint64)
    keep = []
    one = np.uint64(1)
    for i in range(n):
        blk = i >> 6
        if not (remv[blk] >> np.uint64(i & 63)) & one:
            keep.append(i)
            remv[blk:] |= mask[i, blk:]
    return order[torch.tensor(keep, dtype=torch.int64).to(b.device)]


def host_tracks(boxes7, classes, scores, thresh):
    """VirtualTracker.non_max_suppression's tensor work, up to the suppressed index lists on the host"""
    n = boxes7.shape[0]
    rz = boxes7[:, 6]
    r = torch.abs(rz - torch.floor(rz / np.pi + 0.5) * np.pi)
    xywh = torch.where((r > np.pi / 4)[:, None], boxes7[:, [0, 1, 4, 3]], boxes7[:, [0, 1, 3, 4]])
    bev = torch.cat([xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, :2] + xywh[:, 2:] / 2], -1)
    cp = torch.cartesian_prod(torch.arange(n), torch.arange(n)).to(boxes7.device)
    mask = torch.zeros((n, n), device=boxes7.device)
    mask[cp[:, 0], cp[:, 1]] = (classes[cp[:, 0]] != classes[cp[:, 1]]).float() * -10000.0
    lt, rb = torch.max(bev[:, None, :2], bev[None, :, :2]), torch.min(bev[:, None, 2:], bev[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = (bev[:, 2] - bev[:, 0]) * (bev[:, 3] - bev[:, 1])
    iou = inter / (area[:, None] + area[None, :] - inter).clamp(min=1e-8) + mask
    idx1, idx2 = torch.where(torch.triu(iou, diagonal=1) > thresh)
    d = scores[idx1] - scores[idx2]
    return idx1[torch.where(d <= 0)].tolist() + idx2[torch.where(d > 0)].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nms: no GPU (this tool measures on the device only)")
    import nms_ref as R
    from pcr_amd import nms as M
    rows = []
    for n in SIZES:
        row = {"N": n}
        for kind in ("rotated", "axis"):
            boxes_h, scores_h, thresh, _ = R.nms_case(n, kind)
            # distinct scores (k / n is a different float32 for every k <= 4096): torch.sort is not stable, so with ties
            # the two routes could rank differently for a reason that is not the kernels'
            scores_h = ((np.random.default_rng(n).permutation(n) + 1) / np.float32(n)).astype(np.float32)
            assert len(np.unique(scores_h)) == n
            boxes, scores = torch.from_numpy(boxes_h).cuda(), torch.from_numpy(scores_h).cuda()
            out = tuple(torch.empty((k,), dtype=torch.int32, device="cuda") for k in (n, 1, 1))

            def fg():
                M.nms(boxes, scores, thresh, kind=kind, out=out)

            def fh():
                return host_nms(M, boxes, scores, thresh, kind)

            fg()
            kept = fh()
            assert int(out[2]) == 0 and out[0][:int(out[1])].tolist() == kept.tolist(), "the two routes keep different boxes"
            for f in (fg, fh):
                for _ in range(3):
                    f()
            tg, th = [], []
            for _ in range(args.repeats):
                tg.append(window(fg, args.window))
                th.append(host_window(fh, args.window))
            row["kept_" + kind] = int(out[1])
            for k, t in (("G_nms_%s_ms" % kind, tg), ("Hn_host_route_%s_ms" % kind, th)):
                row[k] = {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        b7_h, cls_h, sc_h = R.track_case(n)
        b7, cls, sc = torch.from_numpy(b7_h).cuda(), torch.from_numpy(cls_h).cuda(), torch.from_numpy(sc_h).cuda()
        sup = torch.empty((n,), dtype=torch.int32, device="cuda")

        def ft():
            M.suppress_tracks(b7, cls, sc, 0.1, out=sup)

        def fht():
            return host_tracks(b7, cls.long(), sc, 0.1)

        ft()
        assert np.array_equal(sup.cpu().numpy(), R.track_nms(R.nearest_bev(b7_h), cls_h, sc_h, 0.1)), "the device's mask differs"
        for f in (ft, fht):
            for _ in range(3):
                f()
        tt, tht = [], []
        for _ in range(args.repeats):
            tt.append(window(ft, args.window))
            tht.append(host_window(fht, args.window))
        row["suppressed_tracks"] = int(sup.sum())
        for k, t in (("T_suppress_tracks_ms", tt), ("Ht_host_route_tracks_ms", tht)):
            row[k] = {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_nms.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0),
           "note": "G = pcr_amd.nms.nms into caller-owned buffers, T = suppress_tracks (device events); Hn = the reference's "
                   "NMS route restated in torch: device sort + thresholded IoU matrix (the same overlap kernel) + packed mask "
                   "copied to the host + the C++ sweep as a Python loop over the words + indices copied back; Ht = the "
                   "reference's track NMS in torch ops, ending with the suppressed index lists on the host (host clock for "
                   "both).  The Python loop of Hn stands in for a C++ loop: Hn is an upper bound of that route's time, its "
                   "copies and synchronisations are the part that carries over.  ms per call, median / min / max of the "
                   "repeated windows, the sides alternating in one process",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
