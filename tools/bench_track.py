#!/usr/bin/env python3
"""Times the track-state step behind the assignment on scripted frames (tests/track_ref.py's generator: a bank of C slots,
D detections per frame in 3 classes, (64, 128) features, frame limit 3, a crowded scene so that the track NMS has work):

  S  TrackBank.distances + update + suppress (pcr_amd/tracks.py: fixed-shape launches, no host read)
  G  the same three calls replayed from one captured graph
  H  a torch / host restatement of the reference's route for the same frame: the detections' centres go to the host, are
     transformed in numpy and come back for torch.cdist (get_track_det_distances); the two maps and the small state are
     read back, the decisions are taken on the host (tests/track_ref.py::plan, Python loops as the reference's
     TrackingUpdater) and uploaded, the features are replaced through a torch.where of data-dependent shape
     (PointFeatureSet.replace_old), the track NMS mask is read back and the tracks pruned on the host

A call runs the --frames frames of a sequence from an empty bank; the figures are ms per FRAME.  Device events around
windows of >= --window seconds after a warm-up for S and G, a host clock around H (it ends with the state uploaded and
the device idle); S, G and H alternate in one process, --repeats windows each; the spread is reported next to the median.
What it does NOT measure: the cost of running the match and the assignment over the full capacity instead of over the
active tracks.  Fails without a GPU.

    python tools/bench_track.py [--out profiles/<record>.json]
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

SIZES = ((40, 30), (200, 100))    # (capacity, detections per frame)
FEAT, W, LIMIT, THRESH = (64, 128), 9, 3, 0.1


def window(fn, seconds, per):
    """ms per frame over a window of at least `seconds` (device events; the call count is fixed from a pilot)"""
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


def host_window(fn, seconds, per):
    """ms per frame of a routine that drives the device from the host and ends with the device idle"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(3, int(np.ceil(seconds / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls / per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track: no GPU (this tool measures on the device only)")
    import nms_ref as NR
    import track_ref as R
    from pcr_amd import nms as NMS
    from pcr_amd import tracks as T
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rows = []
    for C, D in SIZES:
        g = np.random.default_rng([C, D])
        st = R.new_state(C, W)
        frames, want = [], None
        for f in range(args.frames):                                 # the script, driven by the restatement
            fr = R.make_frame(g, st, D, W, p_valid=0.9, span=0.5 * D)
            carry, carry_inv = R.rigid(g, span=1.0)
            st = R.plan_frame(st, fr, carry=carry, frame_limit=LIMIT)[0]
            score = (st["steps"].astype(np.float32) + st["scores"]).astype(np.float32)
            st = R.retire(NR.track_nms(NR.nearest_bev(st["boxes"][:, :7]), st["labels"], score, THRESH), st)
            frames.append(dict(track_to_det=dev(fr["track_to_det"]), det_to_track=dev(fr["det_to_track"]),
                               labels=dev(fr["labels"]), lengths=dev(fr["lengths"]), boxes=dev(fr["boxes"]),
                               scores=dev(fr["scores"]), born=dev(fr["born"]), kill=dev(fr["kill"]), carry=dev(carry),
                               carry_inv=dev(carry_inv), host=fr, carry_h=carry, carry_inv_h=carry_inv,
                               feats=torch.randn((D,) + FEAT, device="cuda"), xyz=torch.randn((D, FEAT[1], 3), device="cuda")))
        want = st
        bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)
        S = {k: v.clone() for k, v in frames[0].items() if isinstance(v, torch.Tensor)}      # the capture's static inputs

        def step(fr):
            bank.distances(fr["boxes"], fr["carry_inv"])
            bank.update((fr["track_to_det"], fr["det_to_track"]), fr, born=fr["born"], kill=fr["kill"], carry=fr["carry"],
                        frame_limit=LIMIT)
            bank.suppress(THRESH)

        def fs():
            bank.reset()
            for fr in frames:
                step(fr)

        fs()
        torch.cuda.synchronize()
        for k in R.STATE:
            assert np.array_equal(getattr(bank, k).cpu().numpy(), want[k]), "the device's state differs: %s" % k
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(S)

        def fg():
            bank.reset()
            for fr in frames:
                for k in S:
                    S[k].copy_(fr[k])
                graph.replay()

        fg()
        torch.cuda.synchronize()
        for k in R.STATE:
            assert np.array_equal(getattr(bank, k).cpu().numpy(), want[k]), "the replayed state differs: %s" % k

        host_bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)

        def fh():
            b = host_bank
            b.reset()
            for fr in frames:
                # get_track_det_distances: detections to the host, numpy affine, back, cdist over the active tracks
                xyz1 = np.concatenate([fr["boxes"][:, :3].cpu().numpy(), np.ones((D, 1), np.float32)], 1)
                prev = torch.from_numpy((xyz1 @ fr["carry_inv_h"].reshape(3, 4).T).astype(np.float32)).cuda()
                act = torch.where(b.ids >= 0)[0]
                torch.cdist(b.boxes[act, :2], prev[:, :2], p=2.0)
                # the decisions on the host
                hst = {k: getattr(b, k).cpu().numpy() for k in R.STATE}
                t2d, d2t = fr["track_to_det"].cpu().numpy(), fr["det_to_track"].cpu().numpy()
                h = fr["host"]
                new, src, _, _ = R.plan(hst, t2d, d2t, h["labels"], fr["lengths"].cpu().numpy(), h["boxes"], h["scores"],
                                        born=h["born"], kill=h["kill"], carry=fr["carry_h"], frame_limit=LIMIT)
                for k in R.STATE:
                    getattr(b, k).copy_(torch.from_numpy(new[k]))
                # replace_old / store_new: an index list of data-dependent length
                src_d = torch.from_numpy(src).cuda()
                rows_ = torch.where(src_d >= 0)[0]
                b.feats[rows_] = fr["feats"][src_d[rows_].long()]
                b.xyz[rows_] = fr["xyz"][src_d[rows_].long()]
                # non_max_suppression: the mask is read back and the tracks pruned on the host
                mask = NMS.suppress_tracks(b.boxes[:, :7], b.labels, b.track_scores(), THRESH).cpu().numpy()
                ids = b.ids.cpu().numpy()
                hit = (ids >= 0) & (mask != 0)
                for name, fill in (("ids", -1), ("labels", -1), ("lengths", 0)):
                    a = getattr(b, name).cpu().numpy()
                    a[hit] = fill
                    getattr(b, name).copy_(torch.from_numpy(a))

        fh()
        torch.cuda.synchronize()
        for k in R.STATE:
            assert np.array_equal(getattr(host_bank, k).cpu().numpy(), want[k]), "the host route's state differs: %s" % k
        ts, tg, th = [], [], []
        for _ in range(args.repeats):
            ts.append(window(fs, args.window, args.frames))
            tg.append(window(fg, args.window, args.frames))
            th.append(host_window(fh, args.window, args.frames))
        row = {"capacity": C, "detections": D, "feat_shape": list(FEAT), "frames": args.frames,
               "active_at_end": int((want["ids"] >= 0).sum())}
        for k, t in (("S_bank_step_ms_per_frame", ts), ("G_graph_replay_ms_per_frame", tg), ("H_host_route_ms_per_frame", th)):
            row[k] = {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_track.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0),
           "note": "S = TrackBank.distances + update + suppress per frame, eager (device events); G = the same calls "
                   "replayed from one captured graph, the frame's inputs copied into static buffers first (device events); "
                   "H = a torch / host restatement of the reference's route for the same frames (host clock, ends with "
                   "the device idle): detections to the host and back for cdist, decisions on the host in Python "
                   "(tests/track_ref.py::plan), features replaced through torch.where, the NMS mask read back.  ms per "
                   "frame, median / min / max of the repeated windows, S, G and H alternating in one process; each call "
                   "runs the whole sequence from an empty bank (the reset is included on all three sides).  The match "
                   "and the assignment over the full capacity are NOT part of any of the three",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
