#!/usr/bin/env python3
"""Times the scoring against ground truth (pcr_amd/truth.py, include/pcr.h section A7) in a ReIDNet.track_step frame of the
toy Point-Transformer, on bench_match_live.py's scripted scene (D objects in 3 classes that drive on; the detections ARE
the ground-truth boxes, so every detection is a true positive), at (capacity, detections, ground truth) = SIZES:

  F   whole track_step frames (live_only) without truth=, eager, and F+ with truth= (book.match, book.decide before the
      update, book.record after the track NMS)
  G   one such frame replayed from a captured graph, the frame's inputs copied into static buffers first, without / with
      truth= (G, G+)
  T   the truth half alone on the last frame's recorded inputs: match + decide + record, eager and replayed (TG)
  H   a torch / host restatement of the reference's route for that same half: cdist + class mask on the device, the matrix
      to the host for scipy's linear_sum_assignment (tests/assoc_ref.py::lsa where scipy is missing: see "lsa" in the
      record), the threshold through torch.where, then the index lists to the host for np.intersect1d, the decision sets,
      get_stats and update_gt_track_mapping (tests/truth_ref.py::ListTruth)

ms per frame; device events around windows of >= --window seconds for F, G, T, a host clock around H (it ends with the
device idle); the variants alternate in one process, --repeats windows each; median / min / max.  Fails without a GPU.

    python tools/bench_truth.py [--out profiles/<record>.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = ((40, 30, 30), (200, 100, 100))    # (capacity, detections, ground-truth boxes per frame)
N, W, THRESH = 128, 9, 2.0


def host_window(fn, seconds):
    """ms per call of a routine that drives the device from the host and ends with the device idle"""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_truth: no GPU (this tool measures on the device only)")
    import bench
    import assoc_ref as AR
    import truth_ref as R
    from bench_match_live import FRAMES, scene, stats, window
    from pcr_amd import testing as PT
    from pcr_amd import tracks as TR
    from pcr_amd import truth as TU
    try:
        from scipy.optimize import linear_sum_assignment
        lsa_name = "scipy"
    except ImportError:
        linear_sum_assignment = lambda c: (np.arange(c.shape[0]), AR.lsa(c)[0])      # (square problems here: every row assigned)
        lsa_name = "tests/assoc_ref.py::lsa (scipy is not installed)"
    model, _ = bench.build_pt_model([N, 64, 32])
    rows = []
    with torch.no_grad():
        cal = PT.synthetic_clouds(16, N, seed=1, kind="box").cuda()
        model.calibrate_precision(cal[:8], cal[8:])
        for C, D, G in SIZES:
            frames = scene(D, N + 20, seed=D)
            gt_ids = torch.arange(G, dtype=torch.int32, device="cuda")
            banks = {t: TR.TrackBank(C, D, feat_shape=(64, N), box_width=W) for t in (False, True)}
            book = TU.TruthBook(banks[True], G, G, kind="centre", thresh=THRESH)

            def truth_of(f, boxes, labels):
                return dict(book=book, boxes=boxes, labels=labels, ids=gt_ids, tte=torch.full_like(gt_ids, FRAMES - 1 - f))

            rec = {}

            def run(with_truth, record=False):
                bank = banks[with_truth]
                bank.reset()
                book.reset()
                for f, (pts, boxes, labels, scores) in enumerate(frames):
                    if record and f == FRAMES - 1:
                        rec["ids_before"] = bank.ids.clone()
                    out = model.track_step(bank, pts, boxes, labels, scores, crop_args=dict(seed=5), live_only=True,
                                           truth=truth_of(f, boxes, labels) if with_truth else None)
                return out

            a, b = run(False), run(True, record=True)
            for k in a:
                assert a[k] is None or torch.equal(a[k], b[k]), "truth= changes %s" % k
            m = book.metrics()
            assert m["tp"] == FRAMES * D and m["fp"] == m["fn"] == 0, m
            last = {k: v.clone() for k, v in b.items() if isinstance(v, torch.Tensor)}
            next_id = int(banks[True].next_id[0])
            # the truth half alone, on the last frame's recorded inputs
            pts, boxes, labels, scores = frames[-1]
            labels32 = labels.to(torch.int32)
            gt = dict(boxes=boxes, labels=labels32, ids=gt_ids, tte=torch.zeros_like(gt_ids))
            half = TU.TruthBook(banks[True], G, G, kind="centre", thresh=THRESH)

            def truth_half():
                half.match(boxes, labels32, gt)
                half.decide((last["track_to_det"], last["det_to_track"]), labels32)
                half.record(last["det_slot"], last["det_id"])

            truth_half()
            torch.cuda.synchronize()
            g_half = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_half):
                truth_half()
            gt_ids_h, gt_tte_h = gt_ids.cpu().numpy().astype(np.int64), np.zeros(G, np.int64)
            lt = R.ListTruth()

            def host_route():
                lt.trkid_to_gt = np.arange(next_id, dtype=np.int64) % G          # what earlier frames left (any content)
                lt.trkid_to_tte = np.ones(next_id, np.int64)
                mask = (labels32[:, None] != labels32[None, :]).float() * 10000.0
                cost = torch.cdist(boxes[:, :2], boxes[:, :2]) + mask
                r, c = linear_sum_assignment(cost.cpu().numpy())
                r_d, c_d = torch.from_numpy(np.asarray(r)).cuda(), torch.from_numpy(np.asarray(c)).cuda()
                keep = torch.where(cost[r_d, c_d] < THRESH)
                tp_det, tp_gt = r_d[keep].cpu().numpy(), c_d[keep].cpu().numpy()
                ids = rec["ids_before"].cpu().numpy()
                slots = np.nonzero(ids >= 0)[0]
                cs = {int(s): i for i, s in enumerate(slots)}
                tp = lt.decisions(ids[slots].astype(np.int64), tp_det, tp_gt, gt_ids_h, D)
                t2d = last["track_to_det"].cpu().numpy()
                matched = [(int(s), int(t2d[s])) for s in slots if t2d[s] >= 0]
                taken = {d for _, d in matched}
                lt.get_stats(dict(track_match=[cs[s] for s, _ in matched], det_match=[d for _, d in matched],
                                  det_newborn=[d for d in range(D) if d not in taken], det_false_positive=[],
                                  track_false_positive=[], track_false_negative=[cs[int(s)] for s in slots if t2d[s] < 0]), tp)
                det_id = last["det_id"].cpu().numpy().astype(np.int64)
                kept = np.nonzero(det_id >= 0)[0]
                ck = {int(d): i for i, d in enumerate(kept)}
                sel = [i for i, d in enumerate(tp_det) if int(d) in ck]
                lt.update_mapping(next_id, gt_tte_h, gt_ids_h, np.array([ck[int(tp_det[i])] for i in sel], np.int64),
                                  tp_gt[sel].astype(np.int64), det_id[kept])

            host_route()
            variants = [("F_frame_eager", lambda: run(False), FRAMES), ("F+_frame_eager_truth", lambda: run(True), FRAMES),
                        ("T_truth_half_eager", truth_half, 1), ("TG_truth_half_graph", g_half.replay, 1)]
            times = {name: [] for name, _, _ in variants}
            th = []
            for _ in range(args.repeats):
                for name, fn, per in variants:
                    times[name].append(window(fn, args.window, per))
                th.append(host_window(host_route, args.window))
            row = {"capacity": C, "detections": D, "ground_truth": G, "points": N, "frames": FRAMES}
            for name, _, _ in variants:
                row[name + "_ms"] = stats(times[name])
            row["H_host_route_ms"] = stats(th)
            rows.append(row)
            print(json.dumps(row), flush=True)
            dump(args, model, lsa_name, rows)
            # one whole frame from a graph, last: the bank is in the state the eager runs left (full), the inputs are static
            S = [t.clone() for t in frames[-1]]
            graphs = {}
            for t in (False, True):                              # (an error here ends the run: nothing is launched after it)
                torch.cuda.synchronize()
                graphs[t] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[t]):
                    model.track_step(banks[t], S[0], S[1], S[2], S[3], crop_args=dict(seed=5), live_only=True,
                                     truth=truth_of(FRAMES - 1, S[1], S[2]) if t else None)

            def replay(t):
                for dst, src in zip(S, frames[-1]):
                    dst.copy_(src)
                graphs[t].replay()

            tg = {False: [], True: []}
            for _ in range(args.repeats):
                for t in (False, True):
                    tg[t].append(window(lambda: replay(t), args.window, 1))
            row["G_frame_graph_ms"], row["G+_frame_graph_truth_ms"] = stats(tg[False]), stats(tg[True])
            print(json.dumps({k: row[k] for k in ("G_frame_graph_ms", "G+_frame_graph_truth_ms")}), flush=True)
            dump(args, model, lsa_name, rows)


def dump(args, model, lsa_name, rows):
    """the record as it stands (rewritten after every stage, so that a run that ends in an error leaves the earlier ones)"""
    out = {"tool": "tools/bench_truth.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "precision": model.precision_level(), "lsa": lsa_name,
           "note": "ms per frame, median / min / max of the repeated windows, the variants alternating in one process.  F / F+: "
                   "whole eager ReIDNet.track_step frames (live_only) of a scripted scene without / with truth= (a call runs "
                   "the scene's frames from an empty bank and an empty book; the resets are included on both sides); G / G+: "
                   "the last frame replayed from one captured graph over a full bank, inputs copied into static buffers "
                   "first; T / TG: book.match + decide + record alone, eager / replayed; H: a torch / host restatement of "
                   "the reference's route for that half (host clock, ends with the device idle; not the reference's own "
                   "code: the mapping it reads holds synthetic content and its decision lists are built in Python loops, so "
                   "the figure is indicative only)",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
