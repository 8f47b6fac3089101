#!/usr/bin/env python3
"""Times the identity metrics (pcr_amd/identity.py, include/pcr.h section A9) in a ReIDNet.track_step frame of the toy
Point-Transformer, on bench_match_live.py's scripted scene (the detections ARE the ground-truth boxes), at (capacity,
detections, ground truth) = SIZES:

  F+  whole track_step(truth=) frames (live_only), eager, and F++ with truth["identity"] on top (one more launch)
  G+  one such frame replayed from a captured graph, the inputs copied into static buffers first, without / with the
      identity book (G+, G++)
  R   IdentityBook.record alone on the last frame's buffers, eager and replayed (RG)
  C   IdentityBook.close_scene(reset=False) over a synthetic scene (a tracker that mostly keeps its identities, with swaps),
      eager and replayed (CG), at the default caps (200 x 400 active of 256 x 512) and at 1024 x 1024 (1000 x 1000 active),
      and Z, reset_scene alone

ms per frame / per call; device events around windows of >= --window seconds; the variants alternate in one process,
--repeats windows each; median / min / max.  Fails without a GPU.

    python tools/bench_ident.py [--out profiles/<record>.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = ((40, 30, 30), (200, 100, 100))    # (capacity, detections, ground-truth boxes per frame)
CLOSE = ((256, 512, 200, 400), (1024, 1024, 1000, 1000))      # (max_rows, max_cols, active rows, active columns)
N, W, THRESH, ID_CAP = 128, 9, 2.0, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ident: no GPU (this tool measures on the device only)")
    import bench
    import ident_ref as R
    from bench_match_live import FRAMES, scene, stats, window
    from pcr_amd import identity as ID
    from pcr_amd import testing as PT
    from pcr_amd import tracks as TR
    from pcr_amd import truth as TU
    model, _ = bench.build_pt_model([N, 64, 32])
    record = {"tool": "tools/bench_ident.py", "window_s": args.window, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "precision": None,
              "note": "ms per frame (F, G) or per call (R, C, Z), median / min / max of the repeated windows, the variants "
                      "alternating in one process.  F+ / F++: whole eager ReIDNet.track_step(truth=) frames (live_only) of a "
                      "scripted scene without / with truth['identity'] (a call runs the scene's frames from an empty bank and "
                      "empty books; the resets are included on both sides); G+ / G++: the last frame replayed from one captured "
                      "graph over a full bank; R / RG: IdentityBook.record alone, eager / replayed; C / CG: close_scene(reset="
                      "False) -- compaction, assignment, score -- over a synthetic scene, eager / replayed; Z: reset_scene",
              "frames": [], "close": []}

    def dump():
        record["precision"] = model.precision_level()
        if args.out:
            with open(args.out, "w") as f:
                json.dump(record, f, indent=1)
                f.write("\n")

    with torch.no_grad():
        cal = PT.synthetic_clouds(16, N, seed=1, kind="box").cuda()
        model.calibrate_precision(cal[:8], cal[8:])
        for C, D, G in SIZES:
            frames = scene(D, N + 20, seed=D)
            gt_ids = torch.arange(G, dtype=torch.int32, device="cuda")
            banks = {t: TR.TrackBank(C, D, feat_shape=(64, N), box_width=W) for t in (False, True)}
            books = {t: TU.TruthBook(banks[t], G, G, kind="centre", thresh=THRESH) for t in (False, True)}
            ident = ID.IdentityBook(books[True], ID_CAP)

            def truth_of(t, f, boxes, labels):
                d = dict(book=books[t], boxes=boxes, labels=labels, ids=gt_ids, tte=torch.full_like(gt_ids, FRAMES - 1 - f))
                if t:
                    d["identity"] = ident
                return d

            def run(t):
                banks[t].reset()
                books[t].reset()
                if t:
                    ident.reset()
                for f, (pts, boxes, labels, scores) in enumerate(frames):
                    out = model.track_step(banks[t], pts, boxes, labels, scores, crop_args=dict(seed=5), live_only=True,
                                           truth=truth_of(t, f, boxes, labels))
                return out

            a, b = run(False), run(True)
            for k in a:
                assert a[k] is None or torch.equal(a[k], b[k]), "identity= changes %s" % k
            assert torch.equal(books[False].stats, books[True].stats)
            ident.close_scene()
            m = ident.metrics()
            # (a bank that runs full leaves later detections without an id: pred_total may stay below tp)
            assert m["gt_total"] == m["tp"] == FRAMES * D and 0 < m["idtp"] <= m["pred_total"] <= FRAMES * D, m
            assert m["overflow"] == m["inexact"] == m["dropped_gt"] == m["dropped_id"] == 0, m
            idf1 = m["idf1"]
            ident.record()
            torch.cuda.synchronize()
            g_rec = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_rec):
                ident.record()
            variants = [("F+_frame_eager_truth", lambda: run(False), FRAMES), ("F++_frame_eager_identity", lambda: run(True), FRAMES),
                        ("R_record_eager", ident.record, 1), ("RG_record_graph", g_rec.replay, 1)]
            times = {name: [] for name, _, _ in variants}
            for _ in range(args.repeats):
                for name, fn, per in variants:
                    times[name].append(window(fn, args.window, per))
            row = {"capacity": C, "detections": D, "ground_truth": G, "points": N, "frames": FRAMES, "id_cap": ID_CAP,
                   "idf1": round(idf1, 4)}
            for name, _, _ in variants:
                row[name + "_ms"] = stats(times[name])
            record["frames"].append(row)
            print(json.dumps(row), flush=True)
            dump()
            # one whole frame from a graph, last: the banks are full, the inputs static (an error here ends the run)
            S = [t.clone() for t in frames[-1]]
            graphs = {}
            for t in (False, True):
                torch.cuda.synchronize()
                graphs[t] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[t]):
                    model.track_step(banks[t], S[0], S[1], S[2], S[3], crop_args=dict(seed=5), live_only=True,
                                     truth=truth_of(t, FRAMES - 1, S[1], S[2]))

            def replay(t):
                for dst, src in zip(S, frames[-1]):
                    dst.copy_(src)
                graphs[t].replay()

            tg = {False: [], True: []}
            for _ in range(args.repeats):
                for t in (False, True):
                    tg[t].append(window(lambda: replay(t), args.window, 1))
            row["G+_frame_graph_truth_ms"], row["G++_frame_graph_identity_ms"] = stats(tg[False]), stats(tg[True])
            print(json.dumps({k: row[k] for k in ("G+_frame_graph_truth_ms", "G++_frame_graph_identity_ms")}), flush=True)
            dump()
        # closing a scene
        bank = TR.TrackBank(40, 30, feat_shape=(64, N), box_width=W)
        for max_rows, max_cols, nr, nc in CLOSE:
            book = TU.TruthBook(bank, 30, 1024)
            ident = ID.IdentityBook(book, ID_CAP, max_rows=max_rows, max_cols=max_cols)
            cooc = np.zeros((ident.gt_rows, ID_CAP), np.int32)
            cooc[np.ix_(np.arange(nr), np.arange(nc) * 4)] = R.golden_case(nr, nc, "diagonal", seed=1)
            ident.cooc.copy_(torch.from_numpy(cooc))
            ident.gt_track[:nr, :2] = 40
            close = lambda: ident.close_scene(reset=False)
            close()
            want = int(ident.table[0])
            assert want > 0 and int(ident.table[12]) == int(ident.table[13]) == 0      # neither OVERFLOW nor INEXACT
            try:                                             # the optimum itself, where scipy is at hand
                from scipy.optimize import linear_sum_assignment
                r, c = linear_sum_assignment(cooc.astype(np.int64), maximize=True)
                assert int(cooc[r, c].sum()) == want, (int(cooc[r, c].sum()), want)
            except ImportError:
                pass
            torch.cuda.synchronize()
            g_close = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_close):
                close()
            variants = [("C_close_eager", close), ("CG_close_graph", g_close.replay), ("Z_reset_scene", ident.reset_scene)]
            times = {name: [] for name, _ in variants}
            for _ in range(args.repeats):
                for name, fn in variants[:2]:
                    times[name].append(window(fn, args.window))
            for _ in range(args.repeats):                    # (last: it empties the scene)
                times["Z_reset_scene"].append(window(ident.reset_scene, args.window))
            row = {"gt_rows": ident.gt_rows, "id_cap": ID_CAP, "max_rows": max_rows, "max_cols": max_cols, "active_rows": nr,
                   "active_cols": nc, "idtp": want}
            for name, _ in variants:
                row[name + "_ms"] = stats(times[name])
            record["close"].append(row)
            print(json.dumps(row), flush=True)
            dump()


if __name__ == "__main__":
    main()
