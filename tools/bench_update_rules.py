#!/usr/bin/env python3
"""Times the update of the track bank under the reference's update_config against the one-flag update it stands beside
(pcr_amd/tracks.py), and a whole tracker frame with and without it:

  bank   a scripted 12-frame scene from an empty bank (the reset is included on both sides), at a capacity of 40 tracks
         with 30 detections and of 200 with 100, feature rows (64, 128):
           plan        pcr_bank_plan_i32 + pcr_bank_move_f32 (TrackBank.update; born / kill = the masks of the scene's
                       det_newborn / track_false_positive decisions)
           rules       pcr_bank_plan_rules_i32 + pcr_bank_move_f32 + pcr_scene_log_append_i32 (TrackBank.update_rules +
                       SceneLog.append) on the same frames and decisions
  frame  ReIDNet.track_step(decisions=(2, 1)) on the toy Point-Transformer (capacity 16, 8 detection rows, 6 boxes of 148
         points), the same frame over and over, without and with update_config= + log=

Each one eager (E) and replayed from a captured graph (G).  ms per frame from device events around windows of >= --window
seconds; all series alternate in one process, --repeats windows each; min, median and max of the windows are reported.
The yardstick is the existing route timed in the same process.  Before timing, the rules route's final state is compared
with the restatement's.  Fails without a GPU.

    python tools/bench_update_rules.py [--out profiles/<record>.json]
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
FEAT, W, LIMIT, FRAMES = (64, 128), 9, 3, 12
CONFIG = dict(match=dict(output=True, active=True, decom=False), det_newborn=dict(output=True, active=True, decom=False),
              det_false_positive=dict(output=False, active=False, decom=True),
              track_false_positive=dict(output=False, active=False, decom=True),
              track_false_negative=dict(output=True, active=True, decom=False))


def window(fn, seconds, per=1):
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


def summary(t):
    return {"min": round(min(t), 4), "median": round(float(np.median(t)), 4), "max": round(max(t), 4)}


def measure(series, args, per):
    """{name: fn} -> {name_E_ms, name_G_ms}: every fn eager and replayed from its own graph, alternating"""
    graphs = {}
    for name, fn in series.items():
        fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            fn()
    times = {(name, mode): [] for name in series for mode in "EG"}
    for _ in range(args.repeats):
        for name, fn in series.items():
            times[(name, "E")].append(window(fn, args.window, per))
            times[(name, "G")].append(window(graphs[name].replay, args.window, per))
    return {"%s_%s_ms" % k: summary(t) for k, t in times.items()}


def bank_rows(args):
    import track_ref as R
    import update_ref as U
    from pcr_amd import tracks as T
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rules_h = U.rules_from_config(CONFIG, ["det_false_positive", "det_newborn"], ["track_false_negative", "track_false_positive"])
    rules = T.UpdateRules(CONFIG, ["det_false_positive", "det_newborn"], ["track_false_negative", "track_false_positive"])
    rows = []
    for C, D in SIZES:
        g = np.random.default_rng([C, D])
        st = R.new_state(C, W)
        frames = []
        for f in range(FRAMES):                                      # the script, driven by the restatement
            fr = U.make_frame(g, st, D, W, 2, 2, junk=False, p_valid=0.9)
            carry = R.rigid(g, span=1.0)[0]
            st = U.plan_frame(st, fr, rules_h, carry=carry, frame_limit=LIMIT)[0]
            d = {k: dev(fr[k]) for k in ("track_to_det", "det_to_track", "labels", "lengths", "boxes", "scores",
                                         "det_decision", "track_decision")}
            d.update(carry=dev(carry), born=dev((fr["det_decision"] == 2).astype(np.int32)),
                     kill=dev((fr["track_decision"] == 2).astype(np.int32)),
                     feats=torch.randn((D,) + FEAT, device="cuda"), xyz=torch.randn((D, FEAT[1], 3), device="cuda"))
            frames.append(d)
        bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)
        log = T.SceneLog(FRAMES * (C + D), C + D, W)

        def plan():
            bank.reset()
            for fr in frames:
                bank.update((fr["track_to_det"], fr["det_to_track"]), fr, born=fr["born"], kill=fr["kill"], carry=fr["carry"],
                            frame_limit=LIMIT)

        def with_rules():
            bank.reset()
            log.reset()
            for fr in frames:
                table = bank.update_rules((fr["track_to_det"], fr["det_to_track"]), fr, fr["det_decision"],
                                          fr["track_decision"], rules, carry=fr["carry"], frame_limit=LIMIT)[3]
                log.append(table)

        with_rules()
        torch.cuda.synchronize()
        for k in R.STATE:
            assert np.array_equal(getattr(bank, k).cpu().numpy(), st[k]), "the device's state differs: %s" % k
        row = {"capacity": C, "detections": D, "frames": FRAMES, "logged_rows": log.records()["id"].shape[0]}
        row.update(measure({"plan": plan, "rules": with_rules}, args, FRAMES))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def frame_row(args):
    import bench
    from pcr_amd import tracks as T
    from test_gpu_tracks import toy_frames
    C, D, M, n = 16, 8, 6, 128
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    model, _ = bench.build_pt_model([n, 64, 32])
    pts, boxes, labels, scores = (dev(x) for x in toy_frames(1, M, n + 20, W, seed=31)[0])
    banks = [T.TrackBank(C, D, feat_shape=(64, n), box_width=W) for _ in range(2)]
    log = T.SceneLog(1 << 20, C + D, W)
    det = dev(np.array([[7.0] * M, [6.0] * M], np.float32))
    trk = dev(np.full((1, C), 8.0, np.float32))
    decisions = dict(detection=("det_newborn", "det_false_positive"), tracking=("track_false_negative",), det_values=det,
                     track_values=trk)
    with torch.no_grad():
        c0 = model.forward_inference_boxes(pts, torch.cat([boxes, boxes.new_zeros((D - M, W))])[:, :7].contiguous(), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])
        plain = lambda: model.track_step(banks[0], pts, boxes, labels, scores, crop_args=dict(seed=5), frame_limit=LIMIT,
                                         decisions=dict(decisions))
        ruled = lambda: model.track_step(banks[1], pts, boxes, labels, scores, crop_args=dict(seed=5), frame_limit=LIMIT,
                                         decisions=dict(decisions), update_config=CONFIG, log=log)
        row = {"capacity": C, "detection_rows": D, "boxes": M, "points": n + 20}
        row.update(measure({"frame": plain, "frame_rules_log": ruled}, args, 1))
    rec = log.records()
    row["log_rows"], row["log_dropped"] = int(rec["id"].shape[0]), rec["dropped"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_update_rules: no GPU (this tool measures on the device only)")
    rec = {"tool": "tools/bench_update_rules.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0),
           "note": "bank: plan = TrackBank.update, rules = TrackBank.update_rules + SceneLog.append, a scripted 12-frame scene "
                   "from an empty bank, reset included.  frame: ReIDNet.track_step(decisions=(2, 1)) on the toy model, "
                   "frame_rules_log with update_config= and log=.  _E_ eager, _G_ replayed from a captured graph.  ms per "
                   "frame (device events), min / median / max of the repeated windows, all series alternating in one process",
           "bank": bank_rows(args), "frame": frame_row(args)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
