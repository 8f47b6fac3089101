#!/usr/bin/env python3
"""Times `ReIDNet.match_gallery` for the one-way matching heads (`concat`, `xcorr-baseline`, `xcorr`) over all pairs of
192 x 192 and 2048 x 2048 objects of 128 points.

concat (the embedding head, pcr_amd/pairs_head.py):
  G  the gallery route: pool_channel_max + the two per-object tables + pcr_pair_head_f32 over the whole list
  L  the pair launch alone, on tables made once
  Y  the yardstick: the same logits through the launches the library had before -- torch.cat([emb[i], emb[j]], 1) and the
     dense / GroupNorm launches of the head (_head_rows), in chunks of 262144 pairs so that the (P, 256) rows fit memory
xcorr-baseline / xcorr (192 x 192 only; informative): match_gallery beside the xcorr_eff model's match_gallery on the same
  objects.
Each eager and replayed from a captured graph; a variant that could not be run is recorded as "UNTIMED" with the reason.

Device events around windows of >= --window seconds after a warm-up; the variants of a shape alternate in one process,
--repeats windows each; median / min / max.  Fails without a GPU.

    python tools/bench_gallery_heads.py [--out profiles/<record>.json]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = ((192, 192), (2048, 2048))
N = 128
YARD_CHUNK = 262144

BASELINE = dict(
    type="ReIDNet", hidden_size=128, combine="cat", match_type="concat", output_sequence_size=64,
    backbone=dict(type="Pointnet_Backbone", input_channels=0, use_xyz=True, conv_out=64),
    backbone_list=[128, 64, 32], pool_type="max", downsample=None, cls_head=None, fp_head=None,
    match_head=[dict(type="LinearRes", n_in=256, n_out=256, norm="GN", ng=32),
                dict(type="Linear", in_features=256, out_features=1)],
    shape_head=None, cross_stage1=None, cross_stage2=None, local_stage1=None, local_stage2=None)
LOCAL = dict(type="local_self_attention", d_model=64, nhead=2, attention="linear", knum=48, pos_size=64)


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


def stats(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def captured(fn):
    """fn replayed from one graph, or the reason it could not be captured"""
    try:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        graph.replay()
        torch.cuda.synchronize()
        return graph.replay, None
    except Exception as e:      # noqa: BLE001  (recorded, not hidden: the variant is UNTIMED)
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def build(cfg):
    from mmdet3d.models import build_model
    from pcr_amd import testing as PT
    m = build_model(copy.deepcopy(cfg))
    m.load_state_dict(PT.seeded_state_dict(PT.manifest_of(m), 0), strict=True)
    return m.cuda().eval()


def encode(model, clouds):
    xyz, h = [], []
    for lo in range(0, clouds.shape[0], 256):
        x, f = model.forward_inference(clouds[lo:lo + 256].cuda())[:2]
        xyz.append(x), h.append(f)
    return torch.cat(xyz).contiguous(), torch.cat(h).contiguous()


def run_variants(variants, args):
    replays, why = {}, {}
    for name, fn in variants:
        fn()                                                    # warm: nothing is loaded inside a capture
        replays[name], why[name] = captured(fn)
    times = {name: ([], []) for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            times[name][0].append(window(fn, args.window))
            if replays[name] is not None:
                times[name][1].append(window(replays[name], args.window))
    ms = {name: {"eager": stats(times[name][0]),
                 "graph": stats(times[name][1]) if times[name][1] else "UNTIMED (%s)" % why[name]} for name, _ in variants}
    return ms, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gallery_heads: no GPU (this tool measures on the device only)")
    import bench
    from pcr_amd import pairs_head
    from pcr_amd import testing as PT
    concat = build(BASELINE)
    eff, _ = bench.build_pt_model([N, 64, 32])
    pt_cfg = copy.deepcopy(bench.PT_MODEL)
    pt_cfg["backbone_list"] = [N, 64, 32]
    stnet = build(dict(pt_cfg, match_type="xcorr-baseline"))
    orig = build(dict(pt_cfg, match_type="xcorr", local_stage1=dict(LOCAL), local_stage2=dict(LOCAL)))
    rows = []
    with torch.no_grad():
        cal = PT.synthetic_clouds(16, N, seed=1, kind="box").cuda()
        for m in (concat, eff, stnet, orig):
            m.calibrate_precision(cal[:8], cal[8:])
        for Q, G in SIZES:
            M = Q + G
            clouds = PT.synthetic_clouds(M, N, seed=G, kind="box")
            qi = torch.arange(Q, dtype=torch.int32, device="cuda").repeat_interleave(G)
            gi = torch.arange(G, dtype=torch.int32, device="cuda").repeat(Q) + Q
            pairs = torch.stack([qi, gi], dim=1).contiguous()
            P = pairs.shape[0]
            xyz, h = encode(concat, clouds)
            pl = pairs_head.plan(concat.match_head, h.device)
            emb = concat.embed(h)
            u, v = pairs_head.tables(pl, emb)
            out = torch.empty(P, dtype=torch.float32, device="cuda")

            def yardstick():
                parts = []
                for lo in range(0, P, YARD_CHUNK):
                    i, j = pairs[lo:lo + YARD_CHUNK, 0].long(), pairs[lo:lo + YARD_CHUNK, 1].long()
                    parts.append(concat._head_rows(torch.cat([emb[i], emb[j]], dim=1)))
                return torch.cat(parts)

            got, ref = concat.match_gallery(h, xyz, pairs), yardstick()
            dev = float((got - ref).abs().max())
            assert dev < 1e-4, dev                                  # the yardstick computes the same thing
            variants = [("G_match_gallery", lambda: concat.match_gallery(h, xyz, pairs)),
                        ("L_pair_launch", lambda: pairs_head.pair_logits(pl, emb, u, v, pairs, out=out)),
                        ("Y_cat_head_rows", yardstick)]
            ms, times = run_variants(variants, args)
            med = lambda name, k: float(np.median(times[name][k]))      # noqa: E731
            row = {"queries": Q, "gallery": G, "pairs": P, "points": N, "head": "concat",
                   "max_abs_gallery_minus_yardstick": dev, "ms": ms,
                   "gallery_over_yardstick": {"eager": round(med("G_match_gallery", 0) / med("Y_cat_head_rows", 0), 4)}}
            if times["G_match_gallery"][1] and times["Y_cat_head_rows"][1]:
                row["gallery_over_yardstick"]["graph"] = round(med("G_match_gallery", 1) / med("Y_cat_head_rows", 1), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if (Q, G) != SIZES[0]:
                continue
            # the attention heads beside xcorr_eff on the same objects (every model encodes them with its own weights)
            variants = []
            for name, m in (("xcorr_eff", eff), ("xcorr_baseline", stnet), ("xcorr", orig)):
                mx, mh = encode(m, clouds)
                variants.append((name, lambda m=m, mx=mx, mh=mh: m.match_gallery(mh, mx, pairs)))
            ms, _ = run_variants(variants, args)
            row = {"queries": Q, "gallery": G, "pairs": P, "points": N, "head": "attention heads (informative)", "ms": ms}
            rows.append(row)
            print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_gallery_heads.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0),
           "note": "ms per call, median / min / max of the repeated windows (device events), the variants of a shape "
                   "alternating in one process.  concat: G = match_gallery (pool_channel_max + the two tables + "
                   "pcr_pair_head_f32 over the whole list); L = the pair launch alone; Y = the yardstick, the same logits as "
                   "torch.cat([emb[i], emb[j]], 1) + the head's dense / GroupNorm launches in chunks of 262144 pairs, default "
                   "precision mode.  gallery_over_yardstick = G / Y (below 1: the new route is faster).  attention heads: "
                   "match_gallery of the xcorr_eff, xcorr-baseline and xcorr models over all pairs (seeded weights, each "
                   "model's own features); eager = the Python calls, graph = one captured graph replayed",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
