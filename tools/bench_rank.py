#!/usr/bin/env python3
"""Times the ranking of a gallery on the device (include/pcr.h section A8, pcr_amd/retrieval.py) against a torch
restatement of the same step, and what share of `ReIDNet.retrieve` the ranking is.  Q x G of 192 x 192 (the `gallery128`
shape) and 2048 x 2048, K = 10; objects in 4 classes, so three quarters of a score row are -inf, and a handful of true
candidates per query.

  S  score_matrix + rank_gallery + RankBook.add: the three launches an evaluation adds per chunk of queries
  R  rank_gallery alone, on the same score matrix
  T  the torch restatement of R on the same score matrix: torch.topk for the top-k, comparisons for the candidates, the
     true set and the first hit, and a stable descending sort + cumulative sum for the average precision
  t  T without the average precision (no sort): top-k and first hit only
  W  `ReIDNet.retrieve` as a whole over (64, 128) features of the toy Point-Transformer: compare_pairs, match_gallery
     (live_only), score_matrix, rank_gallery
  each eager and replayed from a captured graph; a variant that could not be run is recorded as "UNTIMED" with the reason

Device events around windows of >= --window seconds after a warm-up; the variants of a shape alternate in one process,
--repeats windows each; median / min / max.  Fails without a GPU.

    python tools/bench_rank.py [--out profiles/<record>.json]
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

SIZES = ((192, 192), (2048, 2048))
N, K, CLASSES, RANKS = 128, 10, 4, (1, 5, 10)


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


def torch_rank(scores, qids, gids, k, with_ap=True):
    """the ranking step in torch ops (ties are torch's, not the library's rule: a yardstick, not a reference)"""
    neg = float("-inf")
    cand = scores != neg
    n_cand = cand.sum(dim=1)
    top = torch.topk(scores, k, dim=1)
    truth = cand & (qids[:, None] == gids[None, :]) & (qids[:, None] >= 0)
    n_true = truth.sum(dim=1)
    best = torch.where(truth, scores, scores.new_full((), neg)).amax(dim=1)
    first = torch.where(n_true > 0, (scores > best[:, None]).sum(dim=1), n_true.new_full((), -1))
    if not with_ap:
        return top.indices, top.values, n_cand, n_true, first
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    hits = truth.gather(1, order).to(torch.float64)
    prec = hits.cumsum(dim=1) / torch.arange(1, scores.shape[1] + 1, device=scores.device, dtype=torch.float64)
    ap = ((prec * hits).sum(dim=1) / n_true.clamp(min=1)).to(torch.float32)
    return top.indices, top.values, n_cand, n_true, first, ap


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank: no GPU (this tool measures on the device only)")
    import bench
    from pcr_amd import associate as A
    from pcr_amd import retrieval as RT
    from pcr_amd import testing as PT
    model, _ = bench.build_pt_model([N, 64, 32])
    rows = []
    with torch.no_grad():
        cal = PT.synthetic_clouds(16, N, seed=1, kind="box").cuda()
        model.calibrate_precision(cal[:8], cal[8:])
        for Q, G in SIZES:
            g = np.random.default_rng(Q)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
            q_cls, g_cls = dev((np.arange(Q) % CLASSES).astype(np.int32)), dev((np.arange(G) % CLASSES).astype(np.int32))
            q_ids = dev((np.arange(Q) % max(G // 8, 1)).astype(np.int32))          # about eight gallery entries per identity,
            g_ids = dev((g.permutation(G) % max(G // 8, 1)).astype(np.int32))      # a quarter of them in the query's class
            pairs, count = A.compare_pairs(q_cls, g_cls, num_classes=CLASSES)
            logits = dev(g.standard_normal(Q * G).astype(np.float32))
            scores, out, book = torch.empty((Q, G), device="cuda"), RT.rank_buffers(Q, K, "cuda"), RT.RankBook(RANKS, "cuda")

            def launches():
                RT.score_matrix(logits, pairs, count, Q, G, out=scores)
                book.add(RT.rank_gallery(scores, q_ids, g_ids, topk=K, out=out), gallery=G)

            launches()
            ours = {k: v.clone() for k, v in out.items()}
            ref = torch_rank(scores, q_ids, g_ids, K)
            # the yardstick computes the same thing (random scores: no ties among the candidates)
            assert torch.equal(ours["topk_idx"].long(), ref[0]) and torch.equal(ours["n_true"].long(), ref[3])
            assert torch.equal(ours["first_hit"].long(), ref[4]) and float((ours["ap"] - ref[5]).abs().max()) < 1e-6
            xyz, h = [], []
            clouds = PT.synthetic_clouds(Q + G, N, seed=G, kind="box")
            for lo in range(0, Q + G, 256):
                x, f = model.forward_inference(clouds[lo:lo + 256].cuda())[:2]
                xyz.append(x), h.append(f)
            xyz, h = torch.cat(xyz).contiguous(), torch.cat(h).contiguous()

            def whole():
                return model.retrieve(h[:Q], xyz[:Q], q_cls, None, h[Q:], xyz[Q:], g_cls, None, query_ids=q_ids,
                                      gallery_ids=g_ids, topk=K, num_classes=CLASSES, live_only=True)

            variants = [("S_scatter_rank_accumulate", launches),
                        ("R_rank_gallery", lambda: RT.rank_gallery(scores, q_ids, g_ids, topk=K, out=out)),
                        ("T_torch_topk_sort_ap", lambda: torch_rank(scores, q_ids, g_ids, K)),
                        ("t_torch_topk_first_hit", lambda: torch_rank(scores, q_ids, g_ids, K, with_ap=False)),
                        ("W_retrieve", whole)]
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
            row = {"queries": Q, "gallery": G, "topk": K, "classes": CLASSES, "live_pairs": int(count[0]), "ms": {}}
            for name, _ in variants:
                row["ms"][name] = {"eager": stats(times[name][0]),
                                   "graph": stats(times[name][1]) if times[name][1] else "UNTIMED (%s)" % why[name]}
            med = lambda name, i: float(np.median(times[name][i]))      # noqa: E731
            row["rank_over_torch"] = {"eager": round(med("R_rank_gallery", 0) / med("T_torch_topk_sort_ap", 0), 4)}
            if times["R_rank_gallery"][1] and times["T_torch_topk_sort_ap"][1]:
                row["rank_over_torch"]["graph"] = round(med("R_rank_gallery", 1) / med("T_torch_topk_sort_ap", 1), 4)
            row["ranking_share_of_retrieve"] = {"eager": round(med("S_scatter_rank_accumulate", 0) / med("W_retrieve", 0), 5)}
            if times["W_retrieve"][1]:
                row["ranking_share_of_retrieve"]["graph"] = round(med("S_scatter_rank_accumulate", 1) / med("W_retrieve", 1), 5)
            rows.append(row)
            print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_rank.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "precision": model.precision_level(),
           "note": "ms per call, median / min / max of the repeated windows (device events), the variants of a shape "
                   "alternating in one process.  S = score_matrix + rank_gallery + RankBook.add; R = rank_gallery alone; T = "
                   "the torch restatement of R (torch.topk, comparisons, a stable sort and a cumulative sum for the "
                   "average precision) on the same score matrix; t = T without the average precision; W = "
                   "ReIDNet.retrieve as a whole (compare_pairs, match_gallery with live_only over 128-point features of "
                   "the toy Point-Transformer, score_matrix, rank_gallery).  eager = the Python calls, graph = one "
                   "captured graph replayed.  rank_over_torch = R / T (below 1: the launch is faster); "
                   "ranking_share_of_retrieve = S / W (S holds the accumulate launch, W does not: an upper bound).  "
                   "Objects in 4 classes: a quarter of a score row are candidates",
           "shapes": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
