#!/usr/bin/env python3
"""Times the ranking of a wide gallery on the device (include/pcr.h section A12, pcr_amd/retrieval.py): against the narrow
kernel at the width both cover, against a torch restatement above it, and as a share of `ReIDNet.retrieve_wide`.  Q = 64
queries, K = 10, every gallery entry a candidate, scores a random permutation per row (no ties: the yardsticks can be held
to the same answer).

  narrow  G = 4096, one true candidate per query:
            N  rank_gallery (one wave per query, the row in LDS)
            X  rank_gallery_wide on the same score matrix
  torch   G = 16384, 65536, 262144, with 1 and with 64 true candidates per query:
            X  rank_gallery_wide
            T  the torch restatement tools/bench_rank.py uses (torch.topk, comparisons, a stable sort and a cumulative sum)
  share   G = 16384 over (64, 128) features of the toy Point-Transformer, objects in 4 classes, gallery blocks of 4096:
            W  retrieve_wide as a whole (fill_scores; per block compare_pairs, match_gallery with live_only, scatter_scores;
               rank_gallery_wide)
            S  its ranking part alone: fill_scores + the four scatter_scores + rank_gallery_wide over kept pair lists
  each eager and replayed from a captured graph, T eager only; a variant that was not run is recorded as "UNTIMED" with the
  reason

Device events around windows of >= --window seconds after a warm-up; the variants of a shape alternate in one process,
--repeats windows each; median / min / max.  Fails without a GPU.

    python tools/bench_rank_wide.py [--out profiles/<record>.json]
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

from bench_rank import captured, stats, torch_rank, window  # noqa: E402

Q, K, N, CLASSES, BLOCK = 64, 10, 128, 4, 4096
NARROW_G, TORCH_G, TORCH_TRUE, SHARE_G = 4096, (16384, 65536, 262144), (1, 64), 16384
# the torch yardstick is timed eagerly only: at these widths torch.sort and torch.topk leave the in-block kernels that
# tools/bench_rank.py captures at 2048 entries, and a replay of their captured graph is not relied on here
EAGER_ONLY = {"T_torch_topk_sort_ap": "not captured: rows above 4096 entries"}


def timed(variants, args):
    """{name: {"eager": stats, "graph": stats or "UNTIMED (...)"}} and the medians, the variants alternating"""
    replays, why = {}, {}
    for name, fn in variants:
        fn()                                                        # warm: nothing is loaded inside a capture
        replays[name], why[name] = captured(fn) if name not in EAGER_ONLY else (None, EAGER_ONLY[name])
    times = {name: ([], []) for name, _ in variants}
    for i in range(args.repeats):
        for name, fn in variants:
            print("# window %d: %s" % (i, name), file=sys.stderr, flush=True)
            times[name][0].append(window(fn, args.window))
            if replays[name] is not None:
                times[name][1].append(window(replays[name], args.window))
    ms = {name: {"eager": stats(times[name][0]),
                 "graph": stats(times[name][1]) if times[name][1] else "UNTIMED (%s)" % why[name]} for name, _ in variants}
    med = lambda name, i: float(np.median(times[name][i])) if times[name][i] else None      # noqa: E731
    return ms, med


def ratio(med, a, b):
    out = {"eager": round(med(a, 0) / med(b, 0), 4)}
    if med(a, 1) is not None and med(b, 1) is not None:
        out["graph"] = round(med(a, 1) / med(b, 1), 4)
    return out


def rows_of(G, n_true, seed):
    """scores (Q, G): a random permutation of G distinct values per row; ids with n_true gallery entries per query"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    scores = (torch.argsort(torch.rand((Q, G), device="cuda", generator=gen), dim=1).float() / 16).contiguous()
    g = np.random.default_rng(seed)
    groups = G // n_true
    g_ids = torch.from_numpy((g.permutation(G) % groups).astype(np.int32)).cuda()
    q_ids = torch.from_numpy(g.permutation(groups)[:Q].astype(np.int32)).cuda()
    return scores, q_ids, g_ids


def same_answer(ours, ref):
    assert torch.equal(ours["topk_idx"].long(), ref[0]) and torch.equal(ours["n_true"].long(), ref[3])
    assert torch.equal(ours["first_hit"].long(), ref[4]) and float((ours["ap"] - ref[5]).abs().max()) < 1e-6
    assert not bool(ours["info"].any())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_wide: no GPU (this tool measures on the device only)")
    import bench
    from pcr_amd import associate as A
    from pcr_amd import frame
    from pcr_amd import retrieval as RT
    from pcr_amd import testing as PT
    rec = {"tool": "tools/bench_rank_wide.py", "window_s": args.window, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "queries": Q, "topk": K}
    with torch.no_grad():
        # ---- wide against narrow ---------------------------------------------------------------------------------------------
        scores, q_ids, g_ids = rows_of(NARROW_G, 1, 1)
        out_n, out_x = RT.rank_buffers(Q, K, "cuda"), RT.rank_buffers(Q, K, "cuda")
        variants = [("N_rank_gallery", lambda: RT.rank_gallery(scores, q_ids, g_ids, topk=K, out=out_n)),
                    ("X_rank_gallery_wide", lambda: RT.rank_gallery_wide(scores, q_ids, g_ids, topk=K, out=out_x))]
        for _, fn in variants:
            fn()
        assert all(torch.equal(out_n[k], out_x[k]) for k in RT.OUTPUTS)
        same_answer(out_x, torch_rank(scores, q_ids, g_ids, K))
        ms, med = timed(variants, args)
        rec["narrow"] = {"gallery": NARROW_G, "true_per_query": 1, "ms": ms,
                         "wide_over_narrow": ratio(med, "X_rank_gallery_wide", "N_rank_gallery")}
        print(json.dumps(rec["narrow"]), flush=True)
        # ---- wide against torch ----------------------------------------------------------------------------------------------
        rec["torch"] = []
        for G in TORCH_G:
            for n_true in TORCH_TRUE:
                scores, q_ids, g_ids = rows_of(G, n_true, G + n_true)
                out_x = RT.rank_buffers(Q, K, "cuda")
                variants = [("X_rank_gallery_wide", lambda: RT.rank_gallery_wide(scores, q_ids, g_ids, topk=K, out=out_x)),
                            ("T_torch_topk_sort_ap", lambda: torch_rank(scores, q_ids, g_ids, K))]
                variants[0][1]()
                same_answer(out_x, torch_rank(scores, q_ids, g_ids, K))
                assert bool((out_x["n_true"] == n_true).all())
                ms, med = timed(variants, args)
                row = {"gallery": G, "true_per_query": n_true, "ms": ms,
                       "wide_over_torch": ratio(med, "X_rank_gallery_wide", "T_torch_topk_sort_ap")}
                rec["torch"].append(row)
                print(json.dumps(row), flush=True)
        # ---- share of an evaluation chunk ------------------------------------------------------------------------------------
        G = SHARE_G
        model, _ = bench.build_pt_model([N, 64, 32])
        cal = PT.synthetic_clouds(16, N, seed=1, kind="box").cuda()
        model.calibrate_precision(cal[:8], cal[8:])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        g = np.random.default_rng(G)
        q_cls, g_cls = dev((np.arange(Q) % CLASSES).astype(np.int32)), dev((np.arange(G) % CLASSES).astype(np.int32))
        q_ids, g_ids = dev(np.arange(Q, dtype=np.int32)), dev(g.permutation(G).astype(np.int32))     # one true candidate each
        xyz, h = [], []
        clouds = PT.synthetic_clouds(Q + G, N, seed=G, kind="box")
        for lo in range(0, Q + G, 256):
            x, f = model.forward_inference(clouds[lo:lo + 256].cuda())[:2]
            xyz.append(x), h.append(f)
        xyz, h = torch.cat(xyz).contiguous(), torch.cat(h).contiguous()
        scores, out_x = torch.empty((Q, G), device="cuda"), RT.rank_buffers(Q, K, "cuda")

        def whole():
            return model.retrieve_wide(h[:Q], xyz[:Q], q_cls, None, h[Q:], xyz[Q:], g_cls, None, query_ids=q_ids,
                                       gallery_ids=g_ids, topk=K, num_classes=CLASSES, live_only=True, gallery_block=BLOCK,
                                       scores=scores)
        res = whole()
        live = int(res["counts"].sum())
        kept = []
        for lo in range(0, G, BLOCK):                                   # the pair lists and logits retrieve_wide does not keep
            pairs, count = A.compare_pairs(q_cls, g_cls[lo:lo + BLOCK], num_classes=CLASSES)
            logits = frame.match_across(model, torch.cat([h[:Q], h[Q + lo:Q + lo + BLOCK]]),
                                        torch.cat([xyz[:Q], xyz[Q + lo:Q + lo + BLOCK]]), pairs, Q, count)
            kept.append((logits, pairs, count, lo, min(BLOCK, G - lo)))
        check = torch.empty_like(scores)

        def ranking():
            RT.fill_scores(check)
            for logits, pairs, count, lo, width in kept:
                RT.scatter_scores(logits, pairs, count, check, lo, width)
            return RT.rank_gallery_wide(check, q_ids, g_ids, topk=K, out=out_x)
        ranking()
        assert torch.equal(check, res["scores"]) and all(torch.equal(out_x[k], res[k]) for k in RT.OUTPUTS)
        ms, med = timed([("S_fill_scatter_rank", ranking), ("W_retrieve_wide", whole)], args)
        rec["share"] = {"gallery": G, "gallery_block": BLOCK, "classes": CLASSES, "live_pairs": live, "ms": ms,
                        "precision": model.precision_level(),
                        "ranking_share_of_retrieve_wide": ratio(med, "S_fill_scatter_rank", "W_retrieve_wide")}
        print(json.dumps(rec["share"]), flush=True)
    rec["note"] = ("ms per call, median / min / max of the repeated windows (device events), the variants of a shape "
                   "alternating in one process; eager = the Python calls, graph = one captured graph replayed.  Q = 64, K = "
                   "10, every gallery entry a candidate, a random permutation of distinct scores per row.  narrow: N = "
                   "rank_gallery, X = rank_gallery_wide on the same (64, 4096) matrix, one true candidate per query; "
                   "wide_over_narrow = X / N.  torch: X against T = the torch restatement of tools/bench_rank.py (torch.topk, "
                   "comparisons, a stable sort and a cumulative sum); wide_over_torch = X / T (below 1: the launch is "
                   "faster).  share: W = ReIDNet.retrieve_wide over 128-point features of the toy Point-Transformer "
                   "(live_only, objects in 4 classes, gallery blocks of 4096), S = fill_scores + the scatter_scores + "
                   "rank_gallery_wide alone; ranking_share_of_retrieve_wide = S / W")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
