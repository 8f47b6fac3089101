#!/usr/bin/env python3
"""Times the scoring of a validation split with and without a device-side book (pcr_amd/matchbook.py) on the synthetic crop
directory of tools/bench_store.py (300 objects, 3-8 observations each), the batches coming from one `CropStore` on either
route, at 256 and at 512 pairs of 128 points per batch:

  F   the whole split: `evaluate.evaluate_model(.., store=)` -- forward_test per batch, the per-pair columns kept, gathered
      and scored on the host: the yardstick -- against the same call with `book=` (validate_step per batch, one table read
      at the end); host clock around the whole call, ending with a device synchronisation, in one process, the two routes
      alternating
  B   one batch: `ReIDNet.validate_step` eager (host clock, synchronised) and replayed from a HIP graph (device events), and
      next to it the existing route's encode + match half of the same batch (`siamese_forward` + `match_forward_inference`,
      eager, host clock): what the step adds to it is the batch's bookkeeping and the one record launch

--repeats windows each after a warm-up; median / min / max.  No ratio is asserted.  Fails without a GPU.

    python tools/bench_validate.py [--out profiles/<record>.json]      (default: profiles/validate_bench.json)
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

POINTS, BATCHES = 128, (256, 512)


def host_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def calls_for(seconds, one_ms):
    """calls that fill a window of `seconds` when one takes one_ms"""
    return max(3, int(np.ceil(seconds * 1e3 / max(one_ms, 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-combinations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validate: no GPU (this tool measures on the device only)")
    import bench
    import bench_store as BS
    from pcr_amd import evaluate as EV, loader as LD, matchbook as MB, pairs as PR, store as ST
    with tempfile.TemporaryDirectory() as root:
        meta = BS.write_crops(root)
        crops = LD.CropDirectory(root)
        table = crops.table(meta, num_classes=3)
        pos, neg = PR.build_val_pairs(table, args.max_combinations, seed=0)
        ds = LD.ValPairs(table, pos, neg, crops.read, POINTS, 8, read_dense=lambda tok: np.zeros((3, 8)), visibility={})
        store = ST.CropStore.from_directory(root, table, device="cuda")
        model, _ = bench.build_pt_model([POINTS, 64, 32])
        book = MB.MatchBook("cuda")
        kw = dict(seed=0, rank=0, world=1, cls_to_idx={"a": 0, "b": 1, "c": 2}, num_classes=3, store=store)
        rec = {"tool": "tools/bench_validate.py", "device": torch.cuda.get_device_name(0), "points": POINTS,
               "objects": BS.OBJECTS, "pairs_in_split": len(ds), "window_s": args.window, "repeats": args.repeats}
        for bs in BATCHES:
            def full_host():
                return EV.evaluate_model(model, ds, bs, **kw)

            def full_book():
                return EV.evaluate_model(model, ds, bs, book=book, **kw)
            a, b = full_host(), full_book()                  # the warm-up, and the two routes agree before they are timed
            assert a["num_pairs"] == b["num_pairs"] == len(ds)
            x = a["logits"]
            if not bool(((x > 0) & (x <= 1e-6)).any()):       # (outside that interval the two decision rules are one)
                assert a["val_match_acc"] == b["val_match_acc"], (a["val_match_acc"], b["val_match_acc"])
            th, tb = [], []
            calls_f = calls_for(args.window, host_ms(full_host, 1))
            for _ in range(args.repeats):
                th.append(host_ms(full_host, calls_f))
                tb.append(host_ms(full_book, calls_f))

            # one batch of bs pairs
            batch = store.val_batch(0, min(bs, len(ds)), 0, n=POINTS)
            if len(batch["sparse_1"]) < bs:
                batch = EV._padded(batch, bs)
            held = {k: torch.stack(v).clone() for k, v in batch.items()}
            views = {k: list(t.unbind(0)) for k, t in held.items()}
            s1, s2 = held["sparse_1"], held["sparse_2"]
            one = MB.MatchBook("cuda")
            count = torch.tensor([bs], dtype=torch.int32, device="cuda")

            def step():
                model.validate_step(views, one, count)

            def half():
                return bench.hot_path(model, s1, s2)
            with torch.no_grad():
                step(), half()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step()
                calls = calls_for(args.window, host_ms(step, 3))
                te, tg, tm = [], [], []
                for _ in range(args.repeats):
                    te.append(host_ms(step, calls))
                    tg.append(BS.device_window(graph.replay, args.window))
                    tm.append(host_ms(half, calls))
            rec["batch_%d" % bs] = {
                "batches_in_split": -(-len(ds) // bs),
                "F_full_split_host_route_ms": BS.stats(th), "F_full_split_book_ms": BS.stats(tb),
                "B_validate_step_eager_ms": BS.stats(te), "B_validate_step_graph_ms": BS.stats(tg),
                "B_encode_match_half_eager_ms": BS.stats(tm)}
        rec["note"] = ("F: evaluate_model over the whole split with store=, host clock around the call, synchronised; the host "
                       "route keeps, gathers and scores per-pair columns on the CPU, the book route reads one table.  B: one "
                       "batch; eager rows are host clock, synchronised, the graph row device events.  Every window holds as "
                       "many calls as fill window_s.")
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
