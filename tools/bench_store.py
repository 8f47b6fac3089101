#!/usr/bin/env python3
"""Times the data path of training at the config-4 shape (256 pairs of 128 points) from a synthetic crop directory written
to a temporary directory (300 objects, 3-8 observations each, 3-400 points):

  H   the host path: one `loader.EpochLoader` batch (`TrainPairs.__getitem__` file reads + `subsample_pc`) and
      `data.collate_pairs` to the device, host clock, ending with a device synchronisation
  D   the device path: one `store.DeviceEpochLoader` batch (`CropStore.train_batch`: the pair rule and the gather), device
      events; eager, and replayed from a HIP graph
  S   the training step the batches feed (`Trainer.step` on one fixed batch, graph mode), device events
  run_epochs iterations per second with either loader in front of the same trainer (host clock around whole epochs)

--repeats windows each after a warm-up, the sides alternating in one process; median / min / max.  Fails without a GPU.

    python tools/bench_store.py [--out profiles/<record>.json]      (default: profiles/store_bench.json)
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "point-cloud-reid_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PAIRS, POINTS, OBJECTS = 256, 128, 300


def write_crops(root, seed=0):
    g = np.random.default_rng(seed)
    meta = {}
    for i in range(OBJECTS):
        fp = i % 5 == 4
        tok = ("FP_%03d" if fp else "obj_%03d") % i
        meta[tok] = dict(cls=i % 3, fp=fp)
        for obs in range(int(g.integers(3, 9))):
            d = os.path.join(root, tok, str(obs))
            os.makedirs(d)
            n = int(g.integers(3, 401))
            (g.standard_normal((n, 3)).astype(np.float32) + i).tofile(os.path.join(d, "pts_xyz.bin"))
    return meta


class SparseOnly:
    """a TrainPairs whose items carry no dense cloud, so that `collate_pairs` lets the sparse one stand in: the same batch
    layout as the device path's"""

    def __init__(self, ds):
        self.ds, self.flag = ds, ds.flag

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        it = self.ds[i]
        del it["dense_1"], it["dense_2"]
        return it


def stats(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def device_window(fn, seconds):
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


def host_window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_store: no GPU (this tool measures on the device only)")
    import bench
    from pcr_amd import loader as LD, store as ST, train
    with tempfile.TemporaryDirectory() as root:
        meta = write_crops(root)
        crops = LD.CropDirectory(root)
        table = crops.table(meta, num_classes=3)
        np.random.seed(0)
        ds = LD.TrainPairs(table, crops.read, subsample_sparse=POINTS)
        t0 = time.perf_counter()
        store = ST.CropStore.from_directory(root, table, device="cuda")
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        host = LD.EpochLoader(SparseOnly(ds), PAIRS, seed=0, device="cuda")
        devl = ST.DeviceEpochLoader(store, ds, PAIRS, seed=0)

        # one batch
        def fh():
            return next(iter(host.epoch(0)))
        order = torch.as_tensor(np.arange(PAIRS) % len(ds), dtype=torch.int32).cuda()
        items = torch.as_tensor(ds.idx[np.arange(PAIRS) % len(ds)].astype(np.int32)).cuda()
        seed = torch.zeros(1, dtype=torch.int64, device="cuda")

        def fd():
            return store.train_batch(items, order, seed, n=POINTS)
        fd()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = fd()

        def fg():
            seed.add_(1)
            graph.replay()
        # the step the batches feed
        model, _ = bench.build_pt_model([128, 64, 32])
        model.train()
        tr = train.Trainer(model, max_iters=10 ** 6, lr=1e-4, grad_clip=1.0, graph=True)
        fixed = fd()
        for _ in range(6):
            tr.step(fixed)

        def fs():
            tr.step(fixed)
        for f in (fh, fd, fg, fs):
            f()
        th, td, tg, ts = [], [], [], []
        for _ in range(args.repeats):
            th.append(host_window(fh, 3))
            td.append(device_window(fd, args.window))
            tg.append(device_window(fg, args.window))
            ts.append(device_window(fs, args.window))
        assert store.flags() & ~ST.INFO_RETRY == 0 and len(captured["sparse_1"]) == PAIRS

        # whole epochs in front of the same trainer
        rate = {}
        for name, ld in (("host", host), ("device", devl)):
            LD.run_epochs(tr, ld, 2)
            torch.cuda.synchronize()
            rs = []
            for r in range(3):
                t0 = time.perf_counter()
                out = LD.run_epochs(tr, ld, args.epochs, start_epoch=10 * r)
                torch.cuda.synchronize()
                rs.append(len(out) / (time.perf_counter() - t0))
            rate[name] = stats(rs)
        rec = {"tool": "tools/bench_store.py", "device": torch.cuda.get_device_name(0), "pairs": PAIRS, "points": POINTS,
               "objects": OBJECTS, "items": len(ds), "crops": store.num_rows, "store_bytes": store.nbytes,
               "store_load_s": round(t_load, 3), "window_s": args.window, "repeats": args.repeats,
               "H_host_batch_to_device_ms": stats(th), "D_device_batch_eager_ms": stats(td),
               "D_device_batch_graph_ms": stats(tg), "S_train_step_graph_ms": stats(ts),
               "run_epochs_it_per_s": rate, "batches_per_epoch": len(devl), "epochs_per_window": args.epochs,
               "note": "H: EpochLoader batch + collate_pairs to the device, host clock, page cache warm; D: "
                       "CropStore.train_batch (pair rule + gather + the int64 view of labels and ids), device events; S: "
                       "Trainer.step (graph mode) on a fixed batch; run_epochs: iterations per second of whole epochs, host "
                       "clock, the same trainer behind either loader"}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
