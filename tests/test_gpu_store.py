"""GPU: the device crop store (pcr_amd/store.py, include/pcr.h section A6, csrc/store_kernels.hip).  Both launches equal
their numpy restatement (tests/store_ref.py) bit for bit; on crops that need no resampling a device batch equals
`collate_pairs` of the host items tensor for tensor, trains to the same loss bits and evaluates to the same logits; the
samples of a pair do not depend on the batch size or the shard; a captured batch draws fresh samples from a new seed."""
import os

import numpy as np
import pytest
import torch

import store_ref as SR
from pcr_amd import _lib as L
from pcr_amd import data as D
from pcr_amd import loader as LD
from pcr_amd import pairs as PR
from pcr_amd import store as ST
from test_loader import make_crops
from test_store_cpu import hand_table, rows_of

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def i32(a):
    return dev(np.asarray(a).astype(np.int32))


# ---- the gather ----
def raw_gather(points, offsets, rows, n, keys=None, rand=None, seed=None):
    """pcr_store_gather_f32 on the caller's own buffers -> clouds, sizes, info (numpy)"""
    B = len(rows)
    clouds = torch.full((B, n, 3), float("nan"), device=DEV)
    sizes = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    seed_t = None if seed is None else torch.tensor([seed], dtype=torch.int64, device=DEV)
    L.run.pcr_store_gather_f32(points, L.ptr(offsets), offsets.numel() - 1, i32(rows), None if keys is None else i32(keys),
                               None if rand is None else dev(rand.view(np.int32)), L.ptr(seed_t), clouds, sizes, info, B, n,
                               L.stream_ptr())
    return clouds.cpu().numpy(), sizes.cpu().numpy(), int(info.item())


@pytest.mark.parametrize("n", [1, 100, 128])
def test_gather_equals_the_restatement(n):
    g = np.random.default_rng(100 + n)
    lens = sorted({0, 1, 2, 3, max(n - 1, 0), n, n + 1, 5000})
    R = len(lens)
    crops = [g.standard_normal((ln, 3)).astype(np.float32) for ln in lens]
    lead = 7                                                  # the first crop starts at a non-zero offset
    points = np.concatenate([np.full((lead, 3), 1e9, np.float32)] + crops)
    offsets = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    pts_d, off_d = dev(points), dev(offsets)
    for B in (1, 3, 130):
        rows = g.integers(0, R, B)                            # repeated rows
        rows[0] = R - 1                                       # the long crop
        if B > 1:
            rows[1:1 + R] = np.arange(R)[:B - 1]              # every length
            rows[-1] = -1
        keys = g.integers(0, 2 ** 31 - 1, B)
        rand = g.integers(0, 2 ** 32, (B, n), dtype=np.uint64).astype(np.uint32)
        rand[:, 0] = 0xFFFFFFFF
        for kw in (dict(rand=rand), dict(seed=5, keys=keys), dict(seed=-2 ** 63 + 12345), dict()):
            got = raw_gather(pts_d, off_d, rows, n, **kw)
            want = SR.gather(points, offsets, rows, n, **kw)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (n, B, sorted(kw))
            assert np.array_equal(got[1], want[1]) and got[2] == want[2] == 0
        if B > 1:
            assert got[1][-1] == 0 and not got[0][-1].any()   # a -1 row: zeros, size 0, no flag
    # rows past the table: zeros, size 0, the flag -- never a read
    rows = np.array([R, 1, 2 ** 31 - 1, R - 1])
    got = raw_gather(pts_d, off_d, rows, n, seed=1)
    want = SR.gather(points, offsets, rows, n, seed=1)
    assert got[2] == want[2] == SR.INFO_ROW
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert not got[0][[0, 2]].any() and got[1].tolist() == [0, 1, 0, 5000]


# ---- the pair rule ----
@pytest.fixture(scope="module")
def hand_store():
    table = hand_table()
    keys, _ = rows_of(table)
    g = np.random.default_rng(3)
    arrays = [g.standard_normal((table.by_token[tok]["frames"][n], 3)).astype(np.float32) for tok, n in keys]
    return ST.CropStore.from_arrays(arrays, keys=keys, device=DEV, table=table), arrays


def test_pair_rule_equals_the_restatement(hand_store):
    store, _ = hand_store
    true = np.asarray(store.table.true_index)
    for B in (1, 70):
        items = true[np.arange(B) % len(true)][::-1].copy()
        keys = np.arange(B) * 7 + 3
        for seed in (0, 0x1234567800000009):
            store.info.zero_()
            got = [t.cpu().numpy() for t in store.train_pairs(i32(items), i32(keys), seed)]
            rows, labels, ids, info, trace = SR.train_pairs(store.host_tables, items, keys, seed=seed)
            assert np.array_equal(got[0], rows) and np.array_equal(got[1], labels) and np.array_equal(got[2], ids)
            assert store.flags() == info == 0
    # both kinds of pair and both pools occurred at B = 70
    assert any(t["positive"] for t in trace) and {t["use_tp"] for t in trace if not t["positive"]} == {True, False}
    # items the tables cannot serve: out of range, an object with one observation, a false positive's class gate passes but
    # a single observation does not -> -1 everywhere and the item flag
    toks = [o["token"] for o in store.table.objects]
    items = np.array([-1, len(toks), toks.index("A4"), toks.index("F2"), toks.index("A0")])
    got = [t.cpu().numpy() for t in store.train_pairs(i32(items), i32(np.arange(5)), 9)]
    rows, labels, ids, info, _ = SR.train_pairs(store.host_tables, items, np.arange(5), seed=9)
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], labels) and np.array_equal(got[2], ids)
    assert (got[0][:4] == -1).all() and (got[0][4] >= 0).all() and store.flags() == info == SR.INFO_ITEM
    store.info.zero_()


def test_gather_and_train_pairs_refuse_a_bad_argument(hand_store):
    """B = 2, n = 8: strided rows, keys of the wrong length and an out of the wrong shape are a PcrError that names the
    argument, not an assert; nothing is launched and the info word stays clear"""
    store, _ = hand_store
    store.info.zero_()
    B, n = 2, 8
    rows, keys = i32(np.zeros(B)), i32(np.arange(B))
    wide = i32(np.zeros(2 * B))
    clouds, sizes = torch.zeros((B, n, 3), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    for kw, what in ((dict(rows=wide[::2]), "rows must be contiguous"), (dict(keys=i32(np.arange(B + 1))), r"keys must be \(2,\)"),
                     (dict(out=(clouds[:, :n - 1], sizes)), r"out\[0\] \(clouds\) must be \(2, 8, 3\)"),
                     (dict(out=(clouds, i32(np.zeros(B + 1)))), r"out\[1\] \(sizes\) must be \(2,\)"),
                     (dict(rows=rows.long()), "rows must be a torch.int32 tensor"),
                     (dict(rows=rows.cpu()), "MI355X device tensor")):
        a = dict(dict(rows=rows, keys=keys), **kw)
        with pytest.raises(L.PcrError, match=what):
            store.gather(a["rows"], n, keys=a["keys"], seed=1, out=a.get("out"))
    true = int(store.table.true_index[0])
    items = i32(np.full(B, true))
    for kw, what in ((dict(items=i32(np.full(2 * B, true))[::2]), "items must be contiguous"),
                     (dict(keys=i32(np.arange(B + 1))), r"keys must be \(2,\)"),
                     (dict(out=torch.zeros((3, B, 3), dtype=torch.int32, device=DEV)), r"out must be \(3, 2, 2\)"),
                     (dict(out=torch.zeros((3, B, 2), device=DEV)), "out must be a torch.int32 tensor"),
                     (dict(rand=i32(np.zeros(B * ST.PAIR_WORDS - 1))), "rand must hold 80 elements")):
        a = dict(dict(items=items, keys=keys), **kw)
        with pytest.raises(L.PcrError, match=what):
            store.train_pairs(a["items"], a["keys"], 3, rand=a.get("rand"), out=a.get("out"))
    assert store.flags() == 0
    got = store.gather(rows, n, keys=keys, seed=1, out=(clouds, sizes))       # and the right call still goes through
    assert got[0] is clouds and got[1] is sizes


def test_thirty_two_failed_attempts_take_the_first_other_entry(hand_store):
    """the kernel is fed the same words as the restatement through its `rand` input: every candidate pick hits the item's
    own object"""
    store, _ = hand_store
    toks = [o["token"] for o in store.table.objects]
    a2, a3 = toks.index("A2"), toks.index("A3")
    rand = np.zeros((3, SR.PAIR_WORDS), np.uint32)
    rand[:, 2] = 0xFFFFFFFF                                  # density: bucket 6 = {A2, A3}
    rand[:, 3] = 0x80000000                                  # true pool
    rand[1, 4:4 + 31] = 0                                    # item 1 (A3): 31 picks of A2 ... all fine: A2 is not A3
    rand[2, 4:4 + 32] = 0xFFFFFFFF                           # item 2 (A3): 32 picks of A3 itself
    items = np.array([a2, a3, a3])
    store.info.zero_()
    got = [t.cpu().numpy() for t in store.train_pairs(i32(items), i32([0, 1, 2]), 0, rand=dev(rand.view(np.int32)))]
    rows, labels, ids, info, trace = SR.train_pairs(store.host_tables, items, [0, 1, 2], rand=rand.view(np.int32))
    assert [t["attempts"] for t in trace] == [32, 1, 32] and info == SR.INFO_RETRY
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], labels) and np.array_equal(got[2], ids)
    assert ids.tolist() == [[a2, a3], [a3, a2], [a3, a2]] and store.flags() == SR.INFO_RETRY
    store.info.zero_()


# ---- batches ----
N = 128


def fixed_crops(root, seed=0):
    """a toy crop directory in which every crop has exactly N points, or at most 2: no path resamples, so the host's
    items and the device's are the same bits whatever generator either uses"""
    g = np.random.default_rng(seed)
    meta = {}
    for i in range(18):
        fp = i >= 12
        tok = ("FP_%02d" if fp else "obj_%02d") % i
        meta[tok] = dict(cls=i % 2, fp=fp, visibility={})
        for obs in range(int(g.integers(3, 6))):
            d = os.path.join(root, tok, str(obs))
            os.makedirs(d)
            n = N if obs < 2 or g.random() < 0.6 else int(g.integers(1, 3))
            (g.standard_normal((n, 3)).astype(np.float32) + i).tofile(os.path.join(d, "pts_xyz.bin"))
            meta[tok]["visibility"][obs] = int(g.integers(1, 5))
    return meta


@pytest.fixture(scope="module")
def fixed(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fixed"))
    meta = fixed_crops(root)
    crops = LD.CropDirectory(root)
    table = crops.table(meta, num_classes=2)
    store = ST.CropStore.from_directory(root, table, device=DEV)
    return root, meta, crops, table, store


def host_batch(store, crops, rows, labels, ids, n, extra=None):
    """collate_pairs of the host items rebuilt from rows: files read again, data.subsample_pc"""
    cm = lambda p: np.moveaxis(np.asarray(p), 0, 1)          # noqa: E731
    items = []
    for b in range(rows.shape[0]):
        it = {}
        for s, side in enumerate(("1", "2")):
            tok, obs = store.key_of[rows[b, s]]
            it["sparse_" + side] = D.subsample_pc(cm(crops.read(tok, obs)), n)
        for s, side in enumerate(("1", "2")):
            it["label_" + side], it["id_" + side] = int(labels[b, s]), int(ids[b, s])
            if extra is not None:
                it["size_" + side], it["vis_" + side] = int(extra[0][b, s]), int(extra[1][b, s])
        items.append(it)
    return D.collate_pairs(items, device=DEV)


def assert_same_batch(got, want):
    assert set(got) == set(want)
    for k in want:
        assert len(got[k]) == len(want[k]), k
        for a, b in zip(got[k], want[k]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, (k, a.dtype, b.dtype, a.shape, b.shape)
            assert torch.equal(a, b), k


def test_train_batch_equals_collate_of_the_host_items_and_trains_to_the_same_loss(fixed):
    import bench
    root, meta, crops, table, store = fixed
    np.random.seed(0)
    ds = LD.TrainPairs(table, crops.read, subsample_sparse=N)
    B = 8
    items = i32(ds.idx[np.arange(B) % len(ds)])
    keys = i32(np.arange(B))
    batch = store.train_batch(items, keys, 21, n=N)
    rows, labels, ids = (t.cpu().numpy() for t in store.train_pairs(items, keys, 21))
    assert store.flags() == 0 and (rows >= 0).all()
    want = host_batch(store, crops, rows, labels, ids, N)
    assert_same_batch(batch, want)
    assert batch["dense_1"] is batch["sparse_1"] and batch["sparse_1"][0].shape == (N, 3)
    # one tensor behind every list
    assert len({t.untyped_storage().data_ptr() for t in batch["sparse_1"] + batch["sparse_2"]}) == 1
    # the pair rule's output against the restatement, the clouds against the stored crops
    r2 = SR.train_pairs(store.host_tables, items.cpu().numpy(), np.arange(B), seed=21)
    assert np.array_equal(rows, r2[0]) and np.array_equal(labels, r2[1]) and np.array_equal(ids, r2[2])
    m, _ = bench.build_pt_model([128, 64, 32])
    m.train()
    loss = [m.train_step(b, None)["loss"].detach().cpu() for b in (batch, want)]
    assert torch.equal(loss[0], loss[1]) and torch.isfinite(loss[0]).all()


def test_evaluate_model_with_a_store_equals_the_host_path(fixed):
    import bench
    from pcr_amd import evaluate as EV
    root, meta, crops, table, store = fixed
    vis = {tok: {int(k): v for k, v in e["visibility"].items()} for tok, e in meta.items()}
    pos, neg = PR.build_val_pairs(table, 3, seed=0)
    # (a fixed-size stand-in for the aggregated cloud, as evaluate.build_val_set passes: forward_test stacks it)
    ds = LD.ValPairs(table, pos, neg, crops.read, N, 8, read_dense=lambda tok: np.zeros((3, 8)), visibility=vis)
    assert len(ds) >= 40
    # an item of the store against the dataset's, the size / swapped visibility keys included
    store.val = None
    assert store.set_val_pairs(pos, neg, vis) == len(ds)
    np.random.seed(1)
    its = [ds[i] for i in (0, 1, len(pos), len(ds) - 1)]
    for it in its:                                            # (the store's dense cloud is the sparse one, as
        it.pop("dense_1"), it.pop("dense_2")                  #  collate_pairs fills it for an item without one)
    for j, i in enumerate((0, 1, len(pos), len(ds) - 1)):
        assert_same_batch(store.val_batch(i, i + 1, 0, n=N), D.collate_pairs([its[j]], device=DEV))
    m, _ = bench.build_pt_model([128, 64, 32])
    a = EV.evaluate_model(m, ds, 16, seed=3, rank=0, world=1)
    b = EV.evaluate_model(m, ds, 16, seed=3, rank=0, world=1, store=store)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["targets"], b["targets"])
    assert a["num_pairs"] == b["num_pairs"] == len(ds)
    for k, v in a.items():
        if isinstance(v, (int, float)):
            assert b[k] == v or (v != v and b[k] != b[k]), k
    from pcr_amd import metrics
    assert sorted(a["tables"]) == sorted(b["tables"])
    for name in a["tables"]:
        assert str(metrics.flatten_tables(a["tables"][name])) == str(metrics.flatten_tables(b["tables"][name])), name
    store.val = None


def test_evaluate_checkpoint_with_a_device_store_equals_the_host_path(fixed, tmp_path):
    """config file -> model -> checkpoint -> pairs, once with the host items and once with the crop directory read into
    a CropStore on the device (`device_store=True`): the same logits and the same accuracy"""
    from conftest import ROOT
    from pcr_amd import evaluate as EV
    from pcr_amd import testing as T
    from test_evaluate import VAL_CFG
    from test_gpu_evaluate import CONFIG, DATA
    root, meta, crops, table, _ = fixed
    (tmp_path / "data.py").write_text(DATA % (dict(VAL_CFG, subsample_sparse=N),))
    (tmp_path / "exp.py").write_text(CONFIG)
    sd = T.seeded_state_dict(T.load_manifest(os.path.join(ROOT, "tests", "golden", "pt_manifest.json")), 0)
    ckpt = str(tmp_path / "epoch_1.pth")
    torch.save({"meta": {"epoch": 1}, "state_dict": sd}, ckpt)
    run = lambda **kw: EV.evaluate_checkpoint(str(tmp_path / "exp.py"), ckpt, root, meta=meta, **kw)     # noqa: E731
    a, b = run(), run(device_store=True)
    assert a["num_pairs"] == b["num_pairs"] >= 40 and a["world"] == b["world"] == 1
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["targets"], b["targets"])
    assert a["val_match_acc"] == b["val_match_acc"]


@pytest.fixture(scope="module")
def general(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("general"))
    meta = make_crops(root, n_true=24, n_fp=6, seed=2)
    crops = LD.CropDirectory(root)
    table = crops.table(meta, num_classes=2)
    return root, meta, crops, table, ST.CropStore.from_directory(root, table, device=DEV)


def test_val_batches_do_not_depend_on_batch_size_or_shard(general):
    root, meta, crops, table, store = general
    pos, neg = PR.build_val_pairs(table, 2, seed=0)
    P = store.set_val_pairs(pos, neg)
    assert P >= 40
    n = 32

    def run(cuts):
        out = [store.val_batch(lo, hi, 77, n=n) for lo, hi in zip(cuts[:-1], cuts[1:])]
        return {k: torch.cat([torch.stack(b[k]) for b in out]) for k in ("sparse_1", "sparse_2", "size_1", "size_2", "id_2")}
    whole = run([0, P])
    for cuts in (list(range(0, P, 8)) + [P], list(range(0, P, 32)) + [P]):
        part = run(cuts)
        assert all(torch.equal(part[k], whole[k]) for k in whole)
    half = P // 2                                             # two ranks' shards, each in its own batches
    lo_half, hi_half = run([0, 8, half]), run([half, P])
    assert all(torch.equal(torch.cat([lo_half[k], hi_half[k]]), whole[k]) for k in whole)
    # and they are the restatement's clouds under the global pair index
    rows = store.val["rows"].cpu().numpy().reshape(-1)
    want, sizes, info = SR.gather(store.points.cpu().numpy()[:-1], store.offsets.cpu().numpy(), rows, n, keys=np.arange(2 * P),
                                  seed=77)
    assert np.array_equal(whole["sparse_1"].cpu().numpy(), want[0::2]) and np.array_equal(whole["sparse_2"].cpu().numpy(), want[1::2])
    assert np.array_equal(whole["size_2"].cpu().numpy()[:, 0], sizes[1::2]) and (sizes != n).any() and store.flags() == 0
    assert not torch.equal(run([0, P])["sparse_1"], store_other_seed(store, P, n))
    store.val = None


def store_other_seed(store, P, n):
    return torch.stack(store.val_batch(0, P, 78, n=n)["sparse_1"])


def test_run_epochs_from_the_device_loader_graph_equals_eager(general):
    import bench
    from pcr_amd import train
    root, meta, crops, table, store = general
    np.random.seed(0)
    ds = LD.TrainPairs(table, crops.read, subsample_sparse=N)
    losses = {}
    for graph in (False, True):
        m, _ = bench.build_pt_model([128, 64, 32])
        m.train()
        ld = ST.DeviceEpochLoader(store, ds, samples_per_gpu=4, seed=5)
        assert len(ld) >= 5 and len(ld) == len(LD.EpochLoader(ds, 4, seed=5))
        tr = train.Trainer(m, max_iters=len(ld), lr=1e-3, grad_clip=1.0, graph=graph)
        out = LD.run_epochs(tr, ld, 1)
        assert tr.graph == graph and len(out) == len(ld) == tr.iter      # (the lists of views went through the capture)
        losses[graph] = [float(x) for x in out]
    assert losses[False] == losses[True] and all(np.isfinite(losses[True]))
    assert len(set(losses[True])) == len(losses[True])                   # every batch is another one
    assert store.flags() & ~SR.INFO_RETRY == 0
    # the order on the device is the sampler's, the keys the dataset indices
    ld = ST.DeviceEpochLoader(store, ds, samples_per_gpu=4, num_replicas=2, rank=1, seed=5)
    first = next(iter(ld.epoch(3)))
    sampler = LD.DistributedGroupSampler(ds.flag, 4, 2, 1, seed=5)
    sampler.set_epoch(3)
    order = np.asarray(list(sampler))[:4]
    rows, labels, ids, _, _ = SR.train_pairs(store.host_tables, ds.idx[order], order, seed=ST.epoch_seed(5, 3))
    assert torch.cat(first["id_1"]).tolist() == ids[:, 0].tolist() and torch.cat(first["id_2"]).tolist() == ids[:, 1].tolist()
    assert torch.cat(first["label_2"]).tolist() == labels[:, 1].tolist()


def test_captured_train_batch_draws_fresh_samples_from_a_new_seed(general):
    root, meta, crops, table, store = general
    np.random.seed(0)
    ds = LD.TrainPairs(table, crops.read, subsample_sparse=N)
    B, n = 6, 32
    items_h, keys_h = ds.idx[np.arange(B) % len(ds)], np.arange(B) + 40
    items, keys = i32(items_h), i32(keys_h)
    seed = torch.tensor([11], dtype=torch.int64, device=DEV)
    points, offsets = store.points.cpu().numpy()[:-1], store.offsets.cpu().numpy()

    def want(s):
        rows, labels, ids, info, _ = SR.train_pairs(store.host_tables, items_h, keys_h, seed=s)
        gk = np.stack([2 * keys_h, 2 * keys_h + 1], 1).reshape(-1)
        clouds, _, _ = SR.gather(points, offsets, rows.reshape(-1), n, keys=gk, seed=s)
        return clouds.reshape(B, 2, n, 3), labels, ids

    def check(batch, s):
        clouds, labels, ids = want(s)
        for j, side in enumerate(("1", "2")):
            assert np.array_equal(torch.stack(batch["sparse_" + side]).cpu().numpy(), clouds[:, j])
            assert torch.cat(batch["label_" + side]).tolist() == labels[:, j].tolist()
            assert torch.cat(batch["id_" + side]).tolist() == ids[:, j].tolist()
    check(store.train_batch(items, keys, seed, n=n), 11)     # one eager call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch = store.train_batch(items, keys, seed, n=n)
    ptrs = [t.data_ptr() for k in sorted(batch) for t in batch[k]]
    graph.replay()
    check(batch, 11)
    for s in (12, -5):
        seed.fill_(s)
        graph.replay()
        check(batch, s)
        assert [t.data_ptr() for k in sorted(batch) for t in batch[k]] == ptrs
    assert not np.array_equal(want(12)[0], want(11)[0])
