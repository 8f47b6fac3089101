"""The crop set resident on the device, and pair batches assembled by launches (include/pcr.h section A6,
csrc/store_kernels.hip).

The host path (`loader.EpochLoader` over `TrainPairs`, `evaluate_model` over `ValPairs`) reads one file per cloud,
resamples it with numpy's global generator and copies every cloud, label and id to the device on its own.  Here every
`pts_xyz.bin` is read ONCE into one packed device buffer; a batch is then two launches -- the training pair rule over
int32 tables (`pcr_store_train_pairs_i32`) and `subsamplePC` of both sides (`pcr_store_gather_f32`) -- with no host read
and no host-to-device copy, so that both can be captured in a HIP graph.  The samples come from the counter-based word
W(seed, stream, key, k) of pcr.h: another stream than numpy's, the same distribution, the same bits for a (seed, key)
whatever the batch size or the number of ranks.  `dense_*` is `sparse_*`, as `data.collate_pairs` does when an item has
none (no ReID config trains a loss that reads the aggregated cloud).  INTEGRATION.md 2f has the mapping.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import abi
from . import data as D
from .loader import DistributedGroupSampler, ValPairs
from .pairs import BUCKETS

NB = len(BUCKETS)
PAIR_WORDS = 40                  # PCR_STORE_PAIR_WORDS
INFO_RETRY, INFO_ITEM, INFO_ROW = 1, 2, 4
POOLS = ("tp", "fp")
_WHO = "pcr_amd.store"


def pair_tables(table, row_of, ids=None):
    """the int32 tables of pcr_store_train_pairs_i32 from an `ObjectTable`, every order the one `TrainPairs.__getitem__`
    indexes; `row_of[(token, observation)]` -> store row.  Raises ValueError for a table on which `_class_list_density`
    (a class of a training object without a bucket of two objects in a pool) could raise at draw time: a launch cannot."""
    objs = table.objects
    O, C = len(objs), int(table.num_classes)
    index = {o["token"]: i for i, o in enumerate(objs)}
    ids = ids if ids is not None else index
    nums_off, nums_rows, bucket_off, bucket_rows = [0], [], [0], []
    for o in objs:
        nums_rows += [row_of[(o["token"], n)] for n in o["nums"]]
        nums_off.append(len(nums_rows))
        for b in BUCKETS:
            bucket_rows += [row_of[(o["token"], n)] for n in o["buckets"].get(b, [])]
            bucket_off.append(len(bucket_rows))
    pool_off, pool_objs = [0], []
    for pool in (table.tp, table.fp):
        for c in range(C):
            for b in BUCKETS:
                pool_objs += [index[tok] for tok, _ in pool.get(c, {}).get(b, [])]
                pool_off.append(len(pool_objs))
    off = np.asarray(pool_off)
    for c in sorted({objs[i]["cls"] for i in table.true_index}):
        for p, name in enumerate(POOLS):
            cnt = np.diff(off[(p * C + c) * NB:(p * C + c + 1) * NB + 1])
            if not (cnt >= 2).any():
                raise ValueError("class %d has no point-count bucket with two objects in the %s pool: the pair rule "
                                 "cannot draw a negative for it" % (c, name))
    i32 = lambda a: np.asarray(a if len(a) else [0], dtype=np.int32)      # noqa: E731  (never an empty allocation)
    return dict(num_objects=O, num_classes=C,
                obj_cls=i32([o["cls"] for o in objs]), obj_fp=i32([1 if o.get("fp") else 0 for o in objs]),
                obj_id=i32([ids[o["token"]] for o in objs]),
                nums_off=i32(nums_off), nums_rows=i32(nums_rows), bucket_off=i32(bucket_off), bucket_rows=i32(bucket_rows),
                pool_off=i32(pool_off), pool_objs=i32(pool_objs))


def _seed_tensor(seed, device):
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1:
            raise L.PcrError("seed must be a device int64 tensor of one element or a Python int")
        return seed
    s = int(seed or 0) & 0xFFFFFFFFFFFFFFFF
    return torch.full((1,), s - (1 << 64) if s >= (1 << 63) else s, dtype=torch.int64, device=device)


class CropStore:
    """points (total, 3) f32, offsets (R + 1,) int64, lengths (R,) int32 on `device`; `row_of[(token, observation)]` and
    its inverse `key_of[row]` on the host.  With a `table`: the pair-rule tables too (`tables`, int32 on the device);
    pair_rule=False keeps the table for `set_val_pairs` only (evaluation draws no training pairs, and its table need not
    pass the pair rule's construction-time checks)."""

    n = 128                      # points per cloud: `subsample_sparse` of every ReID config

    def __init__(self, arrays, keys, device="cuda", table=None, ids=None, pair_rule=True):
        arrays = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in arrays]
        self.key_of = list(keys)
        if len(self.key_of) != len(arrays) or len(set(self.key_of)) != len(arrays):
            raise ValueError("one distinct (token, observation) key per crop is needed")
        self.row_of = {k: r for r, k in enumerate(self.key_of)}
        lengths = np.asarray([a.shape[0] for a in arrays], dtype=np.int64)
        offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
        np.cumsum(lengths, out=offsets[1:])
        packed = np.concatenate(arrays + [np.zeros((1, 3), np.float32)], axis=0)     # (one spare point: never empty)
        self.device = torch.device(device)
        self.points = torch.from_numpy(packed).to(self.device)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.lengths = torch.from_numpy(lengths.astype(np.int32)).to(self.device)
        self.num_rows = len(arrays)
        self.info = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.table, self.tables, self._block = table, None, None
        self.val = None
        if table is not None:
            self.ids = ids if ids is not None else {o["token"]: i for i, o in enumerate(table.objects)}
        if table is not None and pair_rule:
            self.host_tables = pair_tables(table, self.row_of, ids)
            self.tables = {k: (torch.from_numpy(v).to(self.device) if isinstance(v, np.ndarray) else v)
                           for k, v in self.host_tables.items()}
            p = abi.StoreTables()
            for k, v in self.tables.items():
                setattr(p, k, L._p(v) if torch.is_tensor(v) else int(v))
            self._block = p

    @classmethod
    def from_arrays(cls, arrays, keys=None, device="cuda", table=None, ids=None, pair_rule=True):
        """arrays: a list of (n_i, 3) arrays; keys: their (token, observation) pairs (default (i, 0))"""
        arrays = list(arrays)
        return cls(arrays, keys if keys is not None else [(i, 0) for i in range(len(arrays))], device, table, ids,
                   pair_rule)

    @classmethod
    def from_directory(cls, crop_root, table, device="cuda", load_fraction=1.0, ids=None, pair_rule=True):
        """every `<crop_root>/<token>/<observation>/pts_xyz.bin` of the table's objects, read once, `load_points`'
        `load_fraction` rule applied at that point"""
        arrays, keys = [], []
        for o in table.objects:
            for obs in sorted(o["frames"], key=int):
                arrays.append(D.load_points(str(crop_root), o["token"], obs, load_fraction=load_fraction)[:, :3])
                keys.append((o["token"], obs))
        return cls(arrays, keys, device, table, ids, pair_rule)

    @property
    def nbytes(self):
        ts = [self.points, self.offsets, self.lengths] + [v for v in (self.tables or {}).values() if torch.is_tensor(v)]
        if self.val is not None:
            ts += [v for v in self.val.values() if torch.is_tensor(v)]
        return sum(t.numel() * t.element_size() for t in ts)

    def flags(self):
        """the sticky info word of the launches so far (a host read): INFO_RETRY | INFO_ITEM | INFO_ROW"""
        return int(self.info.item())

    # ---- the two launches ----
    def gather(self, rows, n, keys=None, rand=None, seed=None, out=None, info=None):
        """rows (B,) int32 -> clouds (B, n, 3) f32, sizes (B,) int32 (pcr_store_gather_f32)"""
        seed_t = _seed_tensor(seed, self.device) if seed is not None else None
        info = self.info if info is None else info
        i32 = torch.int32
        rows = L.tensor(rows, _WHO, "rows", i32, shape=(None,))
        B, n = rows.numel(), int(n)
        keys = L.tensor(keys, _WHO, "keys", i32, shape=(B,), optional=True)
        rand = L.tensor(rand, _WHO, "rand", i32, numel=B * n, optional=True)
        info = L.tensor(info, _WHO, "info", i32, numel=1)
        L.require(out is None or len(out) == 2, _WHO, "out must be (clouds, sizes)")
        clouds = L.out_tensor(None if out is None else out[0], _WHO, "out[0] (clouds)", torch.float32, (B, n, 3), self.device)
        sizes = L.out_tensor(None if out is None else out[1], _WHO, "out[1] (sizes)", i32, (B,), self.device)
        L.require_cuda(self.points, rows, keys, rand, seed_t, info, clouds, sizes)
        L.run.pcr_store_gather_f32(self.points, L.ptr(self.offsets), self.num_rows, rows, keys, rand, L.ptr(seed_t),
                                   clouds, sizes, info, B, n, L.stream_ptr())
        return clouds, sizes

    def train_pairs(self, items, keys, seed=None, rand=None, out=None, info=None):
        """items, keys (B,) int32 -> rows, labels, ids (B, 2) int32 (pcr_store_train_pairs_i32)"""
        if self._block is None:
            raise L.PcrError("this CropStore was built without an ObjectTable: it holds no pair-rule tables")
        seed_t = _seed_tensor(seed, self.device) if seed is not None else None
        info = self.info if info is None else info
        i32 = torch.int32
        items = L.tensor(items, _WHO, "items", i32, shape=(None,))
        B = items.numel()
        keys = L.tensor(keys, _WHO, "keys", i32, shape=(B,))
        rand = L.tensor(rand, _WHO, "rand", i32, numel=B * PAIR_WORDS, optional=True)
        info = L.tensor(info, _WHO, "info", i32, numel=1)
        out = L.out_tensor(out, _WHO, "out", i32, (3, B, 2), self.device)
        L.require_cuda(items, keys, rand, seed_t, info, out)
        L.run.pcr_store_train_pairs_i32(ctypes.byref(self._block), items, keys, rand, L.ptr(seed_t), out[0], out[1],
                                        out[2], info, B, L.stream_ptr())
        return out[0], out[1], out[2]

    # ---- batches ----
    @staticmethod
    def _sides(clouds, labels, ids):
        """(B, 2, ...) tensors -> the model's lists of per-sample views (what `collate_pairs` builds from items)"""
        out = {}
        for s, side in enumerate(("1", "2")):
            out["sparse_" + side] = list(clouds[:, s].unbind(0))
            out["dense_" + side] = out["sparse_" + side]
            out["label_" + side] = list(labels[:, s:s + 1].unbind(0))
            out["id_" + side] = list(ids[:, s:s + 1].unbind(0))
        return out

    def train_batch(self, items, keys, seed, n=None, gather_keys=None):
        """items (B,) int32 object indices (`TrainPairs.idx[i]`), keys (B,) int32 (the samples' dataset indices), seed an
        int or a device int64 tensor -> the model's input dict: `sparse_1/2`, `dense_1/2` (= sparse), `label_1/2`,
        `id_1/2`, each a list of views of one tensor.  n: points per cloud (default: `self.n`); gather_keys: (B, 2) int32
        = 2 * keys + side when the caller holds it already."""
        n = int(self.n if n is None else n)
        seed_t = _seed_tensor(seed, self.device)
        B = items.numel()
        prl = torch.empty((3, B, 2), dtype=torch.int32, device=self.device)
        rows = self.train_pairs(items, keys, seed_t, out=prl)[0]
        if gather_keys is None:
            gather_keys = torch.stack((2 * keys, 2 * keys + 1), dim=1)
        clouds, _ = self.gather(rows.view(-1), n, keys=gather_keys.reshape(-1), seed=seed_t)
        meta = prl[1:3].to(torch.int64)                  # labels, ids as collate_pairs types them
        return self._sides(clouds.view(B, 2, n, 3), meta[0], meta[1])

    def set_val_pairs(self, positives, negatives=(), visibility=None):
        """upload a validation pair list (pairs.build_val_pairs) once: rows, classes, ids and visibility as `ValPairs`
        returns them (its swap of the two visibility entries included), computed on the host here and kept on the device"""
        if self.table is None:
            raise L.PcrError("this CropStore was built without an ObjectTable")
        pairs = list(positives) + list(negatives)
        vis = visibility or {}
        rows, labels, ids, vv = [], [], [], []
        for p in pairs:
            o2 = self.table.by_token[p["tok2"]]
            id1 = self.ids[p["tok1"]]
            if p["tok2"] == p["tok1"] and p["match"]:
                id2 = id1
            else:
                id2 = -1 if o2.get("fp") else self.ids[p["tok2"]]
            v1 = ValPairs.VIS.get(vis.get(p["tok1"], {}).get(int(p["o1"]), -1), -1)
            v2 = ValPairs.VIS.get(vis.get(p["tok2"], {}).get(int(p["o2"]), -1), -1)
            rows.append((self.row_of[(p["tok1"], int(p["o1"]))], self.row_of[(p["tok2"], int(p["o2"]))]))
            labels.append((p["cls1"], p["cls2"]))
            ids.append((id1, id2))
            vv.append((v2, v1))
        P = len(pairs)
        up = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt).reshape(P, 2)).to(self.device)     # noqa: E731
        self.val = dict(num_pairs=P, rows=up(rows, np.int32), labels=up(labels, np.int64), ids=up(ids, np.int64),
                        vis=up(vv, np.int64),
                        keys=up(np.arange(2 * P), np.int32))      # 2 * (global pair index) + side
        return P

    def val_batch(self, lo, hi, seed, n=None):
        """pairs [lo, hi) of the uploaded list -> the model's input dict with the `size_*` / `vis_*` keys of `ValPairs`
        (`size_*`: the stored length).  The keys are the GLOBAL pair indices: a pair's clouds do not depend on the batch
        size or on which rank draws them."""
        if self.val is None:
            raise L.PcrError("CropStore.val_batch: no pair list (set_val_pairs)")
        v = self.val
        lo, hi = int(lo), int(hi)
        L.require(0 <= lo <= hi <= v["num_pairs"], _WHO, "lo, hi = %d, %d must lie in 0 <= lo <= hi <= %d pairs",
                  lo, hi, v["num_pairs"])
        n = int(self.n if n is None else n)
        B = hi - lo
        clouds, sizes = self.gather(v["rows"][lo:hi].view(-1), n, keys=v["keys"][lo:hi].view(-1),
                                    seed=_seed_tensor(seed, self.device))
        out = self._sides(clouds.view(B, 2, n, 3), v["labels"][lo:hi], v["ids"][lo:hi])
        sizes = sizes.view(B, 2).to(torch.int64)
        for s, side in enumerate(("1", "2")):
            out["size_" + side] = list(sizes[:, s:s + 1].unbind(0))
            out["vis_" + side] = list(v["vis"][lo:hi, s:s + 1].unbind(0))
        return out


def epoch_seed(seed, epoch):
    """the seed word of an epoch: a function of (seed, epoch) only, so that every rank and every batch size draws the
    same sample for a dataset index"""
    return ((int(seed or 0) & 0xFFFFFFFF) << 32) | (int(epoch) & 0xFFFFFFFF)


class DeviceEpochLoader:
    """`EpochLoader`'s interface (`epoch(ep)`, `len`) over a CropStore: the `DistributedGroupSampler` order of an epoch
    is uploaded once as one int32 tensor, a batch is a slice of it, the keys are the dataset indices.  No per-batch
    host-to-device copy, no host read; `loader.run_epochs` takes it unchanged."""

    def __init__(self, store, train_pairs, samples_per_gpu, num_replicas=1, rank=0, seed=0, n=None):
        self.store, self.spg, self.seed = store, int(samples_per_gpu), seed
        self.n = int(n if n is not None else getattr(train_pairs, "ns", store.n))
        self.idx = np.asarray(train_pairs.idx, dtype=np.int64)
        self.sampler = DistributedGroupSampler(train_pairs.flag, samples_per_gpu, num_replicas, rank, seed=seed)

    def __len__(self):
        return len(self.sampler) // self.spg

    def epoch(self, epoch):
        self.sampler.set_epoch(epoch)
        order = np.asarray(list(self.sampler), dtype=np.int64)
        up = np.stack([self.idx[order], order, 2 * order, 2 * order + 1]).astype(np.int32)
        dev = torch.from_numpy(up).to(self.store.device)           # the epoch's ONE upload
        items, keys, gkeys = dev[0], dev[1], dev[2:4].t().contiguous()
        seed_t = _seed_tensor(epoch_seed(self.seed, epoch), self.store.device)
        for bi in range(len(self)):
            lo, hi = bi * self.spg, (bi + 1) * self.spg
            yield self.store.train_batch(items[lo:hi], keys[lo:hi], seed_t, n=self.n, gather_keys=gkeys[lo:hi])
