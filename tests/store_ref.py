"""CPU restatement (numpy) of include/pcr.h section A6: the word W(seed, stream, key, k), pick, the gather
(pcr_store_gather_f32 = subsamplePC over packed crops) and the training pair rule (pcr_store_train_pairs_i32 =
TrainPairs.__getitem__ over the CSR tables of pcr_amd.store.pair_tables).  Words in, rows and clouds out; the device
launches equal these bit for bit (tests/test_gpu_store.py), and tests/test_store_cpu.py chains them to the host rules."""
import numpy as np

BUCKETS = 20
PAIR_ATTEMPTS = 32
PAIR_WORDS = 40
INFO_RETRY, INFO_ITEM, INFO_ROW = 1, 2, 4
STREAM_PAIRS, STREAM_GATHER = 1, 2
_M = np.uint64(0xFFFFFFFF)


def mix(x):
    x = np.asarray(x, np.uint64) & _M
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M
    x = x ^ (x >> np.uint64(16))
    return x


def prefix(seed, stream, key):
    """h of pcr.h after (seed, stream, key); key is read as 32 unsigned bits"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    h = mix((seed & 0xFFFFFFFF) ^ 0x9E3779B9)
    h = mix(h ^ np.uint64(seed >> 32))
    h = mix(h ^ np.uint64(stream))
    return mix(h ^ np.uint64(int(key) & 0xFFFFFFFF))


def W(seed, stream, key, k):
    """k: an int or an array of ints -> uint32 word(s)"""
    return mix(prefix(seed, stream, key) ^ np.asarray(k, np.uint64)).astype(np.uint32)


def pick(u, length):
    return (np.asarray(u).astype(np.uint64) * np.uint64(length)) >> np.uint64(32)


def as_words(a):
    """int32 device words -> the 32 unsigned bits the kernels read"""
    return np.asarray(a).astype(np.int64).astype(np.uint32)


def sample_slots(words, length):
    """the stored-point index of every slot: pick(u, len) as int64"""
    return pick(words, length).astype(np.int64)


def gather(points, offsets, rows, n, keys=None, rand=None, seed=0):
    """points (total, 3) f32, offsets (R + 1,) int64, rows (B,) -> clouds (B, n, 3) f32, sizes (B,) int32, info"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    R = offsets.shape[0] - 1
    B = len(rows)
    clouds = np.zeros((B, n, 3), np.float32)
    sizes = np.zeros((B,), np.int32)
    info = 0
    for b, row in enumerate(np.asarray(rows).tolist()):
        if row >= R:
            info |= INFO_ROW
            continue
        if row < 0:
            continue
        lo, hi = int(offsets[row]), int(offsets[row + 1])
        ln = sizes[b] = hi - lo
        if ln <= 2:
            continue
        if ln == n:
            clouds[b] = points[lo:hi]
            continue
        key = b if keys is None else int(keys[b])
        u = W(seed, STREAM_GATHER, key, np.arange(n)) if rand is None else as_words(np.asarray(rand).reshape(B, n)[b])
        clouds[b] = points[lo + sample_slots(u, ln)]
    return clouds, sizes, info


def walk(off, start, need):
    """_class_list_density / _frame_even over one CSR row `off` (BUCKETS + 1 offsets): from bucket `start` down to 0, then
    from 0 up, the first bucket with at least `need` entries; -1 for none"""
    for q in list(range(start, -1, -1)) + list(range(BUCKETS)):
        if off[q + 1] - off[q] >= need:
            return q
    return -1


def train_pairs(tables, items, keys, seed=0, rand=None):
    """tables: the dict of pcr_amd.store.pair_tables -> rows, labels, ids (B, 2) int32, info, trace (one dict per item:
    positive, use_tp, dens, db, fb, attempts -- which branches the item took)"""
    t = tables
    O, C = int(t["num_objects"]), int(t["num_classes"])
    B = len(items)
    rows, labels, ids = (np.full((B, 2), -1, np.int32) for _ in range(3))
    info, trace = 0, []
    for b in range(B):
        o = int(items[b])
        tr = dict(positive=None)
        trace.append(tr)
        c, n = -1, 0
        if 0 <= o < O:
            c = int(t["obj_cls"][o])
            nb = int(t["nums_off"][o])
            n = int(t["nums_off"][o + 1]) - nb
        if c < 0 or c >= C or n < 2:
            info |= INFO_ITEM
            continue
        words = W(seed, STREAM_PAIRS, int(keys[b]), np.arange(PAIR_WORDS)) if rand is None else \
            as_words(np.asarray(rand).reshape(B, PAIR_WORDS)[b])
        it = iter(words.tolist())
        nxt = lambda: next(it)                               # noqa: E731
        me = int(t["obj_id"][o])
        if nxt() >> 31 == 1:
            ia = int(pick(nxt(), n))
            j = int(pick(nxt(), n - 1))
            ib = j + (1 if j >= ia else 0)
            rows[b] = t["nums_rows"][nb + ia], t["nums_rows"][nb + ib]
            labels[b] = c, c
            ids[b] = me, me
            tr.update(positive=True)
            continue
        r1 = t["nums_rows"][nb + int(pick(nxt(), n))]
        r = int(pick(nxt(), n))
        bo = t["bucket_off"][o * BUCKETS:(o + 1) * BUCKETS + 1]
        dens = 0
        while dens < BUCKETS - 1 and bo[dens + 1] - bo[0] <= r:
            dens += 1
        use_tp = nxt() >> 31 == 1
        base = ((0 if use_tp else 1) * C + c) * BUCKETS
        po = t["pool_off"][base:base + BUCKETS + 1]
        db = walk(po, dens, 2)
        other, attempts = -1, 0
        if db >= 0:
            cands = t["pool_objs"][po[db]:po[db + 1]]
            for _ in range(PAIR_ATTEMPTS):
                attempts += 1
                cand = int(cands[int(pick(nxt(), len(cands)))])
                if cand != o:
                    other = cand
                    break
            if other < 0:
                info |= INFO_RETRY
                other = next((int(x) for x in cands if int(x) != o), -1)
        fb = -1
        if 0 <= other < O:
            oo = t["bucket_off"][other * BUCKETS:(other + 1) * BUCKETS + 1]
            fb = walk(oo, db, 1)
        tr.update(positive=False, use_tp=use_tp, dens=dens, db=db, fb=fb, attempts=attempts)
        if fb < 0:
            info |= INFO_ITEM
            continue
        r2 = t["bucket_rows"][oo[fb] + int(pick(nxt(), int(oo[fb + 1] - oo[fb])))]
        rows[b] = r1, r2
        labels[b] = c, (c if use_tp else c + C)
        ids[b] = me, (-1 if t["obj_fp"][other] else int(t["obj_id"][other]))
    return rows, labels, ids, info, trace
