"""CPU: the rules of the device crop store (include/pcr.h section A6) in their numpy restatement (tests/store_ref.py),
chained to the host rules they replace: the word and pick against hand-computed values, the gather against
`data.subsample_pc` on the same index stream, the pair rule against `TrainPairs.__getitem__` run under a scripted
`np.random.choice`, and the CSR tables of pcr_amd.store against the ObjectTable entry for entry.
tests/test_pairs_golden.py chains TrainPairs to the reference's own dataset, tests/test_gpu_store.py the launches to
store_ref: reference -> host rule -> device rule, with no statistical tolerance anywhere."""
import numpy as np
import pytest

import crops_ref
import store_ref as SR
from pcr_amd import data as D
from pcr_amd import loader as LD
from pcr_amd import pairs as PR
from pcr_amd import store as ST


# ---- the word ----
def _mix_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_word_and_pick_hand_values():
    # by hand: mix(0) = 0 (every step keeps zero); mix(1) step by step below, the first two steps read off without a
    # machine: 1 * 0x7feb352d, then ^ (that >> 15 = 0xffd6)
    assert int(SR.mix(0)) == 0
    assert int(SR.mix(1)) == _mix_int(1) and _mix_int(1) != 1
    x = 1
    x ^= x >> 16                       # 1
    x = (x * 0x7FEB352D) & 0xFFFFFFFF  # 0x7feb352d
    assert x == 0x7FEB352D
    x ^= x >> 15                       # 0x7feb352d ^ 0x0000ffd6
    assert x == 0x7FEB352D ^ 0xFFD6 == 0x7FEBCAFB
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(SR.mix(1)) == x
    # the A2 form, unchanged: the same function as the crop kernel's restatement
    v = np.array([0, 1, 2, 0x9E3779B9, 0xFFFFFFFF, 0x80000000, 12345678], np.uint64)
    assert np.array_equal(SR.mix(v), crops_ref._mix(v))
    assert [int(a) for a in SR.mix(v)] == [_mix_int(int(a)) for a in v]
    # W chains five mixes over (seed low ^ golden, seed high, stream, key, k)
    for seed, stream, key, k in ((0, 1, 0, 0), (7, 2, 5, 127), ((0xABCDEF01 << 32) | 0x12345678, 1, 0x7FFFFFFF, 36),
                                 (-3, 2, 9, 1)):
        s = seed & 0xFFFFFFFFFFFFFFFF
        h = _mix_int((s & 0xFFFFFFFF) ^ 0x9E3779B9)
        h = _mix_int(h ^ (s >> 32))
        h = _mix_int(h ^ stream)
        h = _mix_int(h ^ key)
        assert int(SR.W(seed, stream, key, k)) == _mix_int(h ^ k)
    assert np.array_equal(SR.W(7, 2, 5, np.arange(4)), [SR.W(7, 2, 5, k) for k in range(4)])
    # with stream and key folded the way A2 folds (box, slot), the words differ from the crop kernel's: other streams
    assert not np.array_equal(SR.W(3, 2, 0, np.arange(8)), crops_ref.crop_words(3, 0, 8))
    # pick(u, len) = floor(u * len / 2^32)
    assert int(SR.pick(0, 5)) == 0 and int(SR.pick(0xFFFFFFFF, 5)) == 4 and int(SR.pick(0x80000000, 5)) == 2
    assert int(SR.pick(0x33333333, 5)) == 0 and int(SR.pick(0x33333334, 5)) == 1      # 2^32 / 5 = 0x33333333.33
    assert int(SR.pick(0xFFFFFFFF, 1)) == 0 and int(SR.pick(0x7FFFFFFF, 2)) == 0 and int(SR.pick(0x80000000, 2)) == 1
    assert np.array_equal(SR.pick(np.array([0, 0xFFFFFFFF], np.uint32), 5000), [0, 4999])


# ---- the gather against subsample_pc ----
class _Stub:
    """`rng=` of data.subsample_pc: randint answers with pick(u, high) of the given words"""

    def __init__(self, words):
        self.words, self.calls = words, 0

    def randint(self, low, high, size, dtype):
        assert low == 0 and size == len(self.words)
        self.calls += 1
        return SR.pick(self.words, high).astype(dtype)


@pytest.mark.parametrize("n", [1, 32, 100, 128])
def test_gather_rule_equals_subsample_pc_on_the_same_index_stream(n):
    g = np.random.default_rng(n)
    lens = sorted({0, 1, 2, 3, max(n - 1, 0), n, n + 1, 5000})
    crops = [g.standard_normal((ln, 3)).astype(np.float32) for ln in lens]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in crops])]).astype(np.int64)
    points = np.concatenate(crops)
    rows = np.arange(len(lens))
    rand = g.integers(0, 2 ** 32, (len(lens), n), dtype=np.uint64).astype(np.uint32)
    rand[:, 0] = 0xFFFFFFFF                                  # the last point of a crop
    if n > 1:
        rand[:, 1] = 0
    for words, kw in ((rand, dict(rand=rand.view(np.int32))),
                      (np.stack([SR.W(11, 2, 3 * b + 1, np.arange(n)) for b in rows]),
                       dict(seed=11, keys=3 * rows + 1))):
        clouds, sizes, info = SR.gather(points, offsets, rows, n, **kw)
        assert info == 0 and sizes.tolist() == lens
        for b, c in enumerate(crops):
            stub = _Stub(words[b])
            want = D.subsample_pc(np.moveaxis(c, 0, 1), n, rng=stub)
            assert np.array_equal(clouds[b], np.asarray(want, np.float32)), (n, lens[b])
            assert stub.calls == (1 if lens[b] > 2 and lens[b] != n else 0)
    # padding and a row past the table
    clouds, sizes, info = SR.gather(points, offsets, [-1, len(lens), 3], n, rand=rand[:3].view(np.int32))
    assert info == SR.INFO_ROW and sizes[:2].tolist() == [0, 0] and not clouds[:2].any()


# ---- the pair rule against TrainPairs.__getitem__ ----
def hand_table():
    """12 true objects + 4 false positives, 2 classes, point counts placed in chosen buckets (bucket b = [2^b, 2^(b+1))).
    Class 0, true pool: bucket 0 {A5}, 1 {A1}, 3 {A0 A1 A2 A3 A5}, 5 {A3 A4}, 6 {A2 A3}, 7 {A0}; false positives:
    3 {F0 F1}, 5 {F0}, 6 {F1}.  A density of 7 steps DOWN (to 6 / to 3), a density of 1 finds nothing at or below it,
    wraps to the bottom and steps UP to 3; bucket 6 of the true pool holds two objects, so A2 and A3 draw themselves."""
    f = lambda *pts: {i: p for i, p in enumerate(pts)}        # noqa: E731
    objs = [dict(token="A0", cls=0, frames=f(9, 10, 12, 200)),
            dict(token="A1", cls=0, frames=f(8, 15, 11, 2)),
            dict(token="A2", cls=0, frames=f(9, 9, 70)),
            dict(token="A3", cls=0, frames={0: 13, 1: 14, 2: 65, 5: 40}),
            dict(token="F0", cls=0, fp=True, frames=f(9, 35)),
            dict(token="A4", cls=0, frames=f(33)),
            dict(token="A5", cls=0, frames=f(10, 1)),
            dict(token="B0", cls=1, frames=f(20, 21, 22)),
            dict(token="B1", cls=1, frames=f(16, 31, 22)),
            dict(token="F2", cls=1, fp=True, frames=f(17)),
            dict(token="B2", cls=1, frames=f(20, 21, 22, 23)),
            dict(token="B3", cls=1, frames=f(20, 21, 22)),
            dict(token="B4", cls=1, frames=f(5, 20, 600)),
            dict(token="F1", cls=0, fp=True, frames=f(12, 100)),
            dict(token="B5", cls=1, frames=f(5, 6, 7)),
            dict(token="F3", cls=1, fp=True, frames=f(18, 4))]
    return PR.ObjectTable(objs, num_classes=2)


def rows_of(table):
    keys = [(o["token"], n) for o in table.objects for n in sorted(o["frames"])]
    return keys, {k: r for r, k in enumerate(keys)}


class Script:
    """stands in for np.random.choice inside TrainPairs.__getitem__: the k-th draw of item `key` is answered from
    W(seed, 1, key, k) -- top bit for a coin, pick for an index, the integer cumulative bucket counts for a `p=` call"""

    def __init__(self, table, seed):
        self.table, self.seed = table, seed

    def begin(self, obj, key):
        self.obj, self.key, self.k = obj, key, 0

    def word(self):
        w = int(SR.W(self.seed, 1, self.key, self.k))
        self.k += 1
        return w

    def choice(self, a, size=None, replace=True, p=None):
        arr = np.arange(a) if np.isscalar(a) else np.asarray(a)
        if p is not None:
            counts = [len(self.obj["buckets"].get(b, [])) for b in PR.BUCKETS]
            assert np.allclose(p, np.asarray(counts) / sum(counts))
            r = int(SR.pick(self.word(), sum(counts)))
            return arr[int(np.searchsorted(np.cumsum(counts), r, side="right"))]
        if size is None:
            assert arr.tolist() == [0, 1]
            return self.word() >> 31
        if size == 2:
            assert not replace
            ia = int(SR.pick(self.word(), len(arr)))
            j = int(SR.pick(self.word(), len(arr) - 1))
            return arr[[ia, j + (1 if j >= ia else 0)]]
        assert size == 1
        return arr[[int(SR.pick(self.word(), len(arr)))]]


@pytest.fixture(scope="module")
def hand():
    table = hand_table()
    keys, row_of = rows_of(table)
    return table, keys, row_of, ST.pair_tables(table, row_of)


def test_pair_rule_equals_train_pairs_under_scripted_draws(hand, monkeypatch):
    table, keys, row_of, tabs = hand
    reads = []

    def read(tok, obs):
        reads.append((tok, obs))
        return np.zeros((4, 3), np.float32)                  # (exactly ns points: subsample_pc draws nothing)
    ds = LD.TrainPairs(table, read, subsample_sparse=4, shuffle=False)
    assert len(ds) == 10                                     # A0-A3, B0-B5: more than two usable observations
    K = 600
    for seed in (0, 0x1234567800000009):
        script = Script(table, seed)
        monkeypatch.setattr(np.random, "choice", script.choice)
        items = np.array([ds.idx[k % len(ds)] for k in range(K)], np.int32)
        rows, labels, ids, info, trace = SR.train_pairs(tabs, items, np.arange(K), seed=seed)
        assert info == 0
        for k in range(K):
            script.begin(table.objects[items[k]], k)
            del reads[:]
            it = ds[k % len(ds)]
            assert [row_of[r] for r in reads] == rows[k].tolist(), (seed, k)
            assert [it["label_1"], it["label_2"]] == labels[k].tolist(), (seed, k)
            assert [it["id_1"], it["id_2"]] == ids[k].tolist(), (seed, k)
        monkeypatch.undo()
        # every branch of the rule was taken (and compared above)
        neg = [t for t in trace if not t["positive"]]
        assert 200 < len(neg) < 400
        assert any(t["use_tp"] for t in neg) and any(not t["use_tp"] for t in neg)
        for pool in (True, False):
            mine = [t for t in neg if t["use_tp"] == pool]
            assert any(t["db"] < t["dens"] for t in mine)            # _class_list_density steps down
            assert any(t["db"] > t["dens"] for t in mine)            # ... wraps to the bottom and steps up
            assert any(t["db"] == t["dens"] for t in mine)
        assert max(t["attempts"] for t in neg) >= 2                  # the own-object rejection drew again
        assert (ids[:, 1] == -1).sum() > 50 and ((labels[:, 1] - labels[:, 0]) == 2).sum() == (ids[:, 1] == -1).sum()
        # a partner is drawn from the bucket's own candidate list, so it always holds an observation there: inside the
        # pair rule _frame_even's walk never moves (it is held to the host function on its own below)
        assert all(t["fb"] == t["db"] for t in neg)


def test_frame_walk_equals_frame_even_both_ways(hand, monkeypatch):
    """_frame_even on its own: stepping down to the nearest lower bucket, and wrapping to the lowest non-empty one"""
    table, keys, row_of, tabs = hand
    seen = set()
    for oi, o in enumerate(table.objects):
        off = tabs["bucket_off"][oi * SR.BUCKETS:(oi + 1) * SR.BUCKETS + 1]
        for d in range(SR.BUCKETS):
            got = []
            monkeypatch.setattr(np.random, "choice", lambda a, size, replace: (got.append(list(a)), np.asarray(a)[[0]])[1])
            first = LD._frame_even(o, d)
            monkeypatch.undo()
            fb = SR.walk(off, d, 1)
            assert got[0] == o["buckets"][PR.BUCKETS[fb]] and first == got[0][0]
            assert [keys[r] for r in tabs["bucket_rows"][off[fb]:off[fb + 1]]] == [(o["token"], n) for n in got[0]]
            seen.add("down" if fb < d else "up" if fb > d else "stay")
    assert seen == {"down", "up", "stay"}


def test_forced_retry_takes_the_first_other_entry(hand):
    """32 candidate picks that all hit the item's own object (words no generator would give): the first entry of the list
    that is not the own object, and the retry flag"""
    table, keys, row_of, tabs = hand
    a2 = [o["token"] for o in table.objects].index("A2")
    a3 = [o["token"] for o in table.objects].index("A3")
    rand = np.zeros((1, SR.PAIR_WORDS), np.uint32)            # coin 0: negative; observation 0
    rand[0, 2] = 0xFFFFFFFF                                  # density: the last observation's bucket (6: {A2, A3})
    rand[0, 3] = 0x80000000                                  # true pool
    rows, labels, ids, info, trace = SR.train_pairs(tabs, [a2], [0], rand=rand.view(np.int32))
    assert info == SR.INFO_RETRY and trace[0]["attempts"] == 32 and trace[0]["db"] == 6
    assert ids[0].tolist() == [a2, a3] and keys[rows[0, 1]][0] == "A3" and keys[rows[0, 0]] == ("A2", 0)


# ---- table construction ----
def test_tables_reproduce_the_object_table_entry_for_entry(hand):
    table, keys, row_of, t = hand
    toks = [o["token"] for o in table.objects]
    NB = SR.BUCKETS
    assert t["num_objects"] == 16 and t["num_classes"] == 2
    for i, o in enumerate(table.objects):
        assert (t["obj_cls"][i], bool(t["obj_fp"][i]), t["obj_id"][i]) == (o["cls"], bool(o.get("fp")), i)
        assert [keys[r] for r in t["nums_rows"][t["nums_off"][i]:t["nums_off"][i + 1]]] == [(o["token"], n) for n in o["nums"]]
        for b in range(NB):
            lo, hi = t["bucket_off"][i * NB + b], t["bucket_off"][i * NB + b + 1]
            assert [keys[r] for r in t["bucket_rows"][lo:hi]] == [(o["token"], n) for n in o["buckets"].get(PR.BUCKETS[b], [])]
    total = 0
    for p, pool in enumerate((table.tp, table.fp)):
        for c in range(2):
            for b in range(NB):
                lo, hi = t["pool_off"][(p * 2 + c) * NB + b], t["pool_off"][(p * 2 + c) * NB + b + 1]
                want = [tok for tok, _ in pool.get(c, {}).get(PR.BUCKETS[b], [])]
                assert [toks[i] for i in t["pool_objs"][lo:hi]] == want
                total += len(want)
    assert total == len(t["pool_objs"]) == 27           # 12 + 8 true, 4 + 3 false-positive entries, counted by hand
    assert all(v.dtype == np.int32 for v in t.values() if isinstance(v, np.ndarray))
    # an ids map is honoured
    t2 = ST.pair_tables(table, row_of, ids={tok: 100 + i for i, tok in enumerate(toks)})
    assert t2["obj_id"].tolist() == list(range(100, 116))


def test_construction_refuses_a_table_the_rule_could_raise_on():
    table = hand_table()
    objs = [dict(token=o["token"], cls=o["cls"], fp=bool(o.get("fp")), frames=o["frames"]) for o in table.objects
            if o["token"] != "F3"]                           # class 1 keeps one false positive: no bucket of two
    bad = PR.ObjectTable(objs, num_classes=2)
    _, row_of = rows_of(bad)
    with pytest.raises(ValueError, match=r"class 1 .* fp pool"):
        ST.pair_tables(bad, row_of)
    with pytest.raises(ValueError, match=r"class 1 .* fp pool"):
        ST.CropStore.from_arrays([np.zeros((o["frames"][n], 3), np.float32) for o in bad.objects for n in sorted(o["frames"])],
                                 keys=rows_of(bad)[0], device="cpu", table=bad)
    # the host rule does raise on it, at draw time
    with pytest.raises(ValueError):
        LD._class_list_density(bad.fp, 1, 4)
    # and a store on the CPU builds, packs and reports its footprint (the launches need the device)
    keys, _ = rows_of(table)
    st = ST.CropStore.from_arrays([np.ones((table.by_token[tok]["frames"][n], 3), np.float32) for tok, n in keys], keys=keys,
                                  device="cpu", table=table)
    assert st.offsets.tolist()[:3] == [0, 9, 19] and st.lengths.dtype.is_floating_point is False
    assert st.key_of[st.row_of[("A3", 5)]] == ("A3", 5)
    assert st.nbytes >= 12 * int(st.offsets[-1]) + 8 * len(st.offsets)
