"""GPU: the identity metrics (include/pcr.h section A9, pcr_amd/identity.py, ReIDNet.track_step(truth=dict(identity=...)))
against the numpy restatement of tests/ident_ref.py.  Every table is compared bit for bit, the binary64 distance sums by
their bits; the assignment is pcr_lsa_f32's, whose total is exact on these integer matrices, so IDTP is also held against
scipy's totals (tests/golden/ident_lsa.npz).  id_map itself is not compared: ties are free."""
import functools

import numpy as np
import pytest
import torch

import ident_ref as R
import truth_ref as TRU

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_scene(got, want, where):
    for k in R.SCENE:
        assert same_bits(host(got[k]), want[k]), (where, k)


def gpu_scene(scene):
    return {k: dev(scene[k]) for k in R.SCENE}


def gpu_pool(pool):
    return dict(table=dev(pool["table"]), dist_total=dev(pool["dist_total"]))


def gpu_close(scene, pool, max_rows, max_cols):
    """compact, the assignment and score on explicit device tensors (scene, pool: dicts of device tensors; pool is added
    to) -> dict(counts, row_list, col_list, cost, col4row, id_map) on the host"""
    from pcr_amd import associate as A
    from pcr_amd import identity as ID
    gt_rows, id_cap = scene["cooc"].shape
    junk = lambda *shape: torch.full(shape, 77, dtype=torch.int32, device="cuda")      # every element must be written
    t = dict(scene, flags=junk(gt_rows + id_cap), counts=junk(4), row_list=junk(max_rows), col_list=junk(max_cols),
             cost=torch.full((max_rows, max_cols), 7.0, device="cuda"))
    ID.compact(t, gt_rows, id_cap, max_rows, max_cols)
    col4row, row4col, info = A.linear_assignment(t["cost"])
    out = {k: host(t[k]) for k in ("counts", "row_list", "col_list", "cost")}
    del t["flags"], t["cost"]
    t.update(col4row=col4row[0].contiguous(), info=info, id_map=junk(gt_rows), **pool)
    ID.score(t, gt_rows, id_cap, max_rows, max_cols)
    out.update(col4row=host(col4row[0]), id_map=host(t["id_map"]))
    return out


def close_both(scene_h, pool_h, max_rows, max_cols):
    """one scene closed on the device and by the restatement, compared -> (the new host pool, the device's outputs, idtp)"""
    pool_d = gpu_pool(pool_h)
    got = gpu_close(gpu_scene(scene_h), pool_d, max_rows, max_cols)
    pool_h, id_map, idtp, comp = R.close_scene(scene_h, pool_h, max_rows, max_cols)
    for k in ("counts", "row_list", "col_list", "cost"):
        assert same_bits(got[k], comp[k]), k
    assert same_bits(host(pool_d["table"]), pool_h["table"]) and same_bits(host(pool_d["dist_total"]), pool_h["dist_total"])
    # the map is not compared with the restatement's (two optima may map other rows): it is injective, names only pairs
    # with a positive count, and attains the total
    m = got["id_map"]
    named = m[m >= 0]
    assert len(set(named.tolist())) == len(named)
    cooc = scene_h["cooc"]
    assert sum(int(cooc[g, m[g]]) for g in np.flatnonzero(m >= 0)) == idtp
    assert all(cooc[g, m[g]] > 0 for g in np.flatnonzero(m >= 0))
    return pool_h, got, idtp


# ---- 1. the per-frame record --------------------------------------------------------------------------------------------------
# D and G cross the 64-lane word on both sides and take more than one wave's round of boxes (130 > 2 x 64); (1, 130) and
# (130, 1) are the degenerate sides
@pytest.mark.parametrize("D,G", [(1, 1), (63, 65), (64, 64), (65, 63), (130, 130), (1, 130), (130, 1)])
def test_record_equals_the_restatement(D, G):
    from pcr_amd import identity as ID
    seen = dict(twice=0, untracked=0, dropped_gt=0, dropped_id=0, wild_gt=0, tp=0)
    for gt_rows in (1, 64, 65, 300):
        for id_cap in (1, 65, 4096):
            gt_cap = gt_rows + 7                             # ids in [gt_rows, gt_cap) are valid and have no row
            stream = R.random_stream([D, G, gt_rows, id_cap], 12, D, G, gt_cap, gt_rows, id_cap)
            scene = gpu_scene(R.new_scene(gt_rows, id_cap))
            for f, (fr, want) in enumerate(stream):
                t = dict(scene, **{k: dev(v) for k, v in fr.items()})
                ID.record(t, gt_cap, gt_rows, id_cap)
                if f % 4 == 3:
                    assert_scene(scene, want, (gt_rows, id_cap, f))
                ok = (fr["gt_labels"] >= 0) & (fr["gt_ids"] >= 0) & (fr["gt_ids"] < gt_cap)
                ids = fr["gt_ids"][ok].tolist()
                seen["twice"] += len(ids) - len(set(ids))
                seen["wild_gt"] += int(((fr["det_gt"] < -1) | (fr["det_gt"] >= G)).sum())
                tp = (fr["det_labels"] >= 0) & (fr["det_gt"] >= 0) & (fr["det_gt"] < G)
                tp[tp] &= ok[fr["det_gt"][tp]]
                seen["untracked"] += int((tp & (fr["det_id"] < 0)).sum())
            tot = stream[-1][1]["totals"]
            assert tot[R.T_FRAMES] == 12
            seen["tp"] += int(tot[R.T_TP])
            seen["dropped_gt"] += int(tot[R.T_DROPPED_GT])
            seen["dropped_id"] += int(tot[R.T_DROPPED_ID])
    if min(D, G) >= 63:                                      # the streams hold what the rules must ignore
        assert all(v > 0 for v in seen.values()), seen
        assert stream[-1][1]["dist_sum"][0] > 0 and stream[-1][1]["gt_track"][:, R.FRAGS].sum() > 0


def test_record_refuses_what_pcr_ident_ok_refuses_and_takes_empty_sides():
    from pcr_amd import _lib as L
    from pcr_amd import identity as ID
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    scene = gpu_scene(R.new_scene(3, 4))
    empty = dict(det_labels=i32(0), det_gt=i32(0), det_id=i32(0), gt_labels=i32(0), gt_ids=i32(0), cost=torch.zeros(0, 0, device="cuda"))
    ID.record(dict(scene, **empty), 5, 3, 4)                 # D == G == 0: a frame all the same
    want = R.new_scene(3, 4)
    want["totals"][R.T_FRAMES] = 1
    assert_scene(scene, want, "empty")
    with pytest.raises(L.PcrError):
        ID.record(dict(scene, **empty), 5, 3, 5)             # cooc holds 12 elements, not 15
    with pytest.raises(L.PcrError):
        ID.record(dict(scene, **dict(empty, det_id=torch.zeros(0, dtype=torch.int64, device="cuda"))), 5, 3, 4)


# ---- 2. compaction ------------------------------------------------------------------------------------------------------------
EDGE_COLS = (0, 1, 63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4095)
EDGE_ROWS = (0, 63, 64, 65, 127, 128, 255, 256, 299)


def planted(rows, cols, gt_rows=300, id_cap=4096, seed=0):
    """a scene whose co-occurrence matrix has exactly these active rows and columns"""
    g = np.random.default_rng(seed)
    scene = R.new_scene(gt_rows, id_cap)
    rows, cols = np.asarray(rows), np.asarray(cols)
    for k in range(max(len(rows), len(cols))):               # every listed row and column gets a count
        scene["cooc"][rows[k % len(rows)], cols[k % len(cols)]] = g.integers(1, 30)
    for _ in range(3 * len(rows)):
        scene["cooc"][g.choice(rows), g.choice(cols)] = g.integers(1, 30)
    return scene


def test_compaction_across_word_wave_and_workgroup_boundaries():
    scene = planted(EDGE_ROWS, EDGE_COLS)
    pool, got, idtp = close_both(scene, R.new_pool(), 256, 512)
    assert got["row_list"][:len(EDGE_ROWS)].tolist() == list(EDGE_ROWS) and (got["row_list"][len(EDGE_ROWS):] == -1).all()
    assert got["col_list"][:len(EDGE_COLS)].tolist() == list(EDGE_COLS) and (got["col_list"][len(EDGE_COLS):] == -1).all()
    assert idtp > 0 and pool["table"][R.IX["overflow"]] == 0 and pool["table"][R.IX["inexact"]] == 0
    # a dense stretch: ranks beyond one chunk of 1024 flags, and more set flags in a chunk than a wave holds
    cols = np.arange(900, 1400)
    pool, got, idtp = close_both(planted(np.arange(100, 290), cols, seed=1), pool, 256, 512)
    assert got["counts"][:2].tolist() == [190, 500] and got["col_list"][:500].tolist() == cols.tolist() and idtp > 0


@pytest.mark.parametrize("side", ["cols", "rows"])
def test_overflow_is_flagged_one_past_the_cap_and_adds_no_idtp(side):
    cap = 12
    for n, over in ((cap, False), (cap + 1, True)):
        many = np.unique(np.concatenate([np.array(EDGE_ROWS if side == "rows" else EDGE_COLS)[:8], np.arange(60, 70)]))[:n]
        assert len(many) == n
        scene = planted(many, (3, 700)) if side == "rows" else planted((3, 200), many)
        max_rows, max_cols = (cap, 4) if side == "rows" else (4, cap)
        pool, got, idtp = close_both(scene, R.new_pool(), max_rows, max_cols)
        assert pool["table"][R.IX["overflow"]] == int(over) and (idtp == 0) == over
        assert got["counts"][R.N_ROWS if side == "rows" else R.N_COLS] == n
        if over:
            assert (got["cost"] == 0).all() and (got["id_map"] == -1).all()


def test_a_scene_without_a_pair_closes_clean():
    scene = R.new_scene(70, 130)
    scene["totals"][:4] = (5, 9, 0, 0)
    scene["gt_track"][[2, 69], R.PRESENT] = (5, 4)
    scene["gt_track"][[2, 69], R.CUR_GAP] = scene["gt_track"][[2, 69], R.LONGEST_GAP] = (5, 4)
    pool, got, idtp = close_both(scene, R.new_pool(), 8, 8)
    assert idtp == 0 and got["counts"].tolist() == [0, 0, 0, 0] and (got["row_list"] == -1).all() and (got["id_map"] == -1).all()
    m = R.metrics(pool["table"], pool["dist_total"][0])
    assert (m["tracks"], m["ml"], m["tid"], m["lgd"], m["idf1"]) == (2, 2, 4.5, 4.5, 0.0)


# ---- 3. closing a scene ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_file():
    from conftest import load_golden
    return load_golden("ident_lsa")


def test_idtp_equals_the_golden_totals_and_the_restatement():
    gold = golden_file()
    cases = R.golden_cases()
    assert [n for n, _ in cases] == gold["names"].tolist()
    for i, (name, cooc) in enumerate(cases):
        scene = R.new_scene(*cooc.shape)
        scene["cooc"] = cooc
        pool, got, idtp = close_both(scene, R.new_pool(), *cooc.shape)
        assert idtp == int(gold["total_%d" % i]) == int(pool["table"][R.IX["idtp"]]), name
        assert pool["table"][R.IX["inexact"]] == 0 and pool["table"][R.IX["overflow"]] == 0
    # the same through the default caps, the matrix standing inside a larger one
    big = R.new_scene(300, 4096)
    i = [n for n, _ in cases].index("diagonal_100_130")
    big["cooc"][np.ix_(np.arange(100) * 3, np.arange(130) * 31)] = cases[i][1]
    pool, got, idtp = close_both(big, R.new_pool(), 256, 512)
    assert idtp == int(gold["total_%d" % i])


def test_two_scenes_closed_one_after_the_other_pool_as_the_restatement():
    from pcr_amd import identity as ID
    D, G, gt_rows, id_cap, gt_cap = 65, 70, 65, 130, 72
    pool_h, pool_d = R.new_pool(), gpu_pool(R.new_pool())
    for s in range(2):
        stream = R.random_stream([s, 99], 8, D, G, gt_cap, gt_rows, id_cap)
        scene = gpu_scene(R.new_scene(gt_rows, id_cap))
        for fr, want in stream:
            ID.record(dict(scene, **{k: dev(v) for k, v in fr.items()}), gt_cap, gt_rows, id_cap)
        assert_scene(scene, stream[-1][1], s)
        gpu_close(scene, pool_d, 128, 160)
        pool_h, _, idtp, _ = R.close_scene(stream[-1][1], pool_h, 128, 160)
        assert idtp > 0
        assert same_bits(host(pool_d["table"]), pool_h["table"]) and same_bits(host(pool_d["dist_total"]), pool_h["dist_total"])
    t = pool_h["table"]
    assert t[R.IX["frames"]] == 16 and t[R.IX["frag"]] > 0 and t[R.IX["dropped_gt"]] > 0 and t[R.IX["dropped_id"]] > 0
    assert t[R.IX["mt"]] + t[R.IX["pt"]] + t[R.IX["ml"]] == t[R.IX["tracks"]] > 0 and pool_h["dist_total"][0] > 0


def test_a_large_count_sets_inexact():
    scene = planted((1, 5, 9), (2, 70, 300), gt_rows=16, id_cap=512)
    pool, got, idtp = close_both(scene, R.new_pool(), 3, 3)
    assert pool["table"][R.IX["inexact"]] == 0
    scene["cooc"][5, 70] = 1 << 22                            # (3 + 1) * 2^22 = 2^24: no longer below it
    pool, got, idtp = close_both(scene, pool, 3, 3)
    assert pool["table"][R.IX["inexact"]] == 1 and got["counts"][R.MAX_COUNT] == 1 << 22
    scene["cooc"][5, 70] = (1 << 22) - 1
    pool, got, idtp = close_both(scene, pool, 3, 3)
    assert pool["table"][R.IX["inexact"]] == 1                 # (the pooled flag counts the scenes that set it)


# ---- 4. the book, eager and from one captured graph -----------------------------------------------------------------------------
def test_a_scene_through_the_books_eager_and_replayed_from_one_graph():
    from pcr_amd import identity as ID
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    from test_gpu_truth import BOOK, FEAT, LIMIT, NMS_THRESH, sequence
    import track_ref as TR
    C, D, G, W = 26, 12, 12, 9
    sc, seq = sequence(C, D, G, W, 12, seed=3)
    bank = T.TrackBank(C, D, feat_shape=FEAT, box_width=W)
    book = TU.TruthBook(bank, G, sc.gt_cap, kind="centre", thresh=sc.thresh)
    ident = ID.IdentityBook(book, id_cap=256, max_rows=64, max_cols=256)
    assert ident.gt_rows == sc.gt_cap
    frame_keys = ("det_boxes", "det_labels", "det_scores", "gt_boxes", "gt_labels", "gt_ids", "gt_tte")
    own_keys = ("t2d", "d2t", "born", "kill", "lengths", "det_f", "det_x")
    S = {k: dev(seq[0]["fr"][k]) for k in frame_keys}
    S.update({k: dev(seq[0][k]) for k in own_keys})

    def load(s):
        for k in frame_keys:
            S[k].copy_(dev(s["fr"][k]))
        for k in own_keys:
            S[k].copy_(dev(s[k]))

    def step():
        book.match(S["det_boxes"], S["det_labels"], dict(boxes=S["gt_boxes"], labels=S["gt_labels"], ids=S["gt_ids"], tte=S["gt_tte"]))
        book.decide((S["t2d"], S["d2t"]), S["det_labels"], born=S["born"], kill=S["kill"])
        det_slot, det_id, info = bank.update(
            (S["t2d"], S["d2t"]), dict(labels=S["det_labels"], lengths=S["lengths"], boxes=S["det_boxes"], scores=S["det_scores"],
                                       feats=S["det_f"], xyz=S["det_x"]), born=S["born"], kill=S["kill"], frame_limit=LIMIT)
        bank.suppress(NMS_THRESH)
        book.record(det_slot, det_id)
        ident.record()                                       # (the det_id the book's record was given)
        return det_id

    def snapshot():
        return [host(getattr(ident, k)).copy() for k in R.SCENE] + [host(getattr(book, k)).copy() for k in BOOK] + \
               [host(getattr(bank, k)).copy() for k in TR.STATE]

    want, eager = R.new_scene(sc.gt_cap, 256), []
    for f, s in enumerate(seq):
        load(s)
        det_id = step()
        fr = s["fr"]
        cost = TRU.cost(fr["det_boxes"], fr["det_labels"], fr["gt_boxes"], fr["gt_labels"], fr["gt_ids"], sc.gt_cap)
        want = R.record(want, fr["det_labels"], s["truth"]["det_gt"], host(det_id), fr["gt_labels"], fr["gt_ids"], cost, sc.gt_cap)
        assert_scene({k: getattr(ident, k) for k in R.SCENE}, want, f)
        for k in BOOK:
            assert same_bits(host(getattr(book, k)), s["book"][k]), (f, k)
        eager.append(snapshot())
    assert want["cooc"].sum() > 20 and want["gt_track"][:, R.PRESENT].max() >= 10
    ident.close_scene()
    pool, _, idtp, _ = R.close_scene(want, R.new_pool(), 64, 256)
    assert same_bits(host(ident.table), pool["table"]) and same_bits(host(ident.dist_total), pool["dist_total"])
    assert all(int(host(getattr(ident, k)).astype(np.int64).sum()) == 0 for k in ("cooc", "gt_track", "totals"))     # reset
    m = ident.metrics()
    assert m == R.metrics(pool["table"], pool["dist_total"][0], fp=seq[-1]["book"]["stats"][TRU.FP])
    assert m["idtp"] == idtp > 0 and 0 < m["idf1"] <= 1 and m["frames"] == 12 and m["motp"] > 0
    # the same frames from ONE captured graph (the eager run above was the warm-up)
    bank.reset()
    book.reset()
    ident.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    load(seq[0])
    with torch.cuda.graph(graph):                            # a device-to-host copy in here would fail the capture
        step()
    bank.reset()
    book.reset()
    ident.reset()
    for f, s in enumerate(seq):
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(snapshot(), eager[f]):
            assert same_bits(a, b), f
    ident.close_scene()
    assert same_bits(host(ident.table), pool["table"]) and same_bits(host(ident.dist_total), pool["dist_total"])


# ---- 5. the whole frame on the toy model ----------------------------------------------------------------------------------------
def test_track_step_with_identity_changes_nothing_else_and_equals_the_restatement():
    from pcr_amd import _lib as L
    from pcr_amd import identity as ID
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    from test_gpu_truth import BOOK, LIMIT, NMS_THRESH, toy_model_and_frames
    C, D, M, W, n = 16, 8, 6, 9, 128
    model, frames = toy_model_and_frames(4, M, W, n)
    gt_ids = np.arange(M, dtype=np.int32) * 5 + 2
    runs = []
    with torch.no_grad():
        c0 = model.forward_inference_boxes(dev(frames[0][0]), dev(np.concatenate([frames[0][1], np.zeros((D - M, W), np.float32)])[:, :7].copy()), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])
        for with_identity in (False, True):
            bank = T.TrackBank(C, D, feat_shape=(64, n), box_width=W)
            book = TU.TruthBook(bank, D, 40)
            ident = ID.IdentityBook(book, id_cap=32, gt_rows=30, max_rows=16, max_cols=32) if with_identity else None
            want, got = R.new_scene(30, 32), []
            for f, (pts, boxes, labels, scores) in enumerate(frames):
                keep = [m for m in range(M) if f == 0 or m != f % M]            # an object missed: a gap in its track
                truth = dict(book=book, boxes=dev(boxes), labels=dev(labels), ids=dev(gt_ids), tte=dev(np.full(M, 3 - f, np.int32)))
                if with_identity:
                    truth["identity"] = ident
                out = model.track_step(bank, dev(pts), dev(boxes[keep]), dev(labels[keep]), dev(scores[keep]),
                                       crop_args=dict(seed=5 + f), frame_limit=LIMIT, suppress_threshold=NMS_THRESH, truth=truth)
                got.append(({k: host(v).copy() for k, v in out.items() if v is not None},
                            {k: host(v).copy() for k, v in bank.state().items()}, host(bank.feats).copy(),
                            {k: host(getattr(book, k)).copy() for k in BOOK}))
                if with_identity:
                    want = R.record(want, host(book._det_labels), host(out["det_gt"]), host(out["det_id"]), host(book.gt_labels),
                                    host(book.gt_ids), host(book.cost), book.gt_cap)
                    assert_scene({k: getattr(ident, k) for k in R.SCENE}, want, f)
            runs.append(got)
        assert want["totals"].tolist()[:4] == [4, 4 * M, 4 * M - 3, 4 * M - 3] and want["gt_track"][gt_ids, R.PRESENT].tolist() == [4] * M
        assert want["gt_track"][:, R.LONGEST_GAP].sum() == 3 and want["cooc"].sum() == 4 * M - 3
        ident.close_scene()
        pool, _, idtp, _ = R.close_scene(want, R.new_pool(), 16, 32)      # (every tracker id of the scene fits: ids < 32)
        assert same_bits(host(ident.table), pool["table"]) and same_bits(host(ident.dist_total), pool["dist_total"])
        assert ident.metrics()["idtp"] == idtp >= M and pool["table"][R.IX["overflow"]] == 0
        with pytest.raises(L.PcrError, match="identity"):    # a book of another TruthBook
            other = TU.TruthBook(bank, D, 40)
            model.track_step(bank, dev(frames[0][0]), dev(frames[0][1]), dev(frames[0][2]), dev(frames[0][3]),
                             truth=dict(truth, book=other))
    for (o0, st0, f0, b0), (o1, st1, f1, b1) in zip(*runs):
        assert sorted(o0) == sorted(o1)
        for k in o0:
            assert same_bits(o0[k], o1[k]), k
        for k in st0:
            assert same_bits(st0[k], st1[k]), k
        for k in b0:
            assert same_bits(b0[k], b1[k]), k
        assert same_bits(f0, f1)


def test_track_step_with_identity_replayed_from_one_graph_equals_the_eager_run():
    """model.track_step(truth=dict(identity=...)) itself, captured once and replayed over the scene with the frame's inputs
    copied into static buffers: the identity tables, the TruthBook and the bank after every frame equal the eager run's"""
    from pcr_amd import _lib as L
    from pcr_amd import identity as ID
    from pcr_amd import tracks as T
    from pcr_amd import truth as TU
    from test_gpu_truth import BOOK, LIMIT, NMS_THRESH, toy_model_and_frames
    C, D, M, W, n = 16, 8, 6, 9, 128
    model, frames = toy_model_and_frames(4, M, W, n)
    gt_ids = np.arange(M, dtype=np.int32) * 5 + 2
    bank = T.TrackBank(C, D, feat_shape=(64, n), box_width=W)
    book = TU.TruthBook(bank, D, 40)
    ident = ID.IdentityBook(book, id_cap=32, gt_rows=30, max_rows=16, max_cols=32)
    S = [dev(x) for x in frames[0]] + [dev(np.full(M, 3, np.int32))]             # sweep, boxes, labels, scores, tte
    ids = dev(gt_ids)

    def load(f):
        for dst, src in zip(S, frames[f] + (np.full(M, 3 - f, np.int32),)):
            dst.copy_(dev(src))

    def step():
        return model.track_step(bank, S[0], S[1], S[2], S[3], crop_args=dict(seed=5), frame_limit=LIMIT, suppress_threshold=NMS_THRESH,
                                truth=dict(book=book, identity=ident, boxes=S[1], labels=S[2], ids=ids, tte=S[4]))

    def snapshot():
        return [host(getattr(ident, k)).copy() for k in R.SCENE] + [host(getattr(book, k)).copy() for k in BOOK] + \
               [host(v).copy() for _, v in sorted(bank.state().items())]

    def reset():
        bank.reset()
        book.reset()
        ident.reset()

    with torch.no_grad():
        c0 = model.forward_inference_boxes(S[0], dev(np.concatenate([frames[0][1], np.zeros((D - M, W), np.float32)])[:, :7].copy()), seed=5)[0]
        model.calibrate_precision(c0[:D // 2], c0[D // 2:])
        eager = []
        for f in range(len(frames)):
            load(f)
            step()
            eager.append(snapshot())
        assert int(host(ident.totals)[R.T_TP]) == 4 * M and int(host(ident.cooc).sum()) >= M
        reset()
        with pytest.raises(L.PcrError, match="record follows"):                  # the book's reset forgot the last det_id
            ident.record()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        load(0)
        with torch.cuda.graph(graph):                        # a device-to-host copy in here would fail the capture
            step()
        reset()
        for f in range(len(frames)):
            load(f)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(snapshot(), eager[f]):
                assert same_bits(a, b), f
        ident.close_scene()
        m = ident.metrics()
        assert m["frames"] == 4 and m["gt_total"] == m["tp"] == 4 * M and 0 < m["idtp"] <= 4 * M
