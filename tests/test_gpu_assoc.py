"""GPU: compare_pairs / association_cost / linear_assignment / ReIDNet.associate against the numpy restatement
(tests/assoc_ref.py).  Every comparison with the restatement is bit for bit, the duals u and v included."""
import os

import numpy as np
import pytest
import torch

import assoc_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FILL = np.float32(10000.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the solver --------------------------------------------------------------------------------------------------
def float_case(Rr, C, seed):
    """reference-shaped: the augmented matrix itself where the shape is one ((T + D) square), otherwise N(0, 4^2) values
    with three entries in four at the fill value, as the class gate leaves them"""
    if Rr == C and Rr % 2 == 0:
        return R.reference_case(Rr // 2, Rr // 2, seed, classes=8 if Rr >= 100 else 4)[0]
    g = np.random.default_rng(seed)
    c = (g.standard_normal((Rr, C)) * 4).astype(np.float32)
    c[g.random((Rr, C)) < 0.75] = FILL
    return c


def anti_case(Rr, C):
    """c[i][j] = (i + 1)(j + 1): the optimum pairs the largest with the smallest (the anti-diagonal), and every search
    walks through the rows assigned so far"""
    return np.outer(np.arange(1, Rr + 1), np.arange(1, C + 1)).astype(np.float32)


SHAPES = [(1, 1), (1, 5), (5, 1), (63, 63), (64, 64), (65, 65), (17, 130), (130, 17), (200, 200), (400, 400)]
_solved = {}


def solved(key, make):
    """the restatement's answer for a matrix, computed once per module run"""
    if key not in _solved:
        c = make()
        _solved[key] = (c, R.lsa(c))
    return _solved[key]


def check_batch(problems):
    """problems: [(cost, restatement's (col4row, row4col, u, v, info))] of one shape -> one launch, every output compared"""
    from pcr_amd import associate as A
    cost = np.stack([p[0] for p in problems])
    col4row, row4col, info, u, v = A.linear_assignment(dev(cost), return_duals=True)
    plain = A.linear_assignment(dev(cost))
    torch.cuda.synchronize()
    assert col4row.dtype == torch.int32 and row4col.dtype == torch.int32 and info.dtype == torch.int32
    for b, (_, want) in enumerate(problems):
        assert int(info[b]) == want[4], "problem %d: info" % b
        assert np.array_equal(host(col4row[b]), want[0]), "problem %d: col4row" % b
        assert np.array_equal(host(row4col[b]), want[1]), "problem %d: row4col" % b
        assert same_bits(host(u[b]), want[2]), "problem %d: u" % b
        assert same_bits(host(v[b]), want[3]), "problem %d: v" % b
    assert torch.equal(plain[0], col4row) and torch.equal(plain[1], row4col) and torch.equal(plain[2], info)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_lsa_one_problem(shape):
    check_batch([solved(("float", shape, 1), lambda: float_case(*shape, seed=1))])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_lsa_batch_of_three_different_problems(shape):
    special = (("anti", shape), lambda: anti_case(*shape)) if SHAPES.index(shape) % 2 == 1 else \
        (("const", shape), lambda: np.full(shape, 2.5, np.float32))
    check_batch([solved(("int4", shape), lambda: R.integer_case(*shape, 4, seed=3)),      # ties in nearly every step
                 solved(*special),
                 solved(("float", shape, 2), lambda: float_case(*shape, seed=2))])


def test_lsa_anti_diagonal_and_constant_at_200():
    check_batch([solved(("anti", (200, 200)), lambda: anti_case(200, 200)),
                 solved(("const", (200, 200)), lambda: np.full((200, 200), 2.5, np.float32))])
    want = solved(("anti", (200, 200)), None)[1]
    assert np.array_equal(want[0], np.arange(200)[::-1])


def test_lsa_1024_integers():
    """16 columns per lane, rows read from global memory; integers in [0, 1024): exact sums, ties present"""
    check_batch([solved(("int1024", (1024, 1024)), lambda: R.integer_case(1024, 1024, 1024, seed=5))])


def test_lsa_fixture_cases():
    """the matrices scipy's answers are recorded for (tests/golden/assoc_lsa.npz), batched by shape"""
    z = np.load(os.path.join(GOLDEN, "assoc_lsa.npz"))
    by_shape = {}
    for i in range(len(z["kind"])):
        c = z["cost_%d" % i]
        by_shape.setdefault(c.shape, []).append((c, R.lsa(c), i))
    for shape, group in sorted(by_shape.items()):
        check_batch([(c, want) for c, want, _ in group])
        for c, want, i in group:
            if z["kind"][i] == 0:                         # the float cases: scipy's own assignment
                sc = np.full(shape[0], -1, np.int32)
                sc[z["rows_%d" % i]] = z["cols_%d" % i]
                assert np.array_equal(want[0], sc)


def test_lsa_non_finite_problems_are_reported_and_skipped():
    shape = (65, 65)
    good = [solved(("float", shape, s), lambda s=s: float_case(*shape, seed=s)) for s in (1, 2)]
    nan, inf = good[0][0].copy(), good[1][0].copy()
    nan[64, 3] = np.nan
    inf[0, 64] = np.inf
    none = (np.full(65, -1, np.int32), np.full(65, -1, np.int32), np.zeros(65, np.float32), np.zeros(65, np.float32), 1)
    assert R.lsa(nan)[4] == 1 and R.lsa(inf)[4] == 1
    check_batch([good[0], (nan, none), good[1], (inf, none)])


def test_lsa_empty_problems():
    from pcr_amd import associate as A
    for B, Rr, C in ((1, 0, 5), (2, 5, 0), (0, 4, 4), (1, 0, 0)):
        col4row, row4col, info, u, v = A.linear_assignment(torch.empty((B, Rr, C), device="cuda"), return_duals=True)
        assert tuple(col4row.shape) == (B, Rr) and tuple(row4col.shape) == (B, C) and tuple(info.shape) == (B,)
        assert bool((col4row == -1).all()) and bool((row4col == -1).all()) and bool((info == 0).all())
        assert tuple(u.shape) == (B, Rr) and tuple(v.shape) == (B, C)
    c4r, r4c, info = A.linear_assignment(dev(np.array([[3.0, 1.0], [1.0, 3.0]], np.float32)))      # 2-D: a batch of one
    assert host(c4r).tolist() == [[1, 0]] and host(r4c).tolist() == [[1, 0]] and host(info).tolist() == [0]


# ---- 2. the pair list -------------------------------------------------------------------------------------------------
def labels_case(T, D, seed):
    g = np.random.default_rng(seed)
    # below the range (-1), inside it, and above it (9; 3 too for three classes)
    values = np.array([-1, 0, 1, 2, 3, 9], np.int32)
    return (g.choice(values, T), g.choice(values, D),
            g.integers(0, 5, T).astype(np.int32), g.integers(0, 5, D).astype(np.int32))


@pytest.mark.parametrize("T,D", [(1, 1), (5, 7), (64, 64), (65, 200), (300, 257), (0, 9), (9, 0)])
@pytest.mark.parametrize("num_classes", [8, 3])
def test_pairs(T, D, num_classes):
    from pcr_amd import associate as A
    tl, dl, tn, dn = labels_case(T, D, seed=T * 1000 + D)
    if T == 1 and D == 1:
        tl[:], dl[:], tn[:], dn[:] = 2, 2, 2, 2
    for lengths in (False, True):
        a, b = (tn, dn) if lengths else (None, None)
        want, count = R.compare_pairs(tl, dl, a, b, min_points=2, num_classes=num_classes)
        da, db = (dev(tn), dev(dn)) if lengths else (None, None)
        pairs, cnt = A.compare_pairs(dev(tl), dev(dl), da, db, min_points=2, num_classes=num_classes)
        assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (T * D, 2) and tuple(cnt.shape) == (1,)
        assert int(cnt) == count and np.array_equal(host(pairs), want)
        assert count > 0 or T * D == 0
        # a capacity below the count: the true count, the first cap pairs; above it: (0, 0) padding
        for cap in sorted({0, count // 2, count, count + 5}):
            out = (torch.full((cap, 2), -7, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda"))
            got = A.compare_pairs(dev(tl), dev(dl), da, db, num_classes=num_classes, cap=cap, out=out)
            assert got[0] is out[0] and got[1] is out[1]
            wantc, _ = R.compare_pairs(tl, dl, a, b, num_classes=num_classes, cap=cap)
            assert int(out[1]) == count and np.array_equal(host(out[0]), wantc)
    # int64 labels and lengths are converted on the device
    pairs64, cnt64 = A.compare_pairs(dev(tl.astype(np.int64)), dev(dl.astype(np.int64)), dev(tn.astype(np.int64)),
                                     dev(dn.astype(np.int64)), num_classes=num_classes)
    assert torch.equal(pairs64, pairs) and torch.equal(cnt64, cnt)


def test_pairs_min_points_and_many_classes():
    from pcr_amd import associate as A
    g = np.random.default_rng(4)
    tl, dl = g.integers(0, 32, 130).astype(np.int32), g.integers(0, 32, 70).astype(np.int32)
    tn, dn = g.integers(0, 9, 130).astype(np.int32), g.integers(0, 9, 70).astype(np.int32)
    for mp in (0, 5, 9):
        want, count = R.compare_pairs(tl, dl, tn, dn, min_points=mp, num_classes=32)
        pairs, cnt = A.compare_pairs(dev(tl), dev(dl), dev(tn), dev(dn), min_points=mp, num_classes=32)
        assert int(cnt) == count and np.array_equal(host(pairs), want)


# ---- 3. the cost matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D", [(1, 1), (5, 7), (65, 200)])
def test_cost_every_element(T, D):
    from pcr_amd import associate as A
    g = np.random.default_rng(T + D)
    tl, dl, tn, dn = labels_case(T, D, seed=T + 17 * D)
    if T == 1:
        tl[:], dl[:], tn[:], dn[:] = 2, 2, 2, 2
    pairs, count = R.compare_pairs(tl, dl, tn, dn)
    assert 0 < count and (count < len(pairs) or T == 1)
    logits = (g.standard_normal(len(pairs)) * 4).astype(np.float32)
    logits[0] = 0.0                                                     # -0.0 in the matrix
    miss, new = g.standard_normal(T).astype(np.float32), g.standard_normal(D).astype(np.float32)
    dist = (g.random((T, D)) * 44).astype(np.float32)
    for use_dist in (False, True):
        for use_diag in (False, True):
            kw = dict(dist=dist if use_dist else None, track_miss=miss if use_diag else None, det_new=new if use_diag else None)
            want = R.association_cost(logits, pairs, count, T, D, fill=123.5, dist_max=20.0, dist_penalty=1.25, **kw)
            out = torch.full((T + D, D + T), float("nan"), device="cuda")           # poisoned: every element must be written
            got = A.association_cost(dev(logits), dev(pairs), dev(np.array([count], np.int32)), T, D, fill=123.5,
                                     dist_max=20.0, dist_penalty=1.25, out=out,
                                     **{k: None if a is None else dev(a) for k, a in kw.items()})
            assert got is out and same_bits(host(out), want)
    # the defaults are the reference's: fill 10000, 22 m, + 3; a count above the capacity lists the capacity
    got = A.association_cost(dev(logits), dev(pairs), dev(np.array([count], np.int32)), T, D, dist=dev(dist))
    assert same_bits(host(got), R.association_cost(logits, pairs, count, T, D, dist=dist))
    half = max(1, count // 2)
    got = A.association_cost(dev(logits[:half]), dev(pairs[:half]), dev(np.array([count], np.int32)), T, D)
    assert same_bits(host(got), R.association_cost(logits[:half], pairs[:half], count, T, D))


def test_cost_without_tracks_or_detections():
    from pcr_amd import associate as A
    none = dict(logits=torch.empty(0, device="cuda"), pairs=torch.empty((0, 2), dtype=torch.int32, device="cuda"),
                count=torch.zeros(1, dtype=torch.int32, device="cuda"))
    new = np.array([1.0, 2.0, 3.0], np.float32)
    got = host(A.association_cost(T=0, D=3, det_new=dev(new), **none))
    assert same_bits(got, R.association_cost(np.zeros(0, np.float32), np.zeros((0, 2), np.int32), 0, 0, 3, det_new=new))
    got = host(A.association_cost(T=3, D=0, track_miss=dev(new), **none))
    assert np.array_equal(np.diag(got), new) and (got[~np.eye(3, dtype=bool)] == 10000.0).all()
    assert tuple(A.association_cost(T=0, D=0, **none).shape) == (0, 0)


# ---- 4. end to end and capture ----------------------------------------------------------------------------------------
def test_associate_on_the_toy_model():
    import bench
    from pcr_amd import testing as PT
    T, D, n = 5, 7, 128
    model, _ = bench.build_pt_model([n, 64, 32])
    clouds = PT.synthetic_clouds(T + D, n, seed=21, kind="box").cuda()
    tl = torch.tensor([0, 1, 1, 9, 2], dtype=torch.int32, device="cuda")
    dl = torch.tensor([1, 0, 2, 1, 5, 0, 2], dtype=torch.int32, device="cuda")
    tn = torch.tensor([9, 9, 1, 9, 9], dtype=torch.int32, device="cuda")
    dn = torch.tensor([9, 9, 9, 9, 9, 0, 9], dtype=torch.int32, device="cuda")
    miss, new = torch.full((T,), 0.5, device="cuda"), torch.full((D,), -0.25, device="cuda")
    with torch.no_grad():
        xyz, h = model.forward_inference(clouds)
        out = model.associate(h[:T], xyz[:T], tl, tn, h[T:], xyz[T:], dl, dn, track_miss=miss, det_new=new)
        gallery_pairs = out["pairs"] + torch.tensor([0, T], dtype=torch.int32, device="cuda")
        logits = model.match_gallery(h, xyz, gallery_pairs)
    pairs, count = R.compare_pairs(host(tl), host(dl), host(tn), host(dn))
    assert count == 5 and int(out["count"]) == count and np.array_equal(host(out["pairs"]), pairs)
    assert [tuple(p) for p in pairs[:count].tolist()] == [(0, 1), (1, 0), (1, 3), (4, 2), (4, 6)]
    assert torch.equal(out["logits"].view(torch.int32), logits.view(torch.int32))
    cost = R.association_cost(host(out["logits"]), pairs, count, T, D, host(miss), host(new))
    assert same_bits(host(out["cost"]), cost)
    col4row, row4col, u, v, info = R.lsa(cost)
    t2d, d2t = R.decode(col4row, row4col, T, D)
    assert host(out["info"]).tolist() == [0]
    assert np.array_equal(host(out["track_to_det"]), t2d) and np.array_equal(host(out["det_to_track"]), d2t)
    for t, d in enumerate(t2d):                                     # mutually consistent, and only listed pairs are matched
        assert d == -1 or (d2t[d] == t and (t, d) in [tuple(p) for p in pairs[:count].tolist()])
    assert ((d2t >= 0).sum() == (t2d >= 0).sum()) and t2d[2] == -1 and t2d[3] == -1 and d2t[5] == -1
    # nothing to associate: all -1, and the model launches nothing
    with torch.no_grad():
        empty = model.associate(h[:0], xyz[:0], tl[:0], None, h[T:], xyz[T:], dl, None)
    assert tuple(empty["track_to_det"].shape) == (0,) and host(empty["det_to_track"]).tolist() == [-1] * D
    assert int(empty["count"]) == 0


def test_the_three_steps_in_one_captured_graph():
    from pcr_amd import associate as A
    T, D = 40, 50
    N = T + D

    def frame(seed):
        tl, dl, tn, dn = labels_case(T, D, seed)
        g = np.random.default_rng(seed)
        return tl, dl, tn, dn, (g.standard_normal(T * D) * 4).astype(np.float32)

    a, b = frame(1), frame(2)
    tl, dl, tn, dn, logits = [dev(x) for x in a]
    out_p = (torch.empty((T * D, 2), dtype=torch.int32, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"))
    out_c = torch.empty((N, N), device="cuda")
    out_l = (torch.empty((1, N), dtype=torch.int32, device="cuda"), torch.empty((1, N), dtype=torch.int32, device="cuda"),
             torch.empty((1,), dtype=torch.int32, device="cuda"), torch.empty((1, N), device="cuda"), torch.empty((1, N), device="cuda"))

    def steps(out_p, out_c, out_l):
        pairs, count = A.compare_pairs(tl, dl, tn, dn, out=out_p)
        cost = A.association_cost(logits, pairs, count, T, D, out=out_c)
        return A.linear_assignment(cost, return_duals=True, out=out_l)

    steps(out_p, out_c, out_l)                                      # warm: nothing is loaded or opted in inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # a device-to-host copy in here would fail the capture
        steps(out_p, out_c, out_l)
    for x, y in zip((tl, dl, tn, dn, logits), b):
        x.copy_(dev(y))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (*out_p, out_c, *out_l)]
    eager = steps((torch.empty_like(out_p[0]), torch.empty_like(out_p[1])), torch.empty_like(out_c),
                  tuple(torch.empty_like(t) for t in out_l))
    pairs, count = R.compare_pairs(b[0], b[1], b[2], b[3])
    cost = R.association_cost(b[4], pairs, count, T, D)
    want = R.lsa(cost)
    assert int(got[1]) == count and np.array_equal(host(got[0]), pairs) and same_bits(host(got[2]), cost)
    assert np.array_equal(host(got[3][0]), want[0]) and np.array_equal(host(got[4][0]), want[1]) and int(got[5]) == 0
    assert same_bits(host(got[6][0]), want[2]) and same_bits(host(got[7][0]), want[3])
    for g_, e in zip(got[3:], eager):
        assert torch.equal(g_.view(torch.int32), e.view(torch.int32))
    a_pairs, a_count = R.compare_pairs(a[0], a[1], a[2], a[3])
    assert a_count != count                                         # the two frames differ where it matters
