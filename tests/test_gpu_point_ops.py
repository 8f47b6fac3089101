"""GPU parity: every point op of libpcr_hip.so (through the mmdet3d.ops API -> ctypes -> C ABI)
against the C oracle on the same seeded inputs.  Index outputs must be bit-exact."""
import numpy as np
import pytest
import torch

from pcr_amd import testing as T
import point_ops as P

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ops():
    from mmdet3d import ops as O
    return O


@pytest.mark.parametrize("n,m,kind", [(64, 16, "randn"), (100, 40, "box"), (128, 64, "dup"), (256, 256, "dup"),
                                      (1024, 512, "randn"), (1024, 128, "dup"), (3000, 64, "box"),
                                      (4096, 256, "dup"), (5000, 33, "randn"), (17, 17, "randn"), (1, 1, "randn")])
def test_fps_bit_exact(ops, n, m, kind):
    xyz = T.synthetic_clouds(3, n, seed=n + m, kind=kind).numpy()
    want = P.fps(xyz, m)
    got = ops.furthest_point_sample(dev(xyz), m).cpu().numpy()
    assert got.dtype == np.int32 and (got == want).all()


def _tie_clouds(n, kind):
    if kind == "lattice3":     # 27 sites: from pick 28 on every running minimum is 0 and the tie rule alone decides
        return np.random.default_rng(n).integers(0, 3, (3, n, 3)).astype(np.float32)
    return T.synthetic_clouds(3, n, seed=n, kind=kind).numpy()


@pytest.mark.parametrize("n,m,kind,r,k", [(1024, 1024, "lattice3", 0.5, 64), (600, 600, "lattice3", 1.1, 32),
                                          (1024, 512, "dup", 0.2, 32)])
def test_fps_tie_rule_of_the_wave_kernels_against_the_oracle(ops, n, m, kind, r, k):
    """The >= 8-pair wave kernels (513-1024 points; n = 600 with padding lanes) where the reference's tie rule decides
    practically every pick -- pcr_fps_f32 and the fused pcr_fps_ball_query_rows_f32 each against the C ORACLE (the fused
    kernel is otherwise only compared with the separate launches, which share its pick helpers): the pick order, and the
    hit counts against the oracle's ball query of the oracle's centres."""
    from mmdet3d.ops import point_ops as PO
    xyz = _tie_clouds(n, kind)
    want = P.fps(xyz, m)
    got = ops.furthest_point_sample(dev(xyz), m).cpu().numpy()
    assert (got == want).all()
    assert PO.fps_ball_query_rows_ok(n, m, k)
    idx, new_xyz, cnt, _ = PO.fps_ball_query_rows(dev(xyz), m, r, k)
    assert (idx.cpu().numpy() == want).all()
    centres = np.take_along_axis(xyz, want[:, :, None].astype(np.int64), 1)
    assert (new_xyz.cpu().numpy() == centres).all()
    rows = P.ball_query(0.0, r, k, xyz, centres)
    # a row of the oracle: its hits in increasing index order, then copies of the first -> the count is where it stops rising
    rising = np.concatenate([np.ones((3, m, 1), bool), rows[:, :, 1:] > rows[:, :, :-1]], 2)
    want_cnt = np.where(rising.all(2), k, rising.argmin(2))
    assert (cnt.cpu().numpy() == want_cnt).all()


@pytest.mark.parametrize("n,s,k", [(1024, 64, 48), (2048, 64, 48), (4096, 64, 64)])
def test_knn_prefix_overflow_fallbacks_bit_exact(n, s, k):
    """More than kKnnCap = 256 candidates per query: the K-round fallbacks of the register kernel (n = 1024) and of the LDS
    kernel, the one part of both that the shared ranking does not serve.  Every point sits on one of two sites, so each
    query has hundreds of points AT its K-th distance (checked below) and the index decides."""
    from pcr_amd import engine
    from test_oracle_ops import two_site_clouds
    xyz = two_site_clouds(n, k)
    d = xyz[:, :s, None, :] - xyz[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    kth = np.partition(d2, k - 1, axis=2)[:, :, k - 1]
    assert ((d2 <= kth[:, :, None]).sum(2) > 256).all()
    want = P.knn_prefix(xyz, s, k)
    got = engine.knn_prefix(dev(xyz), s, k).cpu().numpy()
    assert (got == want).all()


def test_fps_with_dist_bit_exact(ops):
    g = np.random.default_rng(3)
    for n, m in ((96, 32), (300, 77), (1500, 20)):
        f = g.standard_normal((2, n, 8)).astype(np.float32)
        d = ((f[:, :, None] - f[:, None]) ** 2).sum(-1).astype(np.float32)
        d[0, :, : n // 3] = np.round(d[0, :, : n // 3], 1)        # force exact ties
        want = P.fps_dist(d, m)
        got = ops.furthest_point_sample_with_dist(dev(d), m).cpu().numpy()
        assert (got == want).all()


@pytest.mark.parametrize("n,m,k,r0,r1,kind", [(1024, 512, 32, 0.0, 0.2, "box"), (1024, 512, 32, 0.0, 0.6, "randn"),
                                              (2500, 300, 64, 0.1, 0.5, "dup"), (50, 50, 8, 0.0, 0.01, "randn"),
                                              (128, 128, 16, 0.0, 100.0, "dup"), (300, 77, 20, 0.0, 0.8, "randn"),
                                              (512, 128, 64, 0.0, 0.4, "box"), (1000, 130, 70, 0.05, 0.9, "dup")])
def test_ball_query_bit_exact(ops, n, m, k, r0, r1, kind):
    xyz = T.synthetic_clouds(2, n, seed=5, kind=kind).numpy()
    c = xyz[:, :m].copy()
    c[:, ::7] += 0.05
    want = P.ball_query(r0, r1, k, xyz, c)
    got = ops.ball_query(r0, r1, k, dev(xyz), dev(c)).cpu().numpy()
    assert (got == want).all()


@pytest.mark.parametrize("n,m,k,r1,kind", [(1024, 512, 32, 0.2, "box"), (300, 77, 20, 0.8, "randn"),
                                           (1500, 64, 16, 0.3, "dup")])
def test_ball_query_cnt_counts_genuine_hits(ops, n, m, k, r1, kind):
    from mmdet3d.ops import ball_query_cnt
    xyz = T.synthetic_clouds(2, n, seed=6, kind=kind).numpy()
    c = xyz[:, :m].copy()
    c[:, ::5] += 0.03
    idx, cnt = ball_query_cnt(0.0, r1, k, dev(xyz), dev(c))
    assert (idx.cpu().numpy() == P.ball_query(0.0, r1, k, xyz, c)).all()
    d = c[:, :, None, :] - xyz[:, None, :, :]                      # float32, same operation order as the kernel
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    want = np.minimum(((d2 == 0) | (d2 < np.float32(r1) * np.float32(r1))).sum(-1), k)
    assert (cnt.cpu().numpy() == want).all()


@pytest.mark.parametrize("n,m,k,kind", [(256, 100, 16, "randn"), (1000, 70, 100, "dup"), (128, 128, 1, "box"),
                                        (64, 64, 64, "dup")])
def test_knn_heap_bit_exact(ops, n, m, k, kind):
    xyz = T.synthetic_clouds(2, n, seed=9, kind=kind).numpy()
    c = xyz[:, :m].copy()
    want, _ = P.knn(k, xyz, c)
    got = ops.knn(k, dev(xyz), dev(c), False).cpu().numpy()       # (B,k,m)
    assert got.shape == (2, k, m)
    assert (got.transpose(0, 2, 1) == want).all()
    got_t = ops.knn(k, dev(xyz.transpose(0, 2, 1).copy()), dev(c.transpose(0, 2, 1).copy()), True).cpu().numpy()
    assert (got_t == got).all()
    with pytest.raises(RuntimeError):
        ops.knn(101, dev(xyz), dev(c), False)


@pytest.mark.parametrize("n,s,k,kind", [(128, 128, 32, "randn"), (128, 64, 48, "dup"), (512, 256, 48, "box"),
                                        (1024, 1024, 32, "dup"), (4096, 100, 48, "randn"), (70, 70, 64, "dup"),
                                        (2048, 33, 5, "box"), (4096, 64, 32, "dup"), (3000, 50, 16, "box"),
                                        (2500, 40, 64, "dup"), (1024, 512, 48, "randn"), (1024, 1024, 48, "box"),
                                        (1000, 700, 40, "randn"), (300, 300, 64, "randn"), (640, 640, 33, "dup"),
                                        (256, 256, 48, "randn"), (1024, 1024, 64, "randn"), (90, 90, 48, "randn")])
def test_knn_prefix_bit_exact(n, s, k, kind):
    from pcr_amd import engine
    xyz = T.synthetic_clouds(3, n, seed=21, kind=kind).numpy()
    want = P.knn_prefix(xyz, s, k)
    got = engine.knn_prefix(dev(xyz), s, k).cpu().numpy()
    assert (got == want).all()


@pytest.mark.parametrize("n,k,span", [(1024, 32, 40), (1024, 48, 12), (512, 32, 6), (1024, 32, 3), (700, 64, 25),
                                      (128, 32, 9), (4096, 32, 30), (2048, 48, 14), (3000, 16, 5)])
def test_knn_prefix_lattice_ties_bit_exact(n, k, span):
    """Integer lattice clouds: many EXACTLY equal distances (the index decides) and duplicates -- the truncated
    32-bit ranking must notice every tie among the first K + 1 ranks and take the exact 64-bit sort (few
    distinct distances), and the wider spans mix tie-free and tied queries in one launch.  Clouds above 1024 points run
    the LDS kernel, whose candidates reach the ranking in lane-major order with recomputed distances (round 5)."""
    from pcr_amd import engine
    g = np.random.default_rng(n + k + span)
    xyz = g.integers(0, span, (3, n, 3)).astype(np.float32)
    xyz[1] *= np.float32(0.37)          # non-representable steps: ties survive, rounding differs per axis
    xyz[2] += g.standard_normal((n, 3)).astype(np.float32) * np.float32(1e-6)   # near-ties within a few ulps
    want = P.knn_prefix(xyz, n, k)
    got = engine.knn_prefix(dev(xyz), n, k).cpu().numpy()
    assert (got == want).all()


@pytest.mark.parametrize("n,s,k,s2,k2,kind", [(1024, 1024, 32, 512, 48, "randn"), (4096, 4096, 32, 2048, 48, "box"),
                                              (128, 128, 32, 64, 48, "dup"), (700, 700, 16, 300, 64, "randn"),
                                              (2048, 2048, 48, 1024, 48, "dup"), (512, 400, 8, 400, 33, "box"),
                                              (3000, 2500, 20, 1, 64, "dup"), (256, 256, 32, 0, 48, "randn")])
def test_knn_prefix2_equals_two_searches(n, s, k, s2, k2, kind):
    """pcr_knn_prefix2_f32 (ABI 15): one launch for two set-abstraction levels on the same cloud -- the first s2 queries are
    ranked once for k2 >= k neighbours and write both lists.  Both outputs must equal what two pcr_knn_prefix_f32 launches
    write, entry for entry: random / box / duplicate-heavy clouds (the overflow paths), every kernel size class, s2 = 0 / 1 /
    s, k2 = k."""
    from pcr_amd import engine
    xyz = T.synthetic_clouds(3, n, seed=n + k2, kind=kind).cuda().contiguous()
    g = np.random.default_rng(n)
    lat = torch.from_numpy(g.integers(0, 6, (2, n, 3)).astype(np.float32)).cuda()   # lattice: exact ties everywhere
    for cloud in (xyz, lat):
        a, b = engine.knn_prefix2(cloud, s, k, s2, k2)
        assert torch.equal(a, engine.knn_prefix(cloud, s, k))
        if s2:
            assert torch.equal(b, engine.knn_prefix(cloud, s2, k2))
        else:
            assert b.shape == (cloud.shape[0], 0, k2)


def test_gather_group_fwd_bwd(ops):
    g = np.random.default_rng(0)
    feat = g.standard_normal((3, 19, 257)).astype(np.float32)
    idx = g.integers(0, 257, (3, 100)).astype(np.int32)
    f = dev(feat).requires_grad_(True)
    out = ops.gather_points(f, dev(idx))
    assert (out.detach().cpu().numpy() == P.gather_fwd(feat, idx)).all()
    go = g.standard_normal(out.shape).astype(np.float32)
    out.backward(dev(go))
    # owner-computes scatter: every accumulator adds its entries in index order, exactly like the oracle's loops
    assert np.array_equal(f.grad.cpu().numpy(), P.gather_bwd(go, idx, 257))

    gi = g.integers(0, 257, (3, 40, 12)).astype(np.int32)
    f = dev(feat).requires_grad_(True)
    out = ops.grouping_operation(f, dev(gi))
    assert (out.detach().cpu().numpy() == P.group_fwd(feat, gi)).all()
    go = g.standard_normal(out.shape).astype(np.float32)
    out.backward(dev(go))
    assert np.array_equal(f.grad.cpu().numpy(), P.group_bwd(go, gi, 257))
    first = f.grad.clone()
    f.grad = None
    ops.grouping_operation(f, dev(gi)).backward(dev(go))
    assert torch.equal(first, f.grad)                      # no float atomics: bit-identical from run to run


def test_three_nn_and_interpolate(ops):
    g = np.random.default_rng(1)
    unk = T.synthetic_clouds(2, 700, seed=3, kind="dup").numpy()
    kn = unk[:, :90].copy()
    d2, i3 = P.three_nn(unk, kn)
    dist, idx = ops.three_nn(dev(unk), dev(kn))
    assert (idx.cpu().numpy() == i3).all()
    assert np.allclose(dist.cpu().numpy(), np.sqrt(d2), rtol=1e-6, atol=0)
    w = g.uniform(size=(2, 700, 3)).astype(np.float32)
    feat = g.standard_normal((2, 13, 90)).astype(np.float32)
    f = dev(feat).requires_grad_(True)
    out = ops.three_interpolate(f, idx, dev(w))
    assert (out.detach().cpu().numpy() == P.three_interp_fwd(feat, i3, w)).all()
    go = g.standard_normal(out.shape).astype(np.float32)
    out.backward(dev(go))
    assert np.array_equal(f.grad.cpu().numpy(), P.three_interp_bwd(go, i3, w, 90))


def test_errors_are_python_exceptions(ops):
    x = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError):
        ops.furthest_point_sample(x, 4)                 # CPU tensor: no fallback
    with pytest.raises(AssertionError):
        ops.furthest_point_sample(torch.zeros(2, 3, 8).cuda().transpose(1, 2), 4)   # non-contiguous
    with pytest.raises(AssertionError):
        ops.ball_query(0.5, 0.2, 4, x.cuda(), x.cuda())  # min_radius >= max_radius


# ---- Python-semantic twins of the model path (pointnet2_utils.py:116-137, 218-240) ----
def test_python_twins_match_reference_golden():
    """farthest_point_sample (start index 0) and query_ball_point recorded from the imported reference"""
    from conftest import load_golden
    from mmdet3d.models import pointnet2_utils as U
    g = load_golden("ops_python_twins")
    m = g["meta"]
    xyz = T.synthetic_clouds(m["clouds"], m["n"], seed=m["seed"], kind=m["kind"]).cuda()
    fps = U.farthest_point_sample(xyz, m["m"], start=torch.zeros(m["clouds"], dtype=torch.long))
    assert fps.dtype == torch.int64 and (fps.cpu().numpy() == g["fps"]).all()
    centres = U.index_points(xyz, fps)
    ball = U.query_ball_point(m["radius"], m["nsample"], xyz, centres)
    assert (ball.cpu().numpy() == g["ball"]).all()
    knn = U.knn_point(m["nsample"], xyz, centres)
    assert (np.sort(knn.cpu().numpy(), -1) == g["knn_sorted"]).all()
    assert torch.equal(U.random_point_sample(xyz, 7).cpu(), torch.arange(7).repeat(m["clouds"], 1))


@pytest.mark.parametrize("B,N,M,kind", [(3, 300, 77, "box"), (2, 1024, 256, "randn"), (4, 128, 128, "dup"), (2, 5000, 64, "box")])
def test_python_fps_twin_matches_oracle_with_random_starts(B, N, M, kind):
    import model_oracle as MO
    from mmdet3d.models import pointnet2_utils as U
    xyz = T.synthetic_clouds(B, N, seed=21, kind=kind)
    start = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(4))
    got = U.farthest_point_sample(xyz.cuda(), M, start=start).cpu()
    want = MO.farthest_point_sample_py(xyz, M, start)
    assert torch.equal(got, want)
    # without `start` the first pick is drawn at random, as in the reference: valid indices, first column varies
    r = U.farthest_point_sample(xyz.cuda(), 4)
    assert r.shape == (B, 4) and int(r.min()) >= 0 and int(r.max()) < N


@pytest.mark.parametrize("B,N,S,K,radius,kind", [(2, 400, 100, 16, 0.5, "box"), (3, 256, 64, 32, 0.8, "randn"),
                                                  (2, 1500, 200, 8, 0.3, "dup"), (1, 64, 64, 64, 100.0, "box")])
def test_python_ball_query_twin_matches_oracle(B, N, S, K, radius, kind):
    """rows whose decision could flip with the summation order of the reference's matmul (a distance within 1e-5 of
    r^2) are left out of the comparison; everything else must be identical"""
    import model_oracle as MO
    from mmdet3d.models import pointnet2_utils as U
    xyz = T.synthetic_clouds(B, N, seed=22, kind=kind)
    new_xyz = xyz[:, :S].contiguous()
    got = U.query_ball_point(radius, K, xyz.cuda(), new_xyz.cuda()).cpu()
    want, d = MO.query_ball_point_py(radius, K, xyz, new_xyz, return_dist=True)
    safe = ((d - radius ** 2).abs() > 1e-5 * max(1.0, radius ** 2)).all(dim=-1)
    assert safe.float().mean() > 0.9
    assert torch.equal(got[safe], want[safe])


def test_hip_ops_equal_the_simulated_execution_of_the_cuda_kernels(ops):
    """tests/golden/ops_cuda_semantics.npz (oracle/cuda_sim.py: the .cu kernels' block / tid loops simulated thread by
    thread, independent of the C oracle): exact ties, N = 12 / 100 / 3000, points at exactly r, d2 == 0 below min_r, heaps
    of equal distances, fewer than three known points -- the HIP ops must reproduce every index (and every squared
    distance) bit for bit.  VERDICT r5 next 9a."""
    from test_oracle_ops import _cuda_cases, run_cuda_case

    def knn(k, xyz, c):
        idx = ops.knn(k, dev(xyz), dev(c), False).cpu().numpy().transpose(0, 2, 1)      # (B,k,M) -> (B,M,k)
        # the op returns indices only (KNN.forward, knn.py:16-64); the distances of the golden follow from them
        d = np.take_along_axis(xyz[:, None, :, :].repeat(c.shape[1], 1), idx[..., None].astype(np.int64).repeat(3, -1), 2) \
            - c[:, :, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        return np.ascontiguousarray(idx), d2.astype(np.float32)

    def three_nn(unk, kn):
        dist, idx = ops.three_nn(dev(unk), dev(kn))
        return (dist * dist).cpu().numpy(), idx.cpu().numpy()      # (sqrt of dyadic squares: exact both ways; inf stays inf)
    g, meta = _cuda_cases()
    for name, m in meta.items():
        pairs = run_cuda_case(
            name, m, g,
            lambda xyz, mm: ops.furthest_point_sample(dev(xyz), mm).cpu().numpy(),
            lambda dist, mm: ops.furthest_point_sample_with_dist(dev(dist), mm).cpu().numpy(),
            lambda lo, hi, k, xyz, c: ops.ball_query(lo, hi, k, dev(xyz), dev(c)).cpu().numpy(),
            knn, three_nn)
        for got, want in pairs:
            if name.startswith("nn3") and want.dtype == np.float32:
                assert np.allclose(got, want, rtol=2e-7, atol=0) and (np.isinf(got) == np.isinf(want)).all(), name
            else:
                assert got.dtype == want.dtype and np.array_equal(got, want), name
