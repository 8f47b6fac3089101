"""GPU parity of the neighbour search's candidate bound: for K > 32 the threshold tau comes from TWO
minima per lane (the lane's registers split into two fixed groups) instead of one.  Any valid tau gives the same output,
so every case compares `engine.knn_prefix` / `knn_prefix2` with the C oracle entry for entry; the shapes are the smallest
at which the two-group bound can go wrong: one register per group, a second group that is partly or wholly padding, both
group minima of a lane equal, both sides of the K gate in one launch, the LDS kernel, distances that overflow."""
import numpy as np
import pytest
import torch

from pcr_amd import testing as T
import point_ops as P

pytestmark = pytest.mark.gpu

B = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(xyz, s, k):
    from pcr_amd import engine
    want = P.knn_prefix(xyz, s, k)
    got = engine.knn_prefix(dev(xyz), s, k).cpu().numpy()
    assert (got == want).all()


def mirrored(n, seed, kind):
    """the second half of the cloud repeats the first: point i + n/2 = point i.  With n = 64 T that is register
    t + T/2 of every lane = its register t, so both group minima of a lane are equal for every query"""
    xyz = T.synthetic_clouds(B, n, seed=seed, kind=kind).numpy()
    xyz[:, n // 2:] = xyz[:, : n // 2]
    return xyz


@pytest.mark.parametrize("k", [33, 48, 64])
@pytest.mark.parametrize("kind", ["randn", "dup"])
def test_one_register_per_group(k, kind):
    check(T.synthetic_clouds(B, 128, seed=31 + k, kind=kind).numpy(), 128, k)


@pytest.mark.parametrize("n,k", [(65, 48), (70, 48), (100, 48), (64, 64), (48, 48)])
def test_second_group_partly_or_wholly_empty(n, k):
    """n <= 64: every lane's second minimum is a padding point's +inf, the bound must fall back to rank K-1 of the first;
    n = 65 / 70 / 100: one, six, 36 lanes have a second point"""
    for kind in ("randn", "dup"):
        check(T.synthetic_clouds(B, n, seed=n, kind=kind).numpy(), n, k)


@pytest.mark.parametrize("n,s,k,kind", [(256, 256, 48, "randn"), (1024, 128, 48, "box"), (1024, 128, 64, "dup"),
                                        (2048, 64, 48, "randn")])
def test_both_group_minima_equal(n, s, k, kind):
    check(mirrored(n, n + k, kind), s, k)


@pytest.mark.parametrize("n,s,k", [(128, 128, 48), (256, 256, 48), (1024, 128, 48), (1024, 128, 33), (2048, 64, 48)])
def test_lattice_span_4(n, s, k):
    """integer lattice of span 4 (64 sites): every distance is shared by many points, in both groups of most lanes, and
    far more than K points sit at or below the K-th distance"""
    g = np.random.default_rng(n + k)
    xyz = g.integers(0, 4, (B, n, 3)).astype(np.float32)
    xyz[1] *= np.float32(0.37)
    xyz[2, n // 2:] = xyz[2, : n // 2]
    check(xyz, s, k)


@pytest.mark.parametrize("n,s,k,s2,k2", [(128, 128, 32, 64, 48), (1024, 64, 32, 32, 48)])
def test_gate_both_sides_in_one_launch(n, s, k, s2, k2):
    from pcr_amd import engine
    for kind in ("randn", "dup"):
        xyz = T.synthetic_clouds(B, n, seed=n + k2, kind=kind).numpy()
        a, b = engine.knn_prefix2(dev(xyz), s, k, s2, k2)
        assert (a.cpu().numpy() == P.knn_prefix(xyz, s, k)).all()
        assert (b.cpu().numpy() == P.knn_prefix(xyz, s2, k2)).all()


@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("k", [48, 64])
@pytest.mark.parametrize("kind", ["randn", "dup"])
def test_lds_kernel(n, k, kind):
    check(T.synthetic_clouds(B, n, seed=n + k, kind=kind).numpy(), 64, k)


@pytest.mark.parametrize("n,far,k", [(128, 5, 48), (128, 90, 48), (1024, 990, 48), (2048, 2010, 64)])
def test_overflowing_distances(n, far, k):
    """`far` points have a coordinate of +-2e19: their squared distance to every ordinary point, and to the far points of
    the other sign or axis, overflows to +inf.  The oracle takes the first unused minimum under a strict `<`, so +inf
    distances are ranked by index; with n - far < K ordinary points every ordinary query's list ends in them"""
    g = np.random.default_rng(n + far)
    xyz = T.synthetic_clouds(B, n, seed=n + far, kind="randn").numpy()
    for b in range(B):
        rows = g.permutation(n)[:far]
        xyz[b, rows, g.integers(0, 3, far)] = np.float32(2e19) * g.choice(np.float32([-1, 1]), far)
    check(xyz, min(n, 128), k)
