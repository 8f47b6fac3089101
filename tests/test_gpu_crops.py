"""GPU: points_in_boxes_batch / points_in_boxes_gpu / crops_from_boxes / forward_inference_boxes against the numpy
restatement (tests/crops_ref.py) fed with the table pcr_box_frames_f32 returned for the same boxes: every comparison of
an op's output is bit for bit."""
import numpy as np
import pytest
import torch

import crops_ref as R

pytestmark = pytest.mark.gpu

SCENES = {"scene52k": (30000, 100, 1), "scene294k": (250000, 200, 2)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def scenes():
    out = {k: R.make_scene(*v) for k, v in SCENES.items()}
    assert out["scene52k"][0].shape[0] == 52022 and out["scene294k"][0].shape[0] == 294227
    return out


def frames_of(boxes):
    from pcr_amd import crops
    return host(crops.box_frames(dev(boxes)))


def gravity(boxes):
    b = boxes.copy()
    b[:, 2] = R.box_cz(boxes)
    return b


# ---- 3. the two membership ops ------------------------------------------------------------------------------------
def _check_membership(points, boxes):
    from mmdet3d import ops
    B = points.shape[0]
    frames = np.stack([frames_of(boxes[b]) for b in range(B)]) if boxes.shape[1] else np.zeros((B, 0, 2), np.float32)
    got_b = ops.points_in_boxes_batch(dev(points), dev(boxes))
    got_g = ops.points_in_boxes_gpu(dev(points), dev(boxes))
    assert got_b.dtype == torch.int32 and got_g.dtype == torch.int32
    assert tuple(got_b.shape) == (B, points.shape[1], boxes.shape[1]) and tuple(got_g.shape) == points.shape[:2]
    want_b = R.points_in_boxes_batch(points, boxes, frames)
    assert np.array_equal(host(got_b), want_b)
    assert np.array_equal(host(got_g), R.points_in_boxes_gpu(points, boxes, frames))
    return want_b


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("B", [1, 3])
def test_points_in_boxes_on_scenes(name, B, scenes):
    nbg, nb, seed = SCENES[name]
    batch = [scenes[name]] + [R.make_scene(nbg, nb, seed + 10 * b) for b in range(1, B)]
    m = _check_membership(np.stack([p for p, _ in batch]), np.stack([b for _, b in batch]))
    assert m.sum() > 1000 and (m.sum(axis=2) > 1).any()          # there is something in the boxes, some of it twice


@pytest.mark.parametrize("B", [1, 3])
def test_points_in_boxes_on_hand_made_cases(B):
    pts, boxes, counts = R.hand_scene(100)
    assert pts.shape[0] % 64 != 0
    m = _check_membership(np.stack([pts] * B), np.stack([np.roll(boxes, b, axis=0) for b in range(B)]))
    assert np.array_equal(m[0].sum(axis=0), counts)
    _check_membership(pts[None, :1], boxes[None])                 # P == 1
    _check_membership(pts[None, :257], boxes[None, :0])           # T == 0: nothing holds a point
    # 300 boxes: more than one LDS tile of the first-box kernel, the holder sits in the second tile
    many = np.concatenate([np.repeat(boxes[:1], 290, axis=0), boxes, boxes[:2]])
    g = _check_membership(pts[None], many[None])
    assert g[0].any()


# ---- 4. the fused crop ----------------------------------------------------------------------------------------------
def _check_crops(points, boxes, n, seed=7, combos=None):
    from pcr_amd import crops
    M = boxes.shape[0]
    frames = frames_of(boxes) if M else np.zeros((0, 2), np.float32)
    g = np.random.default_rng([n, M, seed])
    rand = g.integers(0, 1 << 32, (M, n), dtype=np.uint64).astype(np.uint32).view(np.int32)
    dp, drand = dev(points), dev(rand)
    seed_t = torch.tensor([seed], dtype=torch.int64, device="cuda")
    lengths = None
    for zc in (False, True):
        bx = gravity(boxes) if zc else boxes
        db = dev(bx)
        cache = {}
        for frame in ("sensor", "centred", "box"):
            for rule in ("tracker", "dataset"):
                for use_rand in (True, False):
                    if combos is not None and (zc, frame, rule, use_rand) not in combos:
                        continue
                    kw = dict(frame=frame, rule=rule, z_is_centre=zc)
                    if use_rand:
                        got = crops.crops_from_boxes(dp, db, n, rand=drand, **kw)
                        want = R.crop_boxes(points, bx, n, rand=rand, frames=frames, cache=cache, **kw)
                    else:
                        got = crops.crops_from_boxes(dp, db, n, seed=seed_t, **kw)
                        want = R.crop_boxes(points, bx, n, seed=seed, frames=frames, cache=cache, **kw)
                    assert tuple(got[0].shape) == (M, n, 3) and got[0].dtype == torch.float32
                    assert tuple(got[1].shape) == (M,) and got[1].dtype == torch.int32
                    assert np.array_equal(host(got[1]), want[1]), (zc, frame, rule, use_rand)
                    assert np.array_equal(host(got[0]).view(np.uint32), want[0].view(np.uint32)), (zc, frame, rule, use_rand)
                    lengths = want[1]
        again = crops.crops_from_boxes(dp, db, n, seed=seed_t, frame="box")
        again2 = crops.crops_from_boxes(dp, db, n, seed=seed_t, frame="box")
        assert torch.equal(again[0].view(torch.int32), again2[0].view(torch.int32)) and torch.equal(again[1], again2[1])
    return lengths


@pytest.mark.parametrize("name", sorted(SCENES))
def test_crops_on_scenes(name, scenes):
    points, boxes = scenes[name]
    lengths = _check_crops(points, boxes, 128)
    assert lengths.min() < 128 and lengths.max() > 1000
    if name == "scene52k":
        # a (P, 5) sweep: only xyz is read; n not a multiple of 64; n larger than most boxes hold
        sweep = np.concatenate([points, np.full((points.shape[0], 2), np.nan, np.float32)], axis=1)
        _check_crops(sweep, boxes, 200, combos={(False, "box", "tracker", False), (True, "sensor", "dataset", True)})
        _check_crops(points, boxes[:16], 1024, combos={(False, "box", "tracker", True), (False, "centred", "dataset", False)})


def test_crops_on_hand_made_cases():
    from pcr_amd import crops
    n = 100                                                       # not a multiple of 64
    pts, boxes, counts = R.hand_scene(n)
    sweep = np.concatenate([pts, np.zeros((pts.shape[0], 2), np.float32)], axis=1)      # (P, 5)
    lengths = _check_crops(sweep, boxes, n)
    assert np.array_equal(lengths, counts)                        # 0, 1, 2, n-1, n, n+1 and the identical pair
    got = crops.crops_from_boxes(dev(sweep), dev(boxes), n, frame="sensor", rule="dataset")
    c = host(got[0])
    assert not c[:3].any()                                        # 0, 1, 2 points: zeros under the dataset rule
    inside = R.points_in_boxes_batch(pts[None], boxes[None], frames_of(boxes)[None])[0]
    assert np.array_equal(c[4], pts[inside[:, 4] == 1])           # exactly n: the box's points in sweep order
    _check_crops(pts[:1], boxes, 64)                              # P == 1
    _check_crops(pts, boxes[:0], 64)                              # M == 0: empty outputs, nothing launched
    e = crops.crops_from_boxes(dev(pts[:0]), dev(boxes), 8)       # P == 0: zero clouds, zero lengths
    assert not host(e[0]).any() and not host(e[1]).any() and tuple(e[0].shape) == (len(boxes), 8, 3)
    from pcr_amd._lib import PcrError
    with pytest.raises(PcrError):                                 # out of range: refused on the host side
        crops.crops_from_boxes(dev(np.zeros((4, 17), np.float32)), dev(boxes), 8)
    with pytest.raises(PcrError):
        crops.crops_from_boxes(dev(pts), dev(boxes), 0)


def test_crops_at_the_largest_required_shapes():
    """P = 2^20 (a count table beyond the default 64 KiB of LDS), stride 8, n = 4096; and M = 4096 boxes"""
    g = np.random.default_rng(17)
    boxes = R.make_scene(0, 8, 3)[1]
    boxes[:, :2] *= 0.2                                            # +-10 m: the boxes hold a few thousand points each
    sweep = np.zeros((1 << 20, 8), np.float32)
    sweep[:, :3] = g.uniform(-1, 1, (1 << 20, 3)) * np.array([12.0, 12.0, 3.0])
    combos = {(False, "box", "tracker", False), (True, "centred", "dataset", True)}
    lengths = _check_crops(sweep, boxes, 4096, combos=combos)
    assert lengths.min() > 100
    pts, many = R.make_scene(900, 4096, 4)
    _check_crops(pts[:1000], many, 64, combos=combos)


# ---- 5. the frame table -----------------------------------------------------------------------------------------------
def test_frames_against_numpy():
    """pcr_box_frames_f32 against numpy's float64 cos / sin of the SAME float32 rot.  Bound: the device functions are the
    ROCm device library's sinf / cosf, which are specified to the OpenCL accuracy table (sin, cos: <= 4 ulp); numpy's
    float64 functions are the C library's (< 1 ulp of a double = 2^-29 ulp of a float) -- together 4 ulp of the float32
    result plus that 2^-29.  Derived from those two documents, not from what the device returns."""
    g = np.random.default_rng(5)
    boxes = np.zeros((4096 + 9, 7), np.float32)
    boxes[:4096, 6] = g.uniform(-np.pi, np.pi, 4096)
    boxes[4096:, 6] = [0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 1e-3, 3.0, 6.0, -6.0]
    got = frames_of(boxes).astype(np.float64)
    rot = R.box_rot(boxes).astype(np.float64)
    want = np.stack([np.cos(rot), np.sin(rot)], axis=1)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    print("frames: worst error %.3f ulp" % err.max())
    assert (err <= 4.0 + 2.0 ** -29).all()


# ---- 6. membership against numpy's own trigonometry ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_membership_cross_check_with_numpy_trigonometry(name, scenes):
    """An independent membership in float64 with numpy's own cos / sin may disagree with the device only for points next
    to an x / y face.  Rounding bound of the float32 rotation: local_x = sx c - sy s with sx, sy rounded differences (each
    <= 2^-24 relative), two products and a sum (3 roundings, <= 3 * 2^-24 (|sx| + |sy|)) and c, s within 4 ulp (4 * 2^-24
    relative): <= 9 * 2^-24 (|sx| + |sy|) = 5.4e-7 (|sx| + |sy|); the tolerance 1e-5 max(1, |sx| + |sy|) is ~18 times that.
    Points that close to a face of a box they would otherwise be in may be at most 0.05 % of the scene (a condition on
    the inputs)."""
    from mmdet3d import ops
    points, boxes = scenes[name]
    got = host(ops.points_in_boxes_batch(dev(points[None]), dev(boxes[None])))[0]
    p = points.astype(np.float64)
    rot = R.box_rot(boxes).astype(np.float64)
    cz = boxes[:, 2].astype(np.float64) + boxes[:, 5].astype(np.float64) / 2
    near_total, bad = 0, 0
    for t in range(boxes.shape[0]):
        w, l, h = (np.float64(v) for v in boxes[t, 3:6])
        sx, sy = p[:, 0] - np.float64(boxes[t, 0]), p[:, 1] - np.float64(boxes[t, 1])
        lx = sx * np.cos(rot[t]) - sy * np.sin(rot[t])
        ly = sx * np.sin(rot[t]) + sy * np.cos(rot[t])
        tol = 1e-5 * np.maximum(1.0, np.abs(sx) + np.abs(sy))
        zin = np.abs(p[:, 2] - cz[t]) <= h / 2 + 1e-5
        inside = (np.abs(p[:, 2] - cz[t]) <= h / 2) & (np.abs(lx) < l / 2) & (np.abs(ly) < w / 2)
        dx, dy = np.abs(lx) - l / 2, np.abs(ly) - w / 2
        near = zin & (dx <= tol) & (dy <= tol) & ((np.abs(dx) <= tol) | (np.abs(dy) <= tol))
        near_total += int(near.sum())
        differ = inside != (got[:, t] == 1)
        bad += int((differ & ~near).sum())
    print("%s: %d near-face points of %d" % (name, near_total, points.shape[0]))
    assert bad == 0
    assert near_total <= 0.0005 * points.shape[0]


# ---- 7. the in-kernel generator ---------------------------------------------------------------------------------------------
def test_sampler_statistics_and_seed_on_the_device():
    from pcr_amd import crops
    g = np.random.default_rng(11)
    box = np.array([[3.0, -2.0, -1.0, 2.0, 4.5, 1.6, 0.7]], np.float32)
    inside = R.points_inside(box[0], 64, g)
    pts = np.concatenate([inside, g.uniform(20, 30, (500, 3)).astype(np.float32)])
    pts = pts[g.permutation(len(pts))]
    n, seeds = 4096, list(range(100, 116))
    dp, db = dev(pts), dev(box)
    total = np.zeros(len(pts), np.int64)
    first = None
    for sd in seeds:
        c, ln = crops.crops_from_boxes(dp, db, n, frame="sensor", seed=sd)
        assert int(ln[0]) == 64
        c = host(c)[0]
        hit = (c[:, None, :] == pts[None, :, :]).all(axis=2)             # sensor frame: the sweep's own bits
        assert (hit.sum(axis=1) == 1).all()
        cnt = hit.sum(axis=0)
        # one seed: 4096 draws of 64 points, mean 64, sigma = sqrt(4096 * (1/64) * (63/64)) = 7.94
        assert np.abs(cnt[cnt > 0] - 64).max() <= 6 * np.sqrt(n / 64 * 63 / 64) and (cnt > 0).sum() == 64
        total += cnt
        if first is None:
            first = c
        elif sd == seeds[1]:
            assert not np.array_equal(first, c)                            # another seed, another crop
    # all 16 seeds: 65536 draws, mean 1024, sigma = sqrt(65536 * (1/64) * (63/64)) = 31.75 -> the 6-sigma band
    sigma = np.sqrt(len(seeds) * n / 64 * 63 / 64)
    print("hit counts %d..%d (mean 1024, sigma %.1f)" % (total[total > 0].min(), total.max(), sigma))
    assert np.abs(total[total > 0] - len(seeds) * n / 64).max() <= 6 * sigma

    # a captured launch reads the seed word at run time
    seed_t = torch.tensor([100], dtype=torch.int64, device="cuda")
    out = (torch.empty((1, n, 3), device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"))
    crops.crops_from_boxes(dp, db, n, frame="sensor", seed=seed_t, out=out)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        crops.crops_from_boxes(dp, db, n, frame="sensor", seed=seed_t, out=out)
    gr.replay()
    a = out[0].clone()
    assert np.array_equal(host(a)[0], first)                                # seed 100 again: the eager crop
    seed_t.add_(1)
    gr.replay()
    b = out[0].clone()
    assert not torch.equal(a, b)
    seed_t.sub_(1)
    gr.replay()
    assert torch.equal(out[0], a)


# ---- 8 / 9. capture and the model ------------------------------------------------------------------------------------------
def object_scene(M, n_obj, seed):
    """M objects (pcr_amd.testing box clouds, 4 x 2 x 1.5 m) at random poses on a 15 m grid, boxes 1 % larger than the
    object so that no point sits on a face; no background -> points (M * n_obj, 3), boxes (M, 7), objects (M, n_obj, 3)"""
    from pcr_amd import testing as T
    g = np.random.default_rng([0xC20B, seed])
    objs = T.synthetic_clouds(M, n_obj, seed=seed, kind="box").numpy()
    boxes, parts = [], []
    for m in range(M):
        centre = np.array([15.0 * (m % 6) - 40.0, 15.0 * (m // 6) - 30.0, 0.0]) + g.uniform(-2, 2, 3)
        rz = g.uniform(-np.pi, np.pi)
        boxes.append([centre[0], centre[1], centre[2] - 0.5 * 1.5 * 1.01, 2.0 * 1.01, 4.0 * 1.01, 1.5 * 1.01, rz])
        parts.append(R.to_sensor(objs[m].astype(np.float64), centre, rz))
    pts = np.concatenate(parts)
    pts = pts[g.permutation(len(pts))]
    return pts.astype(np.float32), np.array(boxes, np.float32), objs


def _models():
    import bench
    return {"pt128": (lambda: bench.build_pt_model([128, 64, 32])[0], 128, None),
            "ssg1024": (lambda: bench.build_model("ssg", None)[0], 1024, 1024),
            "pointnet256": (lambda: bench.build_model("pointnet", None)[0], 256, 256)}


@pytest.mark.parametrize("kind", ["pt128", "ssg1024", "pointnet256"])
def test_forward_inference_boxes_end_to_end(kind):
    from pcr_amd import crops
    build, n, n_arg = _models()[kind]
    model = build()
    M = 24
    pts, boxes, objs = object_scene(M, n + 37, seed=21)
    dp, db = dev(pts), dev(boxes)
    frames = frames_of(boxes)
    want_c, want_l = R.crop_boxes(pts, boxes, n, frame="box", seed=5, frames=frames)
    cm = kind == "pointnet256"
    ref_in = dev(want_c.transpose(0, 2, 1) if cm else want_c)
    with torch.no_grad():
        model.calibrate_precision(dev(want_c[:M // 2]), dev(want_c[M // 2:]))      # both calls below run at one level
        xyz0, h0 = model.forward_inference(ref_in)
        xyz1, h1, ln = model.forward_inference_boxes(dp, db, n=n_arg, seed=5)
    assert np.array_equal(host(ln), want_l) and (want_l == n + 37).all()      # every box holds its object, whole
    assert torch.equal(xyz0.view(torch.int32), xyz1.view(torch.int32)) and torch.equal(h0.view(torch.int32), h1.view(torch.int32))
    # frame "box" hands back the object's own points.  Bound: each stored sensor coordinate and each box-centre coordinate is
    # rounded to float32 (<= e_in = 2^-24 * max |coordinate| each; the object -> sensor rotation itself is float64), so sx, sy
    # carry <= 2 e_in each and their rotation <= 2 sqrt(2) e_in; the device's rotation adds <= 9 * 2^-24 * (|sx| + |sy|)
    # (see the cross-check above), |sx| + |sy| <= 4 at box scale; z carries 2 e_in.
    e_in = 2.0 ** -24 * float(np.abs(pts).max())
    bound = 2 * np.sqrt(2) * e_in + 9 * 2.0 ** -24 * 4
    got_c = host(crops.crops_from_boxes(dp, db, n, frame="box", seed=5)[0])
    assert np.array_equal(got_c.view(np.uint32), want_c.view(np.uint32))
    for m in range(M):
        d = np.abs(got_c[m][:, None, :].astype(np.float64) - objs[m][None, :, :].astype(np.float64)).max(axis=2).min(axis=1)
        assert d.max() <= bound, (m, d.max(), bound)
    if kind == "pt128":
        ii, jj = torch.meshgrid(torch.arange(M), torch.arange(M), indexing="ij")
        pairs = torch.stack([ii.reshape(-1), jj.reshape(-1)], dim=1).cuda()
        with torch.no_grad():
            s0, s1 = model.match_gallery(h0, xyz0, pairs), model.match_gallery(h1, xyz1, pairs)
        assert s0.numel() == M * M and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


def test_capture_replays_on_new_contents():
    """crops_from_boxes(out=...) and forward_inference_boxes recorded in a HIP graph: after the sweep and the boxes were
    overwritten in place the replay equals the eager result on the new contents, bit for bit.  A capture refuses any
    device-to-host copy, so recording the crop also shows that it performs none."""
    import bench
    from pcr_amd import crops
    model = bench.build_pt_model([128, 64, 32])[0]
    n, M = 128, 24
    pts_a, boxes_a, _ = object_scene(M, 300, seed=31)
    pts_b, boxes_b, _ = object_scene(M, 300, seed=32)
    boxes_b[3, :2] += 400.0                                         # an empty box in the second scene
    dp, db = dev(pts_a), dev(boxes_a)
    seed_t = torch.tensor([9], dtype=torch.int64, device="cuda")
    out = (torch.empty((M, n, 3), device="cuda"), torch.empty((M,), dtype=torch.int32, device="cuda"),
           torch.empty((M, 2), device="cuda"))
    with torch.no_grad():
        first = crops.crops_from_boxes(dp, db, n, seed=seed_t)[0]
        model.calibrate_precision(first[:M // 2], first[M // 2:])   # nothing is measured inside a capture
        for _ in range(2):
            crops.crops_from_boxes(dp, db, n, seed=seed_t, out=out, return_frames=True)
            model.forward_inference_boxes(dp, db, seed=seed_t)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            crops.crops_from_boxes(dp, db, n, seed=seed_t, out=out, return_frames=True)
            xyz_g, h_g, len_g = model.forward_inference_boxes(dp, db, seed=seed_t)
        dp.copy_(dev(pts_b))
        db.copy_(dev(boxes_b))
        g.replay()
        torch.cuda.synchronize()
        c_e, l_e, f_e = crops.crops_from_boxes(dp, db, n, seed=seed_t, return_frames=True)
        xyz_e, h_e, len_e = model.forward_inference_boxes(dp, db, seed=seed_t)
    assert torch.equal(out[0].view(torch.int32), c_e.view(torch.int32)) and torch.equal(out[1], l_e)
    assert torch.equal(out[2].view(torch.int32), f_e.view(torch.int32))
    assert torch.equal(xyz_g.view(torch.int32), xyz_e.view(torch.int32)) and torch.equal(h_g.view(torch.int32), h_e.view(torch.int32))
    assert torch.equal(len_g, len_e) and int(len_e[3]) == 0 and int(len_e[4]) == 300
    want_c, want_l = R.crop_boxes(pts_b, boxes_b, n, seed=9, frames=host(f_e))
    assert np.array_equal(host(out[0]).view(np.uint32), want_c.view(np.uint32)) and np.array_equal(host(out[1]), want_l)
