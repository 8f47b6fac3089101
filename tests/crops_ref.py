"""CPU restatement (numpy) of include/pcr.h section A2: box membership, the sampler, the in-kernel generator, the three
frames and both rules of pcr_crop_boxes_f32, plus the seeded scene generator the crop tests share.

Arithmetic is float32 with the double expressions of the reference's points_in_boxes_cuda.cu:24-49 (z centre, half
extents, comparisons); numpy never fuses a product into a sum.  `frames` ((M, 2) = cos / sin of rz + pi/2) is an INPUT:
fed with the table pcr_box_frames_f32 returned, every output below equals the device's bit for bit.  `box_frames` is
numpy's own table, for the independent cross-checks."""
import numpy as np

HALF_PI = 1.57079632679489661923
F32 = np.float32
SCENE_COUNTS = (0, 1, 2, 3, 5, 17, 40, 127, 128, 129, 300, 2000)


def box_rot(boxes):
    """rot = rz + pi/2: a double sum rounded to float"""
    return (np.asarray(boxes, F32)[:, 6].astype(np.float64) + HALF_PI).astype(F32)


def box_frames(boxes, dtype=F32):
    rot = box_rot(boxes).astype(dtype)
    return np.stack([np.cos(rot), np.sin(rot)], axis=1)


def box_cz(boxes, z_is_centre=False):
    boxes = np.asarray(boxes, F32)
    if z_is_centre:
        return boxes[:, 2].copy()
    return (boxes[:, 2].astype(np.float64) + boxes[:, 5].astype(np.float64) / 2.0).astype(F32)


def box_test(xyz, box, frame, cz):
    """one box against all points -> (inside (P,) bool, local_x, local_y (P,) float32)"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cx, cy, w, l, h = F32(box[0]), F32(box[1]), F32(box[3]), F32(box[4]), F32(box[5])
    cosa, sina = F32(frame[0]), F32(frame[1])
    sx, sy = x - cx, y - cy
    a0 = sx * cosa
    a1 = sy * (-sina)
    lx = a0 + a1
    b0 = sx * sina
    b1 = sy * cosa
    ly = b0 + b1
    z_out = np.abs(z - F32(cz)).astype(np.float64) > np.float64(h) / 2.0
    lx64, ly64 = lx.astype(np.float64), ly.astype(np.float64)
    hl, nhl = np.float64(l) / 2.0, np.float64(-l) / 2.0
    hw, nhw = np.float64(w) / 2.0, np.float64(-w) / 2.0
    inside = ~z_out & (lx64 > nhl) & (lx64 < hl) & (ly64 > nhw) & (ly64 < hw)
    return inside, lx, ly


def points_in_boxes_batch(points, boxes, frames=None):
    """(B, P, 3), (B, T, 7) -> (B, P, T) int32 of 0 / 1"""
    points, boxes = np.asarray(points, F32), np.asarray(boxes, F32)
    B, P, _ = points.shape
    T = boxes.shape[1]
    out = np.zeros((B, P, T), np.int32)
    for b in range(B):
        fr = box_frames(boxes[b]) if frames is None else frames[b]
        cz = box_cz(boxes[b])
        for t in range(T):
            out[b, :, t] = box_test(points[b], boxes[b, t], fr[t], cz[t])[0]
    return out


def points_in_boxes_gpu(points, boxes, frames=None):
    """-> (B, P) int32: the lowest index of a box that holds the point, -1 for none"""
    m = points_in_boxes_batch(points, boxes, frames)
    if m.shape[2] == 0:
        return np.full(m.shape[:2], -1, np.int32)
    first = m.argmax(axis=2).astype(np.int32)
    return np.where(m.any(axis=2), first, np.int32(-1)).astype(np.int32)


def sample_index(u, length):
    """slot word u (uint32) -> in-box rank j = (uint64(u) * len) >> 32"""
    return (np.asarray(u).astype(np.uint64) * np.uint64(length)) >> np.uint64(32)


def _mix(x):
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x, np.uint64) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def crop_words(seed, m, n):
    """the n words of box m under `seed` (pcr.h: the counter-based generator of pcr_crop_boxes_f32) as uint32"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    h = _mix(np.uint64((seed & 0xFFFFFFFF) ^ 0x9E3779B9))
    h = _mix(h ^ np.uint64(seed >> 32))
    h = _mix(h ^ np.uint64(m))
    return _mix(h ^ np.arange(n, dtype=np.uint64)).astype(np.uint32)


def crop_boxes(points, boxes, n, frame="box", rule="tracker", rand=None, seed=0, z_is_centre=False, frames=None, cache=None):
    """points (P, C >= 3), boxes (M, 7) -> clouds (M, n, 3) float32, lengths (M,) int32.  cache: a dict that keeps the
    per-box membership between calls with the SAME points, boxes, frames and z_is_centre (the tests' sweeps over frame /
    rule / words)"""
    points, boxes = np.asarray(points, F32), np.asarray(boxes, F32)
    xyz = points[:, :3]
    M = boxes.shape[0]
    fr = box_frames(boxes) if frames is None else np.asarray(frames, F32)
    cz = box_cz(boxes, z_is_centre)
    clouds = np.zeros((M, n, 3), F32)
    lengths = np.zeros((M,), np.int32)
    for m in range(M):
        if cache is not None and m in cache:
            idx, lx, ly = cache[m]
        else:
            inside, lx, ly = box_test(xyz, boxes[m], fr[m], cz[m])
            idx = np.nonzero(inside)[0]                   # ascending sweep index
            lx, ly = (lx[idx], ly[idx]) if cache is not None else (lx, ly)
            if cache is not None:
                cache[m] = (idx, lx, ly)
        ln = lengths[m] = idx.size
        if rule == "tracker":
            mode = 0 if ln == 0 else 1
        elif rule == "dataset":
            mode = 0 if ln <= 2 else (2 if ln == n else 1)
        else:
            raise ValueError(rule)
        if mode == 0:
            continue
        if mode == 2:
            j = np.arange(n)
        else:
            u = crop_words(seed, m, n) if rand is None else np.asarray(rand[m]).astype(np.int64).astype(np.uint32)
            j = sample_index(u, ln).astype(np.int64)
        pick = idx[j]
        jl = j if cache is not None else pick             # (a cache keeps local_x / local_y of the in-box points only)
        if frame == "sensor":
            c = xyz[pick]
        elif frame == "centred":
            c = np.stack([xyz[pick, 0] - boxes[m, 0], xyz[pick, 1] - boxes[m, 1], xyz[pick, 2] - cz[m]], axis=1)
        elif frame == "box":
            c = np.stack([lx[jl], ly[jl], xyz[pick, 2] - cz[m]], axis=1)
        else:
            raise ValueError(frame)
        clouds[m] = c
    return clouds, lengths


def to_sensor(local, box_centre, rz):
    """box-frame coordinates (k, 3) float64 -> sensor coordinates: the inverse of the membership transform"""
    rot = np.float64(rz) + HALF_PI
    c, s = np.cos(rot), np.sin(rot)
    out = np.empty_like(local)
    out[:, 0] = local[:, 0] * c + local[:, 1] * s + box_centre[0]
    out[:, 1] = -local[:, 0] * s + local[:, 1] * c + box_centre[1]
    out[:, 2] = local[:, 2] + box_centre[2]
    return out


def make_scene(n_background, n_boxes, seed):
    """seeded sweep + boxes: centres uniform in +-50 x +-50 x [-2, 1] m, w 1.5-2.5, l 3.5-5.5, h 1.4-2.0, rz in +-pi;
    box m gets SCENE_COUNTS[m % 12] points uniform in 1.2 x its extent (some fall outside), then background points
    uniform in +-55 x +-55 x +-3; shuffled.  -> points (P, 3) float32, boxes (M, 7) float32 (z = bottom face)"""
    g = np.random.default_rng([0xC209, seed])
    centre = np.stack([g.uniform(-50, 50, n_boxes), g.uniform(-50, 50, n_boxes), g.uniform(-2, 1, n_boxes)], axis=1)
    w, l, h = g.uniform(1.5, 2.5, n_boxes), g.uniform(3.5, 5.5, n_boxes), g.uniform(1.4, 2.0, n_boxes)
    rz = g.uniform(-np.pi, np.pi, n_boxes)
    parts = []
    for m in range(n_boxes):
        k = SCENE_COUNTS[m % len(SCENE_COUNTS)]
        local = g.uniform(-0.6, 0.6, (k, 3)) * np.array([l[m], w[m], h[m]])
        parts.append(to_sensor(local, centre[m], rz[m]))
    parts.append(g.uniform(-1, 1, (n_background, 3)) * np.array([55.0, 55.0, 3.0]))
    pts = np.concatenate(parts, axis=0)
    pts = pts[g.permutation(pts.shape[0])]
    boxes = np.stack([centre[:, 0], centre[:, 1], centre[:, 2] - h / 2, w, l, h, rz], axis=1)
    return pts.astype(F32), boxes.astype(F32)


def points_inside(box, k, g, scale=0.9):
    """k points well inside `box` (bottom-z), float32 sensor coordinates"""
    box = np.asarray(box, np.float64)
    local = g.uniform(-0.5 * scale, 0.5 * scale, (k, 3)) * np.array([box[4], box[3], box[5]])
    return to_sensor(local, (box[0], box[1], box[2] + box[5] / 2), box[6]).astype(F32)


def hand_scene(n, seed=0):
    """what make_scene does not produce: a box far from every point, boxes with exactly 1, 2, n-1, n, n+1 points, two
    identical boxes; P is not a multiple of 64.  Boxes are 500 m apart, no background.  -> points, boxes, counts"""
    g = np.random.default_rng([0xC20A, seed])
    counts = [0, 1, 2, n - 1, n, n + 1, 7, 7]
    boxes, parts = [], []
    for i, k in enumerate(counts):
        box = np.array([500.0 * i - 1000.0, 40.0 * i, -1.0 + 0.1 * i, 2.0, 4.5, 1.6, 0.3 * i - 1.0])
        if i == len(counts) - 1:
            box = boxes[-1].copy()                       # identical to its predecessor, shares its points
        else:
            parts.append(points_inside(box, k, g))
        boxes.append(box)
    pts = np.concatenate(parts, axis=0)
    if pts.shape[0] % 64 == 0:
        pts = np.concatenate([pts, np.array([[9000.0, 9000.0, 0.0]], F32)], axis=0)
    pts = pts[g.permutation(pts.shape[0])]
    return pts.astype(F32), np.stack(boxes).astype(F32), np.array(counts, np.int32)
