"""numpy restatement of the identity metrics (include/pcr.h section A9), written from the header's rules: the per-frame
record over a scene's state, the compaction of the co-occurrence counts, the assignment (assoc_ref.lsa, which equals
pcr_lsa_f32 bit for bit) and the score that adds a scene to the pooled table.  The GPU tests compare the kernels with it
bit for bit, the binary64 sums included; the CPU tests hold it against scipy's totals, a brute force and hand-worked
scenes.  `random_stream` scripts frames with entries the rules must ignore."""
import numpy as np

import assoc_ref as AR

F = np.float32
PRESENT, TRACKED, FRAGS, FIRST_GAP, LONGEST_GAP, CUR_GAP, EVER, LAST, TRACK_COLS = 0, 1, 2, 3, 4, 5, 6, 7, 8
T_FRAMES, T_GT_TOTAL, T_PRED_TOTAL, T_TP, T_DROPPED_GT, T_DROPPED_ID, TOTALS = 0, 1, 2, 3, 4, 5, 8
N_ROWS, N_COLS, MAX_COUNT, COUNTS = 0, 1, 2, 4
TABLE = ("idtp", "frames", "gt_total", "pred_total", "tp", "tracks", "mt", "pt", "ml", "frag", "tid_sum", "lgd_sum",
         "overflow", "inexact", "dropped_gt", "dropped_id")
IX = {k: i for i, k in enumerate(TABLE)}
SCENE = ("cooc", "gt_track", "totals", "dist_sum")


def new_scene(gt_rows, id_cap):
    return dict(cooc=np.zeros((gt_rows, id_cap), np.int32), gt_track=np.zeros((gt_rows, TRACK_COLS), np.int32),
                totals=np.zeros(TOTALS, np.int32), dist_sum=np.zeros(1, np.float64))


def new_pool():
    return dict(table=np.zeros(len(TABLE), np.int64), dist_total=np.zeros(1, np.float64))


def record(scene, det_labels, det_gt, det_id, gt_labels, gt_ids, cost, gt_cap):
    """one frame -> the new scene state; `scene` itself is left alone"""
    s = {k: v.copy() for k, v in scene.items()}
    gt_rows, id_cap = s["cooc"].shape
    D, G = len(det_labels), len(gt_labels)
    ok = [bool(gt_labels[j] >= 0 and 0 <= gt_ids[j] < gt_cap) for j in range(G)]
    tp = [bool(det_labels[d] >= 0 and 0 <= det_gt[d] < G and ok[det_gt[d]]) for d in range(D)]
    lowest = {}                                              # id -> its lowest true positive
    for d in range(D):
        if tp[d]:
            s["dist_sum"][0] = s["dist_sum"][0] + np.float64(cost[d, det_gt[d]])
            lowest.setdefault(int(gt_ids[det_gt[d]]), d)
    for g in sorted({int(gt_ids[j]) for j in range(G) if ok[j]}):
        if g >= gt_rows:
            s["totals"][T_DROPPED_GT] += 1
            continue
        row = s["gt_track"][g]
        i = int(det_id[lowest[g]]) if g in lowest else -1
        row[PRESENT] += 1
        if i >= 0:
            row[TRACKED] += 1
            if row[EVER] and row[LAST] == 0:
                row[FRAGS] += 1
            if not row[EVER]:
                row[FIRST_GAP] = row[CUR_GAP]
            row[EVER], row[CUR_GAP], row[LAST] = 1, 0, 1
            if i < id_cap:
                s["cooc"][g, i] += 1
            else:
                s["totals"][T_DROPPED_ID] += 1
        else:
            row[CUR_GAP] += 1
            row[LONGEST_GAP] = max(row[LONGEST_GAP], row[CUR_GAP])
            row[LAST] = 0
    s["totals"][T_FRAMES] += 1
    s["totals"][T_GT_TOTAL] += sum(ok)
    s["totals"][T_PRED_TOTAL] += sum(bool(det_labels[d] >= 0 and det_id[d] >= 0) for d in range(D))
    s["totals"][T_TP] += sum(tp)
    return s


def compact(cooc, max_rows, max_cols):
    """-> dict(counts (4,), row_list (max_rows,), col_list (max_cols,), cost (max_rows, max_cols))"""
    rows, cols = np.flatnonzero((cooc != 0).any(axis=1)), np.flatnonzero((cooc != 0).any(axis=0))
    counts = np.array([len(rows), len(cols), cooc.max() if cooc.size else 0, 0], np.int32)
    row_list, col_list = np.full(max_rows, -1, np.int32), np.full(max_cols, -1, np.int32)
    row_list[:min(len(rows), max_rows)] = rows[:max_rows]
    col_list[:min(len(cols), max_cols)] = cols[:max_cols]
    cost = np.zeros((max_rows, max_cols), F)
    if len(rows) <= max_rows and len(cols) <= max_cols:
        sub = cooc[np.ix_(rows, cols)]
        cost[:len(rows), :len(cols)] = np.where(sub != 0, -sub.astype(F), F(0))
    return dict(counts=counts, row_list=row_list, col_list=col_list, cost=cost)


def score(scene, pool, comp, col4row, info, max_rows, max_cols):
    """-> (the new pool, id_map (gt_rows,), the scene's idtp)"""
    cooc, gt_rows = scene["cooc"], scene["cooc"].shape[0]
    nr, nc, top = (int(v) for v in comp["counts"][:3])
    overflow, failed = nr > max_rows or nc > max_cols, int(info) != 0
    inexact = failed or (min(max_rows, max_cols) + 1) * top >= 1 << 24
    id_map, idtp = np.full(gt_rows, -1, np.int32), 0
    if not overflow and not failed:
        for r in range(nr):
            c = int(col4row[r])
            if 0 <= c < nc:
                g, i = int(comp["row_list"][r]), int(comp["col_list"][c])
                if cooc[g, i] > 0:
                    idtp += int(cooc[g, i])
                    id_map[g] = i
    pool = {k: v.copy() for k, v in pool.items()}
    t = pool["table"]
    t[IX["idtp"]] += idtp
    for k, src in (("frames", T_FRAMES), ("gt_total", T_GT_TOTAL), ("pred_total", T_PRED_TOTAL), ("tp", T_TP),
                   ("dropped_gt", T_DROPPED_GT), ("dropped_id", T_DROPPED_ID)):
        t[IX[k]] += int(scene["totals"][src])
    for row in scene["gt_track"].astype(np.int64):
        if row[PRESENT] <= 0:
            continue
        t[IX["tracks"]] += 1
        kind = "mt" if 5 * row[TRACKED] >= 4 * row[PRESENT] else "ml" if 5 * row[TRACKED] < row[PRESENT] else "pt"
        t[IX[kind]] += 1
        t[IX["frag"]] += row[FRAGS]
        t[IX["tid_sum"]] += row[FIRST_GAP] if row[EVER] else row[PRESENT]
        t[IX["lgd_sum"]] += row[LONGEST_GAP]
    t[IX["overflow"]] += int(overflow)
    t[IX["inexact"]] += int(inexact)
    pool["dist_total"][0] = pool["dist_total"][0] + scene["dist_sum"][0]
    return pool, id_map, idtp


def close_scene(scene, pool, max_rows, max_cols):
    """compaction, assignment, score -> (the new pool, id_map, idtp, compact's dict)"""
    comp = compact(scene["cooc"], max_rows, max_cols)
    col4row, _, _, _, info = AR.lsa(comp["cost"])
    pool, id_map, idtp = score(scene, pool, comp, col4row, info, max_rows, max_cols)
    return pool, id_map, idtp, comp


def idtp_of(cooc, max_rows=None, max_cols=None):
    """the restatement's IDTP of one co-occurrence matrix alone"""
    cooc = np.asarray(cooc, np.int32)
    scene = new_scene(*cooc.shape)
    scene["cooc"] = cooc
    return close_scene(scene, new_pool(), max_rows or max(cooc.shape[0], 1), max_cols or max(cooc.shape[1], 1))[2]


def metrics(table, dist_total, fp=0):
    """the pooled table -> the identity metrics (pcr_amd.identity.metrics_of restated)"""
    t = {k: int(table[i]) for k, i in IX.items()}
    div = lambda a, b: a / b if b else float("nan")
    out = dict(idtp=t["idtp"], idfn=t["gt_total"] - t["idtp"], idfp=t["pred_total"] - t["idtp"],
               idp=div(t["idtp"], t["pred_total"]), idr=div(t["idtp"], t["gt_total"]),
               idf1=div(2 * t["idtp"], t["gt_total"] + t["pred_total"]), tid=div(t["tid_sum"], t["tracks"]),
               lgd=div(t["lgd_sum"], t["tracks"]), motp=div(float(dist_total), t["tp"]), faf=div(int(fp), t["frames"]))
    for k in ("mt", "pt", "ml", "tracks", "frag", "frames", "gt_total", "pred_total", "tp", "overflow", "inexact", "dropped_gt",
              "dropped_id"):
        out[k] = t[k]
    return out


# ---- scripted streams ----------------------------------------------------------------------------------------------------
def random_frame(g, D, G, gt_cap, gt_rows, id_cap):
    """one frame with what the rules must ignore: padding on both sides, two boxes of one id, ids at and beyond gt_cap /
    gt_rows / id_cap, negative and large, det_gt outside [0, G), untracked true positives"""
    det_labels = np.where(g.random(D) < 0.85, g.integers(0, 3, D), -1).astype(np.int32)
    gt_labels = np.where(g.random(G) < 0.85, g.integers(0, 3, G), -1).astype(np.int32)
    n_ids = max(2, min(gt_cap, (3 * G) // 4))                # few ids: some are carried by two boxes
    gt_ids = g.integers(0, n_ids, G).astype(np.int32)
    wild = g.random(G)
    gt_ids = np.where(wild < 0.06, gt_cap + g.integers(0, 3, G), gt_ids)
    gt_ids = np.where((wild >= 0.06) & (wild < 0.1), -1 - g.integers(0, 3, G), gt_ids)
    gt_ids = np.where((wild >= 0.1) & (wild < 0.13), 2 ** 31 - 1 - g.integers(0, 3, G), gt_ids)
    gt_ids = np.where((wild >= 0.13) & (wild < 0.2), g.integers(0, gt_cap, G), gt_ids).astype(np.int32)      # ... beyond gt_rows
    det_gt = np.full(D, -1, np.int32)
    cols = g.permutation(G)
    for d in range(min(D, G)):
        if g.random() < 0.75:
            det_gt[d] = cols[d]                              # one-to-one
    wild = g.random(D)
    det_gt = np.where(wild < 0.04, G + g.integers(0, 3, D), det_gt)
    det_gt = np.where((wild >= 0.04) & (wild < 0.08), -2 - g.integers(0, 3, D), det_gt).astype(np.int32)
    det_id = g.integers(0, max(min(id_cap, 2 * D), 1), D).astype(np.int32)
    wild = g.random(D)
    det_id = np.where(wild < 0.15, -1, det_id)               # untracked
    det_id = np.where((wild >= 0.15) & (wild < 0.2), id_cap + g.integers(0, 3, D), det_id)
    det_id = np.where((wild >= 0.2) & (wild < 0.23), 2 ** 31 - 1, det_id)
    det_id = np.where((wild >= 0.23) & (wild < 0.26), -2 ** 31, det_id).astype(np.int32)
    cost = (g.uniform(0.0, 3.0, (D, G)) * np.where(g.random((D, G)) < 0.5, 1.0, 1e-3)).astype(F)
    return dict(det_labels=det_labels, det_gt=det_gt, det_id=det_id, gt_labels=gt_labels, gt_ids=gt_ids, cost=cost)


def random_stream(seed, frames, D, G, gt_cap, gt_rows, id_cap):
    """[(frame, the scene state after it)]"""
    g = np.random.default_rng(seed)
    scene, out = new_scene(gt_rows, id_cap), []
    for _ in range(frames):
        fr = random_frame(g, D, G, gt_cap, gt_rows, id_cap)
        scene = record(scene, gt_cap=gt_cap, **fr)
        out.append((fr, scene))
    return out


# ---- generated cases of the fixture tool (tools/make_ident_golden.py) and the tests ----------------------------------------
GOLDEN_SHAPES = ((1, 1), (2, 3), (3, 2), (4, 4), (7, 5), (16, 16), (33, 65), (65, 33), (64, 64), (100, 130), (256, 512))
GOLDEN_KINDS = ("random", "ties", "sparse", "diagonal")


def golden_case(R, C, kind, seed=0):
    """a co-occurrence matrix (R, C) int32 of counts >= 0: `random` up to 200, `ties` of 0 / 1 / 2 only, `sparse` with most
    rows and columns empty, `diagonal` a tracker that mostly keeps its identities with a few swaps"""
    g = np.random.default_rng([R, C, GOLDEN_KINDS.index(kind), seed])
    if kind == "random":
        m = g.integers(0, 201, (R, C))
    elif kind == "ties":
        m = g.integers(0, 3, (R, C))
    elif kind == "sparse":
        m = g.integers(1, 40, (R, C)) * (g.random((R, 1)) < 0.4) * (g.random((1, C)) < 0.4) * (g.random((R, C)) < 0.3)
    else:
        m = np.zeros((R, C), np.int64)
        for r in range(R):
            m[r, (r * 3) % C] += g.integers(5, 40)
            if g.random() < 0.3:
                m[r, g.integers(0, C)] += g.integers(1, 40)
    return m.astype(np.int32)


def golden_cases():
    """[(name, matrix)] in the order of the fixture file"""
    return [("%s_%d_%d" % (kind, R, C), golden_case(R, C, kind)) for R, C in GOLDEN_SHAPES for kind in GOLDEN_KINDS]
