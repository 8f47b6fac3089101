#!/usr/bin/env python3
"""Writes tests/golden/assoc_decisions.npz: what the reference's own associators compute for any set of decisions -- the
matrices of TrackingAssociator.get_cost_mat (margin and softmax, trackers/deprecated/tracking_association.py:22-98), the
decision lists its __call__ returns (:106-271), and the margin matrix and decision indices of TrackingAssociatorMax
(:319-363).  The tests read the file and import neither scipy nor the reference.

The reference file is loaded by path behind a stub of mmdet3d.models.builder.TRACKERS (it needs nothing else of mmdet3d);
create_summary is overridden on the instance (it only makes log scalars).

Cases: (dd, td) in DECISIONS, both kinds, T and D drawn from 1..8, plus one (70, 40) per (dd, td) and kind.  Margin cases
hold 10000 (the class gate's fill) at 30 % of the entries, softmax cases are dense.  A case is DROPPED when scipy's optimum
lands on a 10000 entry (the reference prints and exits there) or when the reference's own consistency check fails (its
simultaneous repair handed one object out twice, :171-197, and it exits too); at least 95 % of the drawn cases must survive.
With dd = 0 the shapes are drawn with D <= T: a detection left over when every track is taken has no row of its own, the
reference's repair then hands it track 0 a second time (:186-197, the minimum over a column that is 10000 throughout) and
exits on every such case, so there is nothing of the reference's to record for D > T.

Per surviving case i: sup_i (T, D) (supervise['cost_mat']: a cost for margin, a score for softmax), det_i (dd, D), trk_i
(td, T), cost_i (the reference's matrix) and, from the decision lists, det_decision_i (D,) / track_decision_i (T,) (0 =
matched, 1 + k = decision k, 1 + dd / 1 + td = unmatched) and track_to_det_i (T,) (-1 = none); for a reduce case cost_i,
det_choice_i, trk_choice_i only.  The vectors T, D, dd, td, kind (0 margin, 1 softmax), reduce describe the cases.

    PCR_REFERENCE_ROOT=/path/to/reference python tools/make_decisions_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get("PCR_REFERENCE_ROOT", "/root/reference")

DECISIONS = ((2, 0), (2, 1), (1, 2), (2, 2), (1, 1), (0, 1), (3, 1))
SMALL_PER_CONFIG = 16
BIG = (70, 40)
FILL = 10000.0


def load_reference():
    class _Registry:
        def register_module(self):
            return lambda cls: cls
    for name in ("mmdet3d", "mmdet3d.models", "mmdet3d.models.builder"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mmdet3d.models.builder"].TRACKERS = _Registry()
    path = os.path.join(REF_ROOT, "mmdet3d", "models", "trackers", "deprecated", "tracking_association.py")
    spec = importlib.util.spec_from_file_location("_pcr_ref_tracking_association", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def draw(g, T, D, dd, td, kind):
    sup = (g.standard_normal((T, D)) * 4.0).astype(np.float32)
    if kind == 0:
        sup[g.random((T, D)) < 0.3] = FILL
    return sup, g.standard_normal((dd, D)).astype(np.float32), g.standard_normal((td, T)).astype(np.float32)


def main():
    import torch
    from scipy.optimize import linear_sum_assignment
    ref = load_reference()
    out, meta = {}, {k: [] for k in ("T", "D", "dd", "td", "kind", "reduce")}
    drawn = kept = 0

    def record(T, D, dd, td, kind, reduce, arrays):
        i = len(meta["T"])
        for k, v in zip(("T", "D", "dd", "td", "kind", "reduce"), (T, D, dd, td, kind, reduce)):
            meta[k].append(v)
        for k, v in arrays.items():
            out["%s_%d" % (k, i)] = v

    for ci, (dd, td) in enumerate(DECISIONS):
        det_names = ["det_d%d" % i for i in range(dd)]
        trk_names = ["track_d%d" % j for j in range(td)]
        tracker = types.SimpleNamespace(detection_decisions=det_names, tracking_decisions=trk_names, dd_num=dd, td_num=td)
        for kind in (0, 1):
            g = np.random.default_rng(1000 * ci + kind)
            shapes = [tuple(int(x) for x in g.integers(1, 9, 2)) for _ in range(SMALL_PER_CONFIG)] + [BIG]
            for T, D in shapes:
                if dd == 0 and D > T:
                    T, D = D, T          # (see the docstring: without a detection decision the reference needs D <= T)
                sup, det, trk = draw(g, T, D, dd, td, kind)
                supervise = {"cost_mat": torch.from_numpy(sup)}
                supervise.update({k: torch.from_numpy(det[i]) for i, k in enumerate(det_names)})
                supervise.update({k: torch.from_numpy(trk[j]) for j, k in enumerate(trk_names)})
                assoc = ref.TrackingAssociator(cost_mat_type="margin" if kind == 0 else "softmax")
                assoc.create_summary = lambda *a, **k: {}
                cost = torch.full((T + dd * D, D + td * T), FILL, dtype=torch.float32)
                cost = assoc.get_cost_mat(num_det=D, num_trk=T, supervise=supervise, tracker=tracker, cost_mat=cost,
                                          track_det_dists=[], device="cpu").numpy().copy()
                drawn += 1
                rows, cols = linear_sum_assignment(cost)
                if (cost[rows, cols] == np.float32(FILL)).any():
                    continue
                try:
                    dec, _, _ = assoc(supervise, tracker, T, D, "car", [], None, "cpu")
                except SystemExit:
                    continue
                kept += 1
                ddec, tdec = np.full(D, 1 + dd, np.int32), np.full(T, 1 + td, np.int32)
                t2d = np.full(T, -1, np.int32)
                ddec[dec["det_match"].numpy()] = 0
                tdec[dec["track_match"].numpy()] = 0
                t2d[dec["track_match"].numpy()] = dec["det_match"].numpy()
                for i, k in enumerate(det_names):
                    ddec[dec[k].numpy()] = 1 + i
                for j, k in enumerate(trk_names):
                    tdec[dec[k].numpy()] = 1 + j
                assert sorted(dec["det_unmatched"].tolist()) == np.flatnonzero(ddec == 1 + dd).tolist()
                assert sorted(dec["track_unmatched"].tolist()) == np.flatnonzero(tdec == 1 + td).tolist()
                record(T, D, dd, td, kind, 0, dict(sup=sup, det=det, trk=trk, cost=cost, det_decision=ddec,
                                                   track_decision=tdec, track_to_det=t2d))
                if kind == 0 and T <= 8:                 # the same inputs through TrackingAssociatorMax's margin matrix
                    amax = ref.TrackingAssociatorMax(cost_mat_type="margin")
                    cm = torch.full((T + (dd > 0) * D, D + (td > 0) * T), FILL, dtype=torch.float32)
                    (cm, _, _), trk_idx, det_idx = amax.get_cost_mat(num_det=D, num_trk=T, supervise=supervise,
                                                                      tracker=tracker, cost_mat=cm, track_det_dists=[],
                                                                      device="cpu")
                    record(T, D, dd, td, 0, 1, dict(sup=sup, det=det, trk=trk, cost=cm.numpy().copy(),
                                                    det_choice=det_idx.numpy().astype(np.int32).reshape(-1),
                                                    trk_choice=trk_idx.numpy().astype(np.int32).reshape(-1)))
    assert kept >= 0.95 * drawn, "only %d of %d drawn cases survive" % (kept, drawn)
    for k, v in meta.items():
        out[k] = np.array(v, np.int32)
    path = os.path.join(ROOT, "tests", "golden", "assoc_decisions.npz")
    np.savez_compressed(path, **out)
    print("%s: %d of %d drawn cases kept, %d records (%d reduce), %d bytes"
          % (path, kept, drawn, len(meta["T"]), int(np.sum(meta["reduce"])), os.path.getsize(path)))


if __name__ == "__main__":
    main()
