#!/usr/bin/env python3
"""Writes tests/golden/assoc_lsa.npz: cost matrices together with what scipy.optimize.linear_sum_assignment -- the solver the
reference's tracker calls (trackers/deprecated/tracking_association.py:141) -- returns for them in float64.  The tests read
the file and never import scipy.

  float cases    built the reference way (tests/assoc_ref.py::reference_case: 4 classes, logits ~ N(0, 4^2), fill 10000,
                 N(0, 1) miss / new diagonals) for (T, D) in FLOAT_SHAPES, FLOAT_SEEDS seeds each;
  integer cases  uniform integers in [0, 64) and [0, 4) (many ties) for (R, C) in INT_SHAPES.

Per case i the file holds cost_i (float32), rows_i / cols_i (scipy's row_ind / col_ind) and the vectors kind (0 float,
1 integer) and total (scipy's float64 total).

    python tools/make_assoc_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

FLOAT_SHAPES = ((1, 1), (3, 5), (5, 3), (17, 33), (64, 64), (100, 37), (128, 128))
FLOAT_SEEDS = 4
INT_SHAPES = ((7, 7), (16, 40), (64, 64), (65, 130), (130, 65))
INT_HIGHS = (64, 4)


def main():
    from scipy.optimize import linear_sum_assignment
    import assoc_ref as R
    out, kind, total = {}, [], []

    def add(cost, k):
        i = len(kind)
        rows, cols = linear_sum_assignment(cost.astype(np.float64))
        out["cost_%d" % i] = cost
        out["rows_%d" % i], out["cols_%d" % i] = rows.astype(np.int32), cols.astype(np.int32)
        kind.append(k)
        total.append(cost.astype(np.float64)[rows, cols].sum())

    for si, (T, D) in enumerate(FLOAT_SHAPES):
        for s in range(FLOAT_SEEDS):
            add(R.reference_case(T, D, seed=100 * si + s)[0], 0)
    for si, (r, c) in enumerate(INT_SHAPES):
        for hi in INT_HIGHS:
            add(R.integer_case(r, c, hi, seed=1000 + 10 * si + hi), 1)
    out["kind"], out["total"] = np.array(kind, np.int32), np.array(total, np.float64)
    path = os.path.join(ROOT, "tests", "golden", "assoc_lsa.npz")
    np.savez_compressed(path, **out)
    print("%s: %d float + %d integer cases, %d bytes" % (path, kind.count(0), kind.count(1), os.path.getsize(path)))


if __name__ == "__main__":
    main()
