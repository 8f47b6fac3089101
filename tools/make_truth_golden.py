#!/usr/bin/env python3
"""Writes tests/golden/truth_lsa.npz: what scipy.optimize.linear_sum_assignment -- the solver the reference's get_iou_idx
calls on a host copy (trackers/deprecated/virtual_tracker.py:206, :218) -- returns in float64 for the cost matrices of
tests/truth_ref.py::lsa_cases (centre distance or -IoU plus the 10000 class mask, padding included).  The tests rebuild the
matrices, check them against the copy kept here, and never import scipy.

Per case i the file holds cost_i (float32), rows_i / cols_i (scipy's row_ind / col_ind); `names` lists the cases.

    python tools/make_truth_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    from scipy.optimize import linear_sum_assignment
    import truth_ref as R
    out, names = {}, []
    for i, (name, case) in enumerate(R.lsa_cases()):
        rows, cols = linear_sum_assignment(case["cost"].astype(np.float64))
        out["cost_%d" % i] = case["cost"]
        out["rows_%d" % i], out["cols_%d" % i] = rows.astype(np.int32), cols.astype(np.int32)
        names.append(name)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "truth_lsa.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
