#!/usr/bin/env python3
"""Writes tests/golden/ident_lsa.npz: the totals scipy.optimize.linear_sum_assignment(maximize=True) finds for the integer
co-occurrence matrices of tests/ident_ref.py::golden_cases (random counts, heavy ties, empty rows and columns, a tracker that
mostly keeps its identities; shapes up to 256 x 512).  The tests rebuild the matrices, check them against the copy kept
here, and never import scipy.

Per case i the file holds cooc_i (int32) and total_i (int64, the maximum total); `names` lists the cases.

    python tools/make_ident_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    from scipy.optimize import linear_sum_assignment
    import ident_ref as R
    out, names = {}, []
    for i, (name, cooc) in enumerate(R.golden_cases()):
        rows, cols = linear_sum_assignment(cooc.astype(np.int64), maximize=True)
        out["cooc_%d" % i] = cooc
        out["total_%d" % i] = np.int64(cooc.astype(np.int64)[rows, cols].sum())
        names.append(name)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "ident_lsa.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
