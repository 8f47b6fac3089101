"""CPU: the library's exported shape queries (what engine.py asks before it builds row tables, tables with the
coordinate term, tile / claim workspaces, kv splits and pooled outputs) answer as recorded in
tests/golden/shape_queries.json over a grid of shapes.  The queries restate no dispatcher rule of their own: a change of
one of these answers is a change of the dispatch, and has to be recorded on purpose.

Recording (only the non-zero answers are stored):  python tests/test_shape_queries.py --record [path/to/libpcr_hip.so]"""
import ctypes
import itertools
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_queries.json")

CH = (3, 16, 32, 48, 64, 96, 128, 192, 256, 512)
KS = (1, 2, 8, 16, 24, 32, 48, 64, 96, 128)
PRECS = (0, 1, 2)
NS = (128, 1024, 2048, 4096)


def _key(*args):
    return ",".join(str(a) for a in args)


def _sa_queries(lib):
    lib.pcr_sa_tile_ws_ints.restype = ctypes.c_long
    lib.pcr_sa_claim_ws_ints.restype = ctypes.c_long
    out = {"sa_uses_row_table": {}, "sa_krow_uses_tiles": {}, "sa_tables_take_xyz": {}, "sa_claim_ws_ints": {},
           "sa_tile_ws_ints": {}}
    for c1, c2, c3, K, prec in itertools.product(CH, CH, CH, KS, PRECS):
        for name, v in (("sa_uses_row_table", lib.pcr_sa_uses_row_table(c1, c2, c3, K, prec)),
                        ("sa_krow_uses_tiles", lib.pcr_sa_krow_uses_tiles(c1, c2, c3, K, prec))):
            if v:
                out[name][_key(c1, c2, c3, K, prec)] = v
        for mode, D in itertools.product((0, 1), (0, 3, 64)):
            v = lib.pcr_sa_tables_take_xyz(mode, D, c1, c2, c3, K, prec)
            if v:
                out["sa_tables_take_xyz"][_key(mode, D, c1, c2, c3, K, prec)] = v
        for N in NS:
            v = lib.pcr_sa_claim_ws_ints(c1, c2, c3, K, N, prec)
            if v:
                out["sa_claim_ws_ints"][_key(c1, c2, c3, K, N, prec)] = v
    for B, S, K, c2, c3 in itertools.product((0, 1, 64), (0, 1, 128, 1000), KS, CH, CH):
        v = lib.pcr_sa_tile_ws_ints(B, S, K, c2, c3)
        if v:
            out["sa_tile_ws_ints"][_key(B, S, K, c2, c3)] = v
    return out


def _attn_queries(lib):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-reid_amd"))
    from pcr_amd import engine
    out = {"attn_kv_splits": {}, "attn_apply_pool_ok": {}}
    for B, Sk, d in itertools.product((1, 8, 256), (1, 31, 32, 64, 100, 128, 500, 512, 1000, 1024, 2000, 2048), (32, 64, 96, 128, 256)):
        v = lib.pcr_attn_kv_splits(B, Sk, d)
        if v:
            out["attn_kv_splits"][_key(B, Sk, d)] = v
    # the host code only tests the pointers for null: one dummy address stands for every tensor
    dummy, null = 64, None
    required = ("feat_q", "feat_k", "xyz_k", "kv", "pos0_w", "pos0_b", "wq", "bq", "wkv", "bkv", "wmerge", "wmlp0",
                "wmlp2", "ln1_g", "ln1_b", "ln2_g", "ln2_b", "xyz_q", "wfinal", "bfinal", "out", "pool_out")
    for (d, c1, cout, cfinal, q_pos, residual, nhead, Lq, prec, bf, xpad) in itertools.product(
            (32, 64, 96, 128, 256), (3, 16, 32, 64, 128), (32, 64, 128), (0, 64, 128), (0, 1), (0, 1), (1, 2, 4, 8),
            (32, 100, 128), (0, 1), (0, 1), (0, 1)):
        p = engine.AttnParams()
        p.B, p.Lq, p.Sk, p.c1, p.c2, p.d, p.cout, p.nhead = 4, Lq, 128, c1, 64, d, cout, nhead
        p.q_pos, p.residual, p.cfinal, p.precision = q_pos, residual, cfinal, prec
        for f in required:
            setattr(p, f, dummy)
        for f in ("wq_bf", "wmlp0_bf", "wmlp2_bf", "wfinal_bf", "wkv_bf"):
            setattr(p, f, dummy if bf else null)
        p.wmlp0_bf_xpad = dummy if xpad else null
        v = lib.pcr_attn_apply_pool_ok(ctypes.byref(p))
        if v:
            out["attn_apply_pool_ok"][_key(d, c1, cout, cfinal, q_pos, residual, nhead, Lq, prec, bf, xpad)] = v
    return out


def answers(lib):
    out = _sa_queries(lib)
    out.update(_attn_queries(lib))
    return out


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def got(lib):
    return answers(lib)


@pytest.mark.parametrize("query", ["sa_uses_row_table", "sa_krow_uses_tiles", "sa_tables_take_xyz", "sa_claim_ws_ints",
                                   "sa_tile_ws_ints", "attn_kv_splits", "attn_apply_pool_ok"])
def test_shape_query_matches_golden(got, query):
    want = json.load(open(GOLDEN))[query]
    assert want, "the golden file holds no non-zero answer of %s" % query
    have = got[query]
    missing = sorted(set(want) - set(have))[:10]
    extra = sorted(set(have) - set(want))[:10]
    changed = sorted(k for k in set(want) & set(have) if want[k] != have[k])[:10]
    assert not (missing or extra or changed), \
        "%s: answers no longer given %s, new answers %s, changed %s" % (query, missing, extra, changed)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit(__doc__)
    import torch  # noqa: F401  (must precede the HIP library)
    if len(sys.argv) > 2:
        L = ctypes.CDLL(os.path.abspath(sys.argv[2]))
    else:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "point-cloud-reid_amd"))
        from pcr_amd import _lib
        L = _lib.load()
    rec = answers(L)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(GOLDEN, {k: len(v) for k, v in rec.items()})
