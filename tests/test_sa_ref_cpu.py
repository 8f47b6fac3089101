"""CPU: tests/sa_ref.py held to account before tests/test_gpu_sa_forms.py relies on it.  The float64 layer against a second
formulation (torch.nn modules cast to double on the materialised (B,cin,S,K) tensor); ragged = K-row in the reference;
planted faults -- what a kernel with a bookkeeping slip would compute -- must move the reference by more than ten times
the bf16x3 bound on every row of the GPU file they apply to; the restated shape rules against the library's exported shape
queries (the library loads without a device); and the GPU file's frozen row table against the restatement."""
import copy
import functools
import os

import pytest
import torch

import sa_ref as R
import test_gpu_sa_forms as G

FAULT_MARGIN = 10 * G.BOUNDS["bf16x3"]


@functools.lru_cache(maxsize=None)
def _layer(mode, D, widths):
    return R.layer(mode, D, widths)


def _row_case(row):
    prec, mode, D, w, K, S, kind, B, table, fast, _ = row
    convs, bns = _layer(mode, D, w)
    return (convs, bns) + G.row_inputs(row, convs, bns)


def _distinct_rows():
    """the rows of the GPU file with distinct inputs (asked precision, table feeding and fast do not change the layer)"""
    seen, out = set(), []
    for row in G.ROWS:
        key = row[1:8]
        if key not in seen:
            seen.add(key)
            out.append(row)
    return out


def _second_formulation(convs, bns, mode, xyz, feat, idx, cidx):
    B, S, K = idx.shape
    il = idx.long()
    x64 = xyz.double()

    def take(t, ix):
        return torch.gather(t, 1, ix.reshape(B, -1, 1).expand(-1, -1, t.shape[-1])).view(*ix.shape, t.shape[-1])

    ci = torch.arange(S).expand(B, S) if cidx is None else cidx.long()
    parts = [take(x64, il) - take(x64, ci).unsqueeze(2)]
    if feat is not None:
        pts = feat.double().permute(0, 2, 1)
        nb = take(pts, il)
        if mode == 0:
            cf = take(pts, ci).unsqueeze(2).expand(-1, -1, K, -1)
            parts += [cf, nb - cf]
        else:
            parts.append(nb)
    x = torch.cat(parts, dim=-1).permute(0, 3, 1, 2).contiguous()      # (B,cin,S,K)
    with torch.no_grad():
        for conv, bn in zip(convs, bns):
            x = torch.relu(copy.deepcopy(bn).double()(copy.deepcopy(conv).double()(x)))
    return x.max(dim=3)[0]


@pytest.mark.parametrize("row", _distinct_rows(), ids=G.row_id)
def test_reference_agreement_ragged_equals_k_row_and_planted_faults(row):
    prec, mode, D, w, K, S, kind, B, table, fast, _ = row
    convs, bns, xyz, feat, idx, cnt, cidx, want0 = _row_case(row)
    rows = R.sa_rows(convs, bns, mode, xyz, feat, idx, cidx)           # (B,S,K,c3)
    want = rows.max(dim=2)[0].transpose(1, 2)
    scale = float(want.abs().max())
    assert torch.equal(want, R.sa_ref(convs, bns, mode, xyz, feat, idx, cidx)) and want.shape == (B, w[2], S)
    assert torch.equal(want, want0)            # (reordering a group's entries does not move its maximum, not by a bit)
    other = _second_formulation(convs, bns, mode, xyz, feat, idx, cidx)
    assert float((other - want).abs().max()) <= 1e-12 * max(1.0, scale)
    # a group's genuine entries are distinct points
    for b in range(B):
        for s in range(0, S, max(1, S // 4)):
            n = int(cnt[b, s])
            assert len(set(idx[b, s, :n].tolist())) == n
    # ragged = K-row: the maximum over all K entries is the maximum over the first cnt
    k = torch.arange(K).view(1, 1, K, 1)
    genuine = k < cnt.view(B, S, 1, 1)
    assert torch.equal(rows.masked_fill(~genuine, 0.0).max(dim=2)[0].transpose(1, 2), want)   # (post-ReLU rows are >= 0)
    # planted faults
    moved = {}
    last = k == (cnt.view(B, S, 1, 1) - 1)
    moved["a"] = rows.masked_fill(~genuine | last, 0.0).max(dim=2)[0].transpose(1, 2)
    nxt = rows.reshape(B * S, K, -1).roll(-1, dims=0)[:, 0].reshape(B, S, -1)
    moved["b"] = torch.maximum(rows.max(dim=2)[0], nxt).transpose(1, 2)
    ci = torch.arange(S).expand(B, S) if cidx is None else cidx.long()
    prev = R.sa_rows(convs, bns, mode, xyz, feat, idx, cidx, coord_centre_idx=ci.roll(1, dims=1))
    moved["c"] = prev.max(dim=2)[0].transpose(1, 2)
    if w[2] > 128:
        moved["d"] = want.clone()
        moved["d"][:, 128:] = 0.0
    if kind is not None and bool((cnt < K).any()):
        bad = torch.where(torch.arange(K).view(1, 1, K) < cnt.unsqueeze(-1), idx, torch.zeros_like(idx))
        moved["e"] = R.sa_ref(convs, bns, mode, xyz, feat, bad, cidx)
    for name, out in sorted(moved.items()):
        d = float((out - want).abs().max()) / scale
        assert d > FAULT_MARGIN, "fault (%s) moves the reference by %.3g of its scale only" % (name, d)
    # the float32 yardstick is far inside every bound
    y32 = float((R.sa_ref32(convs, bns, mode, xyz, feat, idx, cidx).double() - want).abs().max()) / scale
    assert y32 < G.BOUNDS["f32"]


def test_row_table_matches_the_restatement_and_covers_every_reachable_instantiation():
    listed = set()
    for row in G.ROWS:
        prec, mode, D, w, K, S, kind, B, table, fast, expect = row
        d = R.dispatch(mode, D, w[0], w[1], w[2], K, R.PREC[prec], kind is not None, bool(fast))
        name = R.form_name(d)
        if d[1] == "stream_rag":
            name += ":" + R.stream_rag_variant(w[0], w[2], K, bool(table))
        assert name == expect, G.row_id(row)
        listed.add(name)
        if table:
            assert R.uses_row_table(w[0], w[1], w[2], K, R.PREC[prec]) and K % 2 == 0
        if d[1] == "krow_tile":        # S = 2 cpw + 1 (cpw + 3 where that would pass 131 centres): a partial last workgroup
            cpw = R.krow_tile_choice(w[0], w[1], w[2], K)[0]
            assert S in (2 * cpw + 1, cpw + 3) and (cpw == 1 or S % cpw != 0) and S > cpw
        assert max(64, K + 8, S if mode == 0 else 0) <= 256
    assert len({G.row_id(r) for r in G.ROWS}) == len(G.ROWS)

    # one D = 0 row per form (a K-row tile form is its template arguments without TB and the epilogue flag), and one row
    # with more clouds than XCD slots per kernel family and unit
    def form(expect):
        unit, rest = expect.split(" ")
        family, args = rest.split("<")
        if family == "krow_tile":
            args = ",".join(args.rstrip(">").split(",")[1:-1]) + ">"
        return "%s %s<%s" % (unit, family, args)
    forms = {form(r[10]) for r in G.ROWS}
    assert forms == {form(r[10]) for r in G.ROWS if r[2] == 0}, sorted(forms - {form(r[10]) for r in G.ROWS if r[2] == 0})
    families = {r[10].split("<")[0] for r in G.ROWS}
    assert families == {r[10].split("<")[0] for r in G.ROWS if r[7] == 11}
    # every instantiation the restatement reaches for K = 1 .. 192 over the listed widths, in every mode, with and without
    # features and hit counts, is a row
    widths = sorted({r[3] for r in G.ROWS})
    reach = set()
    for w in widths:
        for K in range(1, 193):
            for prec in (0, 1, 2):
                for mode, D in ((0, 8), (1, 5), (1, 0)):
                    for has_cnt in ((False, True) if mode == 1 else (False,)):
                        d = R.dispatch(mode, D, w[0], w[1], w[2], K, prec, has_cnt)
                        name = R.form_name(d)
                        if d[1] == "stream_rag":
                            reach.add(name + ":idx8")
                            name += ":" + R.stream_rag_variant(w[0], w[2], K, True)
                        reach.add(name)
    assert reach <= listed, sorted(reach - listed)
    # the 8-wave table form is reached by no shape: wherever the row table is read, the 12-wave form fits
    assert not any(n.endswith(":tab8") for n in reach)
    for c1 in (32, 64, 128):
        for c3 in (c1, 2 * c1):
            for K in range(2, 193, 2):
                if R.uses_row_table(c1, c1, c3, K, 1):
                    assert R.stream_rag_variant(c1, c3, K, True) == "tab12"


def _kernel_name(expect):
    """a row's instantiation as the kernel trace spells it (template arguments with their defaults filled in)"""
    unit, rest = expect.split(" ")
    prec = R.PREC[unit]
    family, args = rest.split("<")
    args, _, variant = args.partition(">")
    a = [x for x in args.split(",") if x]
    lo = "true" if prec == 1 else "false"
    if family == "generic":
        return "sa_mlp_kernel("
    if family == "krow_tile":
        tb, nr, w2, w3 = a[:4]
        nr2 = a[4] if len(a) > 5 else nr
        rkb = a[5] if len(a) > 6 else "0"
        img = "true" if (prec != 0 and nr2 == "1") else "false"
        return "sa_fused_kernel<%s>" % ", ".join([tb, nr, w2, w3, "true" if a[-1] == "maxe" else "false", nr2, rkb, str(prec), img])
    if family == "rag_tile":
        return "sa_rag_kernel<%s>" % ", ".join(a + [str(prec)])
    if family == "stream":
        return "sa_stream_kernel<%s>" % ", ".join(a + [lo])
    if family == "wsplit":
        return "sa_wsplit_rag_kernel<%s>" % ", ".join(a + [lo])
    assert family == "stream_rag"
    return "sa_stream_rag_kernel<%s>" % ", ".join(a + [lo] + {":idx8": ["false", "8"], ":tab12": ["true", "12"]}[variant])


def test_every_listed_instantiation_was_seen_in_the_kernel_trace():
    """profiles/r16a_sa_forms_kernels.txt: the distinct sa_* kernels of one kernel-trace run of the GPU file alone"""
    from conftest import ROOT
    seen = open(os.path.join(ROOT, "profiles", "r16a_sa_forms_kernels.txt")).read()
    wanted = {_kernel_name(r[10]) for r in G.ROWS}
    assert len(wanted) == len({r[10] for r in G.ROWS})
    missing = sorted(n for n in wanted if "::" + n not in seen)
    assert not missing, missing
    # and nothing ran that the table does not name (the ragged tile plan's helper kernels aside)
    names = {line.split("::", 1)[1].split("(")[0] for line in seen.splitlines() if line.strip()}
    extra = sorted(n for n in names if not n.startswith(("sa_rag_plan", "sa_rag_scan", "sa_rag_flatten", "sa_rag_rows")) and
                   not any(w.rstrip("(") == n for w in wanted))
    assert not extra, extra
    # the forms no shape reaches (listed as not run in the GPU file's docstring) are absent
    assert "sa_stream_kernel<1, 2" not in seen and "sa_stream_rag_kernel<1, 2" not in seen and ", true, 8>" not in seen


def test_k_row_tile_choices_span_every_tb():
    """the cost model picks TB = 4, 5, 6 at K = 112 .. 192, and 79 (TB, MAXE) pairs over the f32 unit's ten width forms"""
    pairs = set()
    for w in [(32, 32, 32), (64, 32, 32), (64, 64, 64), (128, 128, 128), (128, 128, 256), (128, 256, 256), (32, 64, 128),
              (64, 64, 256), (64, 256, 64), (128, 256, 512)]:
        for K in range(1, 193):
            d = R.dispatch(0, 8, w[0], w[1], w[2], K, 0, False)
            if d[1] == "krow_tile":         # (256 channels and more: no tile of that many rows fits, the generic kernel is left)
                pairs.add(d[2])
            else:
                assert d[1] == "generic" and max(w) >= 256 and K > 64
    assert len(pairs) == 79
    assert {R.krow_tile_choice(128, 128, 128, K)[1] for K in (112, 144, 176)} == {4, 5, 6}


def _lib():
    """the library, which needs no device for its shape queries.  Skipped only where it is not built or the loader cannot
    open it (no ROCm runtime on this host); a broken import or another ABI fails"""
    import torch  # noqa: F401  (must precede the HIP library)
    from pcr_amd import _lib as L
    if not os.path.exists(L.SO_PATH):
        pytest.skip("libpcr_hip is not built")
    try:
        return L.load()
    except OSError as e:
        pytest.skip("libpcr_hip does not load: %s" % e)


WIDTHS = [(32, 32, 32), (32, 32, 64), (64, 64, 64), (64, 64, 128), (128, 128, 128), (128, 128, 256), (64, 32, 32),
          (32, 64, 128), (64, 128, 256), (96, 96, 96), (64, 64, 96), (64, 64, 256), (64, 256, 64), (128, 256, 256),
          (128, 256, 512), (24, 40, 72), (72, 100, 120), (256, 256, 256), (128, 128, 192)]


def test_restated_rules_equal_the_exported_shape_queries():
    lib = _lib()
    for w in WIDTHS:
        for K in range(1, 193):
            for prec in (0, 1, 2):
                assert lib.pcr_sa_uses_row_table(w[0], w[1], w[2], K, prec) == R.uses_row_table(w[0], w[1], w[2], K, prec), (w, K)
                assert lib.pcr_sa_krow_uses_tiles(w[0], w[1], w[2], K, prec) == R.krow_uses_tiles(w[0], w[1], w[2], K, prec)
                for mode, D in ((0, 8), (0, 0), (1, 5)):
                    assert lib.pcr_sa_tables_take_xyz(mode, D, w[0], w[1], w[2], K, prec) == \
                        R.tables_take_xyz(mode, D, w[0], w[1], w[2], K, prec), (w, K, mode, D)
                for N in (64, 1023, 1024, 4096):
                    assert lib.pcr_sa_claim_ws_ints(w[0], w[1], w[2], K, N, prec) == R.claim_ws_ints(w[0], w[1], w[2], K, N, prec)
            for B, S in ((1, 1), (3, 33), (11, 129), (2, 1000)):
                assert lib.pcr_sa_tile_ws_ints(B, S, K, w[1], w[2]) == R.tile_ws_ints(B, S, K, w[1], w[2]), (w, K, B, S)
    # the ragged stream plan sends every layer 3 of more than two cout blocks to <2,4>: right only because no 128-wide layer
    # reads the row table (the LDS rule of sas_shape keeps them out), at any K
    for K in range(1, 1025):
        for c3 in (128, 256):
            for prec in (1, 2):
                assert lib.pcr_sa_uses_row_table(128, 128, c3, K, prec) == 0
                assert not R.sas_shape(128, 128, c3, K, True)


_DUMMY = 64         # any address that is not NULL: pcr_sa_launch_form reads pointers against NULL only


def _launch_block(lib, mode, D, w, K, asked, feed, fast, B=3, S=5, N=256):
    """the parameter block engine.SaPlan.run hands pcr_sa_mlp_f32 for such a call, every pointer a dummy.  feed: None (no hit
    counts) | "idx" (hit counts and the index tensor) | "tab" (hit counts and the ball query's row table; the index tensor
    is left out where the shape reads the table, as the engine's callers do).  Hit counts are passed in mode 1 only."""
    from pcr_amd import abi
    p = abi.SaParams()
    p.mode, p.B, p.N, p.S, p.K, p.D = mode, B, N, S, K, D
    p.c1, p.c2, p.c3 = w
    p.xyz = p.out = _DUMMY
    p.feat = _DUMMY if D else None
    for i in range(3):
        p.wp[i] = p.scale[i] = p.shift[i] = _DUMMY
    asked = asked if fast else 0
    ragged = bool(feed) and bool(fast) and mode == 1
    reads_table = ragged and feed == "tab" and lib.pcr_sa_uses_row_table(w[0], w[1], w[2], K, asked)
    p.idx = None if reads_table else _DUMMY
    tiled = ragged or bool(fast and mode == 1 and lib.pcr_sa_krow_uses_tiles(w[0], w[1], w[2], K, asked))
    if tiled and lib.pcr_sa_tile_ws_ints(B, S, K, w[1], w[2]) > 0:
        p.tile_ws = _DUMMY
    if ragged:
        p.cnt = _DUMMY
        p.row_tab = _DUMMY if feed == "tab" else None
    if fast:
        p.wa = p.wa_packed = p.wa_shift_packed = _DUMMY
        p.precision = asked
        if not ragged and lib.pcr_sa_claim_ws_ints(w[0], w[1], w[2], K, N, asked) > 0:
            p.claim_ws = _DUMMY
        for i in range(2):
            p.wps[i] = p.shift_pad[i] = p.wps_bf[i] = _DUMMY
        if D:
            p.wpq = p.pq_ws = _DUMMY
            p.pq_ready = 1
            p.pq_has_xyz = int(asked != 0 and not ragged and not tiled and
                               lib.pcr_sa_tables_take_xyz(mode, D, w[0], w[1], w[2], K, asked))
    return p


def _reported(lib, p):
    """the form the library reports for a block, as the row tables spell it; None: the launch would be refused"""
    import ctypes
    form = (ctypes.c_int * 16)(*([-1] * 16))
    status = lib.pcr_sa_launch_form(ctypes.byref(p), form)
    if status != 0:
        assert status == 1 and list(form) == [-1] * 16
        return None
    d, variant = R.from_library(list(form))
    return R.form_name(d) + (":" + variant if variant else "")


def _restated(mode, D, w, K, asked, feed, fast):
    d = R.dispatch(mode, D, w[0], w[1], w[2], K, asked, bool(feed), bool(fast))
    if d[1] == "generic" and not R.generic_fits(mode, D, w[0], w[1], w[2], K):
        return None                 # (no kernel holds the shape: PCR_ERR_INVALID)
    name = R.form_name(d)
    if d[1] == "stream_rag":
        name += ":" + R.stream_rag_variant(w[0], w[2], K, feed == "tab")
    return name


def test_the_library_reports_the_form_the_restatement_names():
    """pcr_sa_launch_form (the dispatcher's own plan, no device) against sa_ref.dispatch over WIDTHS x K = 1 .. 192 x the
    three precisions x (mode, D) x {no counts, counts with the index, counts with the row table} x fast operands or none"""
    lib = _lib()
    n = 0
    for w in WIDTHS:
        for K in range(1, 193):
            for asked in (0, 1, 2):
                for mode, D in ((0, 8), (0, 0), (1, 5)):
                    for feed in (None, "idx", "tab"):
                        want = {fast: _restated(mode, D, w, K, asked, feed, fast) for fast in (1, 0)}
                        for fast in (1, 0):
                            got = _reported(lib, _launch_block(lib, mode, D, w, K, asked, feed, fast))
                            assert got == want[fast], (w, K, asked, mode, D, feed, fast)
                            n += 1
    assert n == len(WIDTHS) * 192 * 3 * 3 * 3 * 2


def test_the_library_reports_every_row_of_the_gpu_file():
    lib = _lib()
    for row in G.ROWS:
        prec, mode, D, w, K, S, kind, B, table, fast, expect = row
        feed = None if kind is None else ("tab" if table else "idx")
        p = _launch_block(lib, mode, D, w, K, R.PREC[prec], feed, fast, B=B, S=S, N=max(64, K + 8, S if mode == 0 else 0))
        assert _reported(lib, p) == expect, G.row_id(row)
        assert _kernel_args(p, lib) == _kernel_name(expect), G.row_id(row)


def _kernel_args(p, lib):
    """the reported template arguments spelled as a kernel trace spells them (`_kernel_name`)"""
    import ctypes
    form = (ctypes.c_int * 16)()
    assert lib.pcr_sa_launch_form(ctypes.byref(p), form) == 0
    family, n = form[1], form[3]
    if family == 0:
        return "sa_mlp_kernel("
    bools = {1: (4, 8), 2: (), 3: (2,), 4: (2, 3), 5: (2,)}[family]
    args = [("true" if form[4 + i] else "false") if i in bools else str(form[4 + i]) for i in range(n)]
    kernel = ("", "sa_fused_kernel", "sa_rag_kernel", "sa_stream_kernel", "sa_stream_rag_kernel", "sa_wsplit_rag_kernel")[family]
    return "%s<%s>" % (kernel, ", ".join(args))


def test_the_form_query_refuses_what_the_launch_refuses():
    import ctypes
    lib = _lib()
    form = (ctypes.c_int * 16)()
    assert lib.pcr_sa_launch_form(None, form) == 1
    p = _launch_block(lib, 0, 8, (64, 64, 64), 16, 1, None, 1)
    assert lib.pcr_sa_launch_form(ctypes.byref(p), None) == 1
    p.pq_has_xyz, p.pq_ready = 1, 0                  # tables with the coordinate term that nobody built
    assert lib.pcr_sa_launch_form(ctypes.byref(p), form) == 1
    p = _launch_block(lib, 1, 5, (24, 40, 72), 16, 0, "tab", 1)
    p.idx = None                                     # a row table alone where only the generic kernel is left
    assert lib.pcr_sa_launch_form(ctypes.byref(p), form) == 1
