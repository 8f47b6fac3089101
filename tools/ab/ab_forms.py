"""Does a tagged library compute the bits the product library computes, launch form by launch form?  The check of a refactor
of a dispatcher.  lib/libpcr_hip_<TAG>.so -- built with PCR_LIB_TAG=<TAG> python -m pcr_amd.build in a checkout of the other
revision and copied here -- and the product library each run every row of a family's tables once, and what they wrote and the
arithmetic the launches noted are listed side by side.

  python tools/ab/ab_forms.py sa TAG      every row of tests/test_gpu_sa_forms.ROWS (one per reachable kernel instantiation):
                                          CRC-32 of the output, arithmetic unit
  python tools/ab/ab_forms.py attn TAG    every entry of tests/test_gpu_attn_forms.EXPECT in both modes and every gated row of
                                          tests/test_gpu_match_live.py (GATED, TWINS): CRC-32 of the kv image and of the
                                          output, the arithmetic noted by the kv and by the apply launch
  (on an MI355X; exit status 1 on any difference or failed child)

Each library runs in a fresh child process under its own time limit; the second child is not started when the first one
did not end cleanly.  Entry points the tagged library does not have yet are left out of the binding in its child."""
import ctypes, os, subprocess, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_LIMIT = 420           # seconds: the 436 SA rows, their float64 inputs included, took under a minute


def crc(t):
    return "%08x" % zlib.crc32(t.cpu().contiguous().numpy().tobytes())


def sa_rows(lib):
    import torch
    from pcr_amd import engine
    import test_gpu_sa_forms as G
    import sa_ref as R
    for row in G.ROWS:
        prec, mode, D, w, K, S, kind, B, table, fast, expect = row
        convs, bns, plan = G._plan(mode, D, w, fast)
        xyz, feat, idx, cnt, cidx, _ = G.row_inputs(row, convs, bns)
        dev = lambda t: None if t is None else t.cuda()     # noqa: E731
        kw = dict(centre_idx=dev(cidx))
        if kind is not None:
            kw["cnt"] = dev(cnt)
        with engine.precision(prec), torch.no_grad():
            if kind is not None and table:
                out = plan.run(dev(xyz), dev(feat), None, rows=dev(R.row_table(xyz, idx, cnt, cidx)), K=K, **kw)
            else:
                out = plan.run(dev(xyz), dev(feat), dev(idx), **kw)
            arith = lib.pcr_last_launch_arith()
        yield G.row_id(row), "%s %d" % (crc(out), arith)


def attn_rows(lib):
    import torch
    from pcr_amd import _lib as L
    from pcr_amd import engine
    import test_gpu_attn_forms as G
    import test_gpu_match_live as ML
    for key, case, prec, splits, pooled in G.table_rows():
        m = G._gpu_module(case)
        args = G._dev(G.case_data(case))
        prev, engine.KV_SPLITS = engine.KV_SPLITS, splits
        try:
            with engine.precision(prec), torch.no_grad():
                kv = G._plan(case, m, args).kv(args[2], args[3])
                a_kv = lib.pcr_last_launch_arith()
                try:
                    out, a_out = crc(G.run(case, m, args, pooled=pooled)), lib.pcr_last_launch_arith()
                except L.PcrError:
                    out, a_out = "refused", -1
        finally:
            engine.KV_SPLITS = prev
        yield "%s %s" % (key, prec), "%s %d %s %d" % (crc(kv), a_kv, out, a_out)
    gated = [(("cross", 2, 0, Ln, prec), want) for (Ln, prec), want in ML.GATED.items()] + list(ML.TWINS.items())
    for (kind, nhead, cfinal, Ln, prec), want in gated:
        case = ML.gated_case(kind, nhead, cfinal, Ln)
        plan = G.host_plan(case, "cuda")
        g = torch.Generator().manual_seed(Ln + nhead)
        feat, xyz = torch.randn(case.B, 64, Ln, generator=g).cuda(), torch.randn(case.B, Ln, 3, generator=g).cuda()
        live = (ML.dev_count(5), ML.PERIOD, 3)
        with engine.precision(prec), torch.no_grad():
            state = plan.kv(feat, xyz)
            kv = plan.kv(feat, xyz, live=live, out=torch.full_like(state, ML.SENTINEL))
            a_kv = lib.pcr_last_launch_arith()
            xq = xyz if plan.q_pos else None
            shape = plan.apply(feat, xq, state, Ln)
            outs = [plan.apply(feat, xq, state, Ln, live=live, out=torch.full_like(shape, ML.SENTINEL))]
            if want[2]:
                outs.append(plan.apply(feat, xq, state, Ln, pooled=True, live=live))
            a_out = lib.pcr_last_launch_arith()
        yield "%s %s gated" % (case.name, prec), "%s %d %s %d" % (crc(kv), a_kv, "+".join(crc(o) for o in outs), a_out)


FAMILIES = {"sa": sa_rows, "attn": attn_rows}


def child(family):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "point-cloud-reid_amd"), os.path.join(ROOT, "oracle")]
    from pcr_amd import _lib as L
    from pcr_amd import abi
    probe = ctypes.CDLL(L.SO_PATH)
    for name in [n for n in abi.SIGNATURES if not hasattr(probe, n)]:
        print("# %s is not in %s" % (name, os.path.basename(L.SO_PATH)))
        del abi.SIGNATURES[name]
    for rid, what in FAMILIES[family](L.load()):
        print("ROW %s | %s" % (rid, what), flush=True)


def run_child(family, tag):
    env = dict(os.environ, PCR_LIB_TAG=tag)
    if not tag:
        env.pop("PCR_LIB_TAG")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", family], env=env, capture_output=True, text=True,
                       timeout=CHILD_LIMIT)
    rows = dict(l[4:].split(" | ") for l in r.stdout.splitlines() if l.startswith("ROW "))
    for l in r.stdout.splitlines():
        if l.startswith("# "):
            print(l)
    if r.returncode != 0:
        print("child on library '%s' ended with status %d after %d rows:\n%s" % (tag or "product", r.returncode, len(rows),
                                                                                 r.stderr[-2000:]))
        sys.exit(1)
    return rows


def main(family, tag):
    base, new = run_child(family, tag), run_child(family, "")
    bad = 0
    for rid in sorted(set(base) | set(new)):
        a, b = base.get(rid, "-"), new.get(rid, "-")
        bad += a != b
        print("%-52s %-30s %-30s %s" % (rid, a, b, "SAME" if a == b else "DIFFERENT"))
    print("%d rows: %d differ between libpcr_hip_%s.so and libpcr_hip.so" % (len(set(base) | set(new)), bad, tag))
    return 1 if bad or not base else 0


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in list(FAMILIES) + ["--child"]:
        sys.exit(__doc__)
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1], sys.argv[2]))
