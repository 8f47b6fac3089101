"""Does a tagged library compute the bits the product library computes, launch form by launch form?  The check of a refactor
of the set-abstraction dispatch: every row of tests/test_gpu_sa_forms.ROWS (one per reachable kernel instantiation) is run
once on lib/libpcr_hip_<TAG>.so -- built with PCR_LIB_TAG=<TAG> python -m pcr_amd.build in a checkout of the other revision
and copied here -- and once on the product library, and the CRC-32 of each output and the arithmetic unit the launch noted
are listed side by side.

  python tools/ab/ab_sa_forms.py TAG            (on an MI355X; exit status 1 on any difference or failed child)

Each library runs in a fresh child process under its own time limit; the second child is not started when the first one
did not end cleanly.  Entry points the tagged library does not have yet are left out of the binding in its child."""
import ctypes, os, subprocess, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_LIMIT = 420           # seconds: 436 rows, their float64 inputs included, took under a minute


def child():
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "point-cloud-reid_amd")]
    import torch
    from pcr_amd import _lib as L
    from pcr_amd import abi
    probe = ctypes.CDLL(L.SO_PATH)
    for name in [n for n in abi.SIGNATURES if not hasattr(probe, n)]:
        print("# %s is not in %s" % (name, os.path.basename(L.SO_PATH)))
        del abi.SIGNATURES[name]
    from pcr_amd import engine
    import test_gpu_sa_forms as G
    import sa_ref as R
    lib = L.load()
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
        print("ROW %s %08x %d" % (G.row_id(row), zlib.crc32(out.cpu().contiguous().numpy().tobytes()), arith), flush=True)


def run_child(tag):
    env = dict(os.environ, PCR_LIB_TAG=tag)
    if not tag:
        env.pop("PCR_LIB_TAG")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=CHILD_LIMIT)
    rows = dict(l.split(" ", 2)[1:] for l in r.stdout.splitlines() if l.startswith("ROW "))
    for l in r.stdout.splitlines():
        if l.startswith("# "):
            print(l)
    if r.returncode != 0:
        print("child on library '%s' ended with status %d after %d rows:\n%s" % (tag or "product", r.returncode, len(rows),
                                                                                 r.stderr[-2000:]))
        sys.exit(1)
    return rows


def main(tag):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    base, new = run_child(tag), run_child("")
    bad = 0
    for rid in sorted(set(base) | set(new)):
        a, b = base.get(rid, "-"), new.get(rid, "-")
        bad += a != b
        print("%-52s %-12s %-12s %s" % (rid, a, b, "SAME" if a == b else "DIFFERENT"))
    print("%d rows (output CRC-32, arithmetic unit): %d differ between libpcr_hip_%s.so and libpcr_hip.so" % (
        len(set(base) | set(new)), bad, tag))
    return 1 if bad or not base else 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main(sys.argv[1]))
