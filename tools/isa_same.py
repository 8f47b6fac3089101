"""Is the device code of this tree the device code of BASE_REV?  The check of a refactor of the kernel library.

  python tools/isa_same.py BASE_REV

Exports csrc/ and include/ of BASE_REV (git archive) to a temporary directory, compiles every *.hip of both trees to gfx950
device assembly with the build's own flags for that file (pcr_amd.build.compile_flags, PCR_EXTRA_HIPCC_FLAGS included) plus
--cuda-device-only -S -fuse-cuid=none, and compares the texts.  -fuse-cuid=none takes out the one symbol that differs between
two compiles of an unchanged file; the include directory's path does not enter the text.  One verdict per file, the first
differing kernel where two files differ; exit status 1 on any difference, added and removed files included.

It compares and nothing else: what the instructions are is not its business."""
import concurrent.futures, io, os, re, subprocess, sys, tarfile, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-reid_amd"))
from pcr_amd import build

REL_CSRC = os.path.relpath(build.CSRC, ROOT)


def assemble(src, root, out):
    cmd = [build.hipcc()] + build.compile_flags(src, root) + ["--cuda-device-only", "-S", "-fuse-cuid=none", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stderr))
    return open(out).read()


def first_difference(a, b):
    """the symbol that the first differing line of two assembly texts lies under, and the two lines"""
    la, lb = a.split("\n"), b.split("\n")
    n = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
    sym = next((m.group(1) for m in (re.match(r"^(\w+):", l) for l in reversed(la[:n + 1])) if m and not m.group(1).startswith("BB")),
               "(file header)")
    return sym, (la[n] if n < len(la) else "<end>").strip(), (lb[n] if n < len(lb) else "<end>").strip()


def main(rev):
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, REL_CSRC, "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "base"))
        trees = {"base": os.path.join(tmp, "base"), "new": ROOT}
        names = {k: {f for f in os.listdir(os.path.join(r, REL_CSRC)) if f.endswith(".hip")} for k, r in trees.items()}
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            jobs = {(k, f): pool.submit(assemble, os.path.join(trees[k], REL_CSRC, f), trees[k], os.path.join(tmp, k + "_" + f + ".s"))
                    for k in trees for f in sorted(names[k])}
            text = {key: j.result() for key, j in jobs.items()}
    bad = 0
    for f in sorted(names["base"] | names["new"]):
        if f not in names["new"] or f not in names["base"]:
            print("%-28s %s" % (f, "REMOVED" if f in names["base"] else "NEW"))
            bad += 1
        elif text["base", f] == text["new", f]:
            print("%-28s identical (%d lines)" % (f, text["new", f].count("\n")))
        else:
            print("%-28s DIFFERS, first in %s:\n    base: %s\n    new:  %s" % ((f,) + first_difference(text["base", f], text["new", f])))
            bad += 1
    print("%d files, %d not identical to %s; %.0f s" % (len(names["base"] | names["new"]), bad, rev, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
