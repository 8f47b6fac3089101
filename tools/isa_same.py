"""Is the device code of this tree the device code of BASE_REV?  The check of a refactor of the kernel library.

  python tools/isa_same.py BASE_REV [FILE.hip ...]      (no files named: every source)

Exports csrc/ and include/ of BASE_REV (git archive) to a temporary directory, compiles every *.hip of both trees to gfx950
device assembly with the build's own flags for that file (pcr_amd.build.compile_flags, PCR_EXTRA_HIPCC_FLAGS included) plus
--cuda-device-only -S -fuse-cuid=none, and compares the texts.  -fuse-cuid=none takes out the one symbol that differs between
two compiles of an unchanged file; the include directory's path does not enter the text.  One verdict per file, the first
differing kernel where two files differ; exit status 1 on any difference, added and removed files included.

The set-abstraction and attention units (BY_SYMBOL) instantiate their kernels from host code, and the compiler emits templates in the
order the host code first names them: a change of the dispatcher alone reorders the text.  Where the texts of one of those
files differ, it is compared symbol by symbol instead: the same set of function symbols, each body identical once the
function-index numbers in local labels (.LBB12_3, .Lfunc_end12) and the comments are taken out, each kernel's
.amdhsa_kernel block and metadata entry identical.  The verdict then reads "identical by symbol".

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


BY_SYMBOL = ("sa_kernels.hip", "sa_kernels_bf1.hip", "sa_kernels_bf3.hip", "attn_kernels.hip", "attn_kernels_bf3.hip")


def symbols(text):
    """{symbol: (body, .amdhsa_kernel block or "", metadata entry or "")} of an assembly text, local labels' function
    indices normalised and comments dropped (the compiler's loop comments name blocks by function index, and their padding
    follows the label's length)"""
    def norm(t):         # .LBB12_3 -> .LBB#_3, .Lfunc_end12 -> .Lfunc_end#
        return re.sub(r"(\.L[A-Za-z_]+)\d+", r"\1#", re.sub(r"[ \t]*;[^\n]*", "", t))
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n", text, flags=re.M | re.S):
        body = m.group(2)
        hsa = re.search(r"^\s*\.amdhsa_kernel %s\n.*?^\s*\.end_amdhsa_kernel\n" % re.escape(m.group(1)), body, flags=re.M | re.S)
        out[m.group(1)] = [norm(body), hsa.group(0) if hsa else "", ""]
    meta = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", text, flags=re.M | re.S)
    for entry in re.split(r"^(?=  - )", meta.group(1) if meta else "", flags=re.M):
        name = re.search(r"^\s+\.name:\s+(\w+)$", entry, flags=re.M)
        if name and name.group(1) in out:
            out[name.group(1)][2] = entry
    return {k: tuple(v) for k, v in out.items()}


def symbol_difference(a, b):
    """None where two texts hold the same symbols with the same bodies, kernel descriptors and metadata; else what differs"""
    sa, sb = symbols(a), symbols(b)
    if sorted(sa) != sorted(sb):
        return "symbols only in base: %s; only in new: %s" % (sorted(set(sa) - set(sb))[:3], sorted(set(sb) - set(sa))[:3])
    kernels = [k for k in sa if sa[k][1]]
    if not kernels or any(not sa[k][2] or not sb[k][2] for k in kernels):
        return "no kernel descriptors or metadata entries found: the assembly's layout is not what this tool reads"
    for k in sorted(sa):
        for what, x, y in zip(("body", ".amdhsa_kernel block", "metadata"), sa[k], sb[k]):
            if x != y:
                return "%s of %s" % (what, k)
    return None


def first_difference(a, b):
    """the symbol that the first differing line of two assembly texts lies under, and the two lines"""
    la, lb = a.split("\n"), b.split("\n")
    n = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
    sym = next((m.group(1) for m in (re.match(r"^(\w+):", l) for l in reversed(la[:n + 1])) if m and not m.group(1).startswith("BB")),
               "(file header)")
    return sym, (la[n] if n < len(la) else "<end>").strip(), (lb[n] if n < len(lb) else "<end>").strip()


def main(rev, only=()):
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, REL_CSRC, "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "base"))
        trees = {"base": os.path.join(tmp, "base"), "new": ROOT}
        names = {k: {f for f in os.listdir(os.path.join(r, REL_CSRC)) if f.endswith(".hip") and (not only or f in only)}
                 for k, r in trees.items()}
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
        elif f in BY_SYMBOL and symbol_difference(text["base", f], text["new", f]) is None:
            n = symbols(text["new", f])
            print("%-28s identical by symbol (%d functions, %d of them kernels, in another order)" % (
                f, len(n), sum(1 for v in n.values() if v[1])))
        else:
            if f in BY_SYMBOL:
                print("%-28s by symbol: %s" % (f, symbol_difference(text["base", f], text["new", f])))
            print("%-28s DIFFERS, first in %s:\n    base: %s\n    new:  %s" % ((f,) + first_difference(text["base", f], text["new", f])))
            bad += 1
    print("%d files, %d not identical to %s; %.0f s" % (len(names["base"] | names["new"]), bad, rev, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2:]))
