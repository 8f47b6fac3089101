"""Before / after comparison of the compiled kernels of a refactor: resources and per-kernel mnemonic histograms.

  python tools/isa_diff.py emit OUTDIR [source.hip ...]   device assembly + resource remarks of the sources (default:
                                                          point_ops, crop_kernels, assoc_kernels) with the build's flags
  python tools/isa_diff.py compare DIR_A DIR_B            the kernels whose resources or histograms differ

Run `emit` on a checkout of the parent and on the working tree, then `compare`.  Every mnemonic is counted alike."""
import collections, glob, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-cloud-reid_amd", "csrc")
RES = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"),
       ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
       ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def emit(outdir, srcs):
    sys.path.insert(0, os.path.join(ROOT, "point-cloud-reid_amd", "pcr_amd"))
    import build
    os.makedirs(outdir, exist_ok=True)
    for src in srcs:
        base = os.path.basename(src)
        stem = os.path.splitext(base)[0]
        cmd = [build.hipcc()] + build.compile_flags(src) + \
              ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o",
               os.path.join(outdir, stem + ".s")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        with open(os.path.join(outdir, stem + ".res"), "w") as f:
            f.write(r.stderr)


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in RES:
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def histograms(path):
    """{kernel symbol: Counter(mnemonic)} of the functions of a .s file"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            cur = out.setdefault(m.group(1), collections.Counter())
            continue
        if re.match(r"^\s*\.(Lfunc_end|size|section|text|rodata|amdhsa_kernel)", line):
            if ".Lfunc_end" in line:
                cur = None
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", line)
        if m and cur is not None:
            cur[m.group(1)] += 1
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::|void ", "", d).split("(")[0] for n, d in zip(names, r)}


def compare(a, b):
    nk = nd = 0
    for sa in sorted(glob.glob(os.path.join(a, "*.s"))):
        base = os.path.basename(sa)
        sb = os.path.join(b, base)
        if not os.path.exists(sb):
            continue
        ra, rb = resources(sa[:-2] + ".res"), resources(sb[:-2] + ".res")
        ha, hb = histograms(sa), histograms(sb)
        names = demangle(sorted(set(ra) | set(rb)))
        print("== %s: %d kernels" % (base[:-2], len(names)))
        for k in sorted(names):
            nk += 1
            lines = []
            if k not in ra or k not in rb:
                lines.append("  only in %s" % (a if k in ra else b))
            else:
                if ra[k] != rb[k]:
                    lines.append("  RESOURCES %s -> %s" % (ra[k], rb[k]))
                for mn in sorted(set(ha.get(k, {})) | set(hb.get(k, {}))):
                    ca, cb = ha.get(k, {}).get(mn, 0), hb.get(k, {}).get(mn, 0)
                    if ca != cb:
                        lines.append("  %-28s %6d -> %6d" % (mn, ca, cb))
                ta, tb = sum(ha.get(k, {}).values()), sum(hb.get(k, {}).values())
                if lines:
                    lines.append("  %-28s %6d -> %6d" % ("(instructions)", ta, tb))
            if lines:
                nd += 1
                r = ra.get(k) or rb.get(k)
                print("%s  [vgpr %s sgpr %s lds %s occ %s]" % (names[k], r.get("vgpr"), r.get("sgpr"), r.get("lds"), r.get("occ")))
                print("\n".join(lines))
    print("%d kernels compared, %d differ" % (nk, nd))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3:] or [os.path.join(CSRC, n) for n in ("point_ops.hip", "crop_kernels.hip", "assoc_kernels.hip")])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
