"""in ONE process: pass times of workloads on the product library and on a tagged one (lib/libpcr_hip_<TAG>.so, built with
PCR_LIB_TAG=<TAG> python -m pcr_amd.build from another checkout's sources), the two alternating, plus a checksum of the
logits under each.  The tagged library is measured twice per round (T, T'), so that the spread of a library against itself
stands next to the difference between the two.  Both libraries must carry the same ABI number.
usage: ab_lib_inproc.py TAG [workload ...]      (default: pt1024 gallery128)"""
import ctypes, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "point-cloud-reid_amd")]
import numpy as np
import torch
import bench
from pcr_amd import _lib as L
from pcr_amd import abi
from pcr_amd import testing as T

tag = sys.argv[1]
wls = sys.argv[2:] or ["pt1024", "gallery128"]
ROUNDS, ITERS = 6, 10
head = L.load()
tagged = ctypes.CDLL(os.path.join(os.path.dirname(L.SO_PATH), "libpcr_hip_%s.so" % tag))
assert tagged.pcr_abi_version() == head.pcr_abi_version()
for name, sig in abi.SIGNATURES.items():
    if hasattr(tagged, name):                       # (entry points the tagged library does not have yet are never called on it)
        fn = getattr(tagged, name)
        fn.restype, fn.argtypes = abi.prototype(sig)
LIBS = {"T": tagged, "H": head, "T'": tagged}


def passes(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    with torch.no_grad():
        for _ in range(ITERS):
            out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS, out


for wl in wls:
    desc, kind, n, bl, pairs = bench.WORKLOADS[wl]
    if wl.startswith("gallery"):
        G = max(1, int(round(pairs ** 0.5)))
        model, _ = bench.build_pt_model(bl)
        clouds = T.synthetic_clouds(2 * G, n, seed=1234, kind="randn").cuda()
        ii, jj = torch.meshgrid(torch.arange(G), torch.arange(G, 2 * G), indexing="ij")
        combos = torch.stack([ii.reshape(-1), jj.reshape(-1)], dim=1).cuda()
        with torch.no_grad():
            model.calibrate_precision(clouds[:G], clouds[G:])

        def fn():
            xyz, h = model.forward_inference(clouds)
            return model.match_gallery(h, xyz, combos)
    else:
        model, _ = bench.build_model(kind, bl)
        s1, s2 = T.synthetic_pairs(pairs, n, seed=1234, kind="box" if kind == "ssg" else "randn")
        s1, s2 = s1.cuda(), s2.cuda()
        fn = lambda: bench.hot_path(model, s1, s2)      # noqa: E731
    acc, sha = {k: [] for k in LIBS}, {}
    for k, lib in LIBS.items():                     # warm both (kernel load, LDS opt-in)
        L._lib = lib
        for _ in range(2):
            passes(fn)
    for rep in range(ROUNDS):
        for k, lib in LIBS.items():
            L._lib = lib
            ms, out = passes(fn)
            acc[k].append(ms)
            sha[k] = hashlib.sha1(out.float().cpu().numpy().tobytes()).hexdigest()[:12]
    L._lib = head
    for k in LIBS:
        print("%-10s %-3s ms/pass: %s | median %.4f  logits sha %s" % (wl, k, " ".join("%.4f" % x for x in acc[k]),
                                                                       float(np.median(acc[k])), sha[k]))
    t, h, t2 = (float(np.median(acc[k])) for k in ("T", "H", "T'"))
    print("%-10s product vs tagged %+.2f %%; tagged vs itself %+.2f %% (per-round |T - T'| up to %.2f %%); same logits: %s" % (
        wl, 100 * (h - 0.5 * (t + t2)) / (0.5 * (t + t2)), 100 * (t2 - t) / t,
        100 * max(abs(a - b) / a for a, b in zip(acc["T"], acc["T'"])), sha["T"] == sha["H"]))
