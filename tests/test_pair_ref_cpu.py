"""CPU: tests/pair_ref.py held to account before tests/test_gpu_pair_head.py relies on it.  The two float64 forms of the
pair head (on the gathered rows with torch's own linear / group_norm; split into the per-object tables u[i] + v[j]) agree
to 1e-12; the split form in float32 torch arithmetic meets the GPU bound with a factor 2 to spare on the GPU file's inputs;
planted faults -- what a kernel with a bookkeeping slip would compute -- move the result by at least ten times that bound;
the restated shape rule against the library's export (the library loads without a device); and the new parameter block of
pcr_amd/abi.py against the header as the host compiler lays it out."""
import ctypes
import os
import subprocess

import pytest
import torch

import pair_ref as R
from conftest import ROOT

ROWS = [(128, 32, 37), (64, 16, 5), (32, 8, 1)]          # (F, groups, M) of tests/test_gpu_pair_head.py
SCALES = (1.0, 3.0)


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("Fw,groups,M", ROWS + [(64, 32, 9), (128, 8, 4), (32, 2, 3)])
def test_the_two_float64_forms_agree(Fw, groups, M):
    for scale in SCALES:
        inp = R.make_inputs(Fw, groups, M, seed=Fw + M, scale=scale)
        pairs = R.make_pairs(M, 200, seed=M)
        a, b = R.head_direct(inp, pairs), R.head_split(inp, pairs)
        assert a.dtype == b.dtype == torch.float64 and a.shape == (200,)
        assert R.err(b, a) < 1e-12, R.err(b, a)


@pytest.mark.parametrize("Fw,groups,M", ROWS)
def test_float32_reference_arithmetic_meets_the_bound_with_room(Fw, groups, M):
    worst = 0.0
    for scale in SCALES:
        for seed in range(4):
            inp = R.make_inputs(Fw, groups, M, seed=seed, scale=scale)
            pairs = R.make_pairs(M, 1000, seed=seed)
            ref = R.head_direct(inp, pairs)
            worst = max(worst, R.err(R.head_split(inp, pairs, dtype=torch.float32), ref))
    print("F=%d groups=%d: float32 split form err %.3g (bound %.3g)" % (Fw, groups, worst, R.BOUND))
    assert worst <= R.BOUND / 2, worst


@pytest.mark.parametrize("Fw,groups,M", ROWS[:2] + [(32, 8, 6)])
@pytest.mark.parametrize("fault", R.FAULTS + ("mean_pooled",))
def test_planted_faults_are_caught_at_ten_times_the_bound(Fw, groups, M, fault):
    for scale in SCALES:
        inp = R.make_inputs(Fw, groups, M, seed=3, scale=scale)
        pairs = R.make_pairs(M, 300, seed=3)
        pairs = pairs[pairs[:, 0] != pairs[:, 1]] if fault == "residual_swapped" else pairs
        ref = R.head_direct(inp, pairs)
        if fault == "mean_pooled":
            bad = R.head_split(R.make_inputs(Fw, groups, M, seed=3, scale=scale, pooled="mean"), pairs)
        else:
            bad = R.head_split(inp, pairs, fault=fault)
        assert R.err(bad, ref) >= 10 * R.BOUND, (fault, R.err(bad, ref))


def test_shape_rule_matches_the_library(lib):
    yes = 0
    for Fw in (0, 1, 16, 31, 32, 33, 48, 64, 96, 128, 129, 256):
        for groups in (-1, 0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 256):
            assert lib.pcr_pair_head_ok(Fw, groups) == R.pair_head_ok(Fw, groups), (Fw, groups)
            yes += R.pair_head_ok(Fw, groups)
    assert yes == 12                                      # three widths x four group sizes
    assert R.pair_head_ok(128, 32) and not R.pair_head_ok(48, 12) and not R.pair_head_ok(64, 64)


def test_invalid_arguments_return_status(lib):
    from pcr_amd import abi
    assert lib.pcr_pair_head_f32(None, None, None, None) == 1
    p = abi.PairHeadParams()
    p.M, p.F, p.n, p.groups, p.P = 4, 48, 96, 12, 8        # a refused width: before any pointer is looked at
    assert lib.pcr_pair_head_f32(ctypes.byref(p), None, None, None) == 1
    p.F, p.n, p.groups = 64, 128, 16                       # a covered shape, but no tensors
    assert lib.pcr_pair_head_f32(ctypes.byref(p), None, None, None) == 1
    p.P = 0                                                # nothing to score: nothing is launched
    assert lib.pcr_pair_head_f32(ctypes.byref(p), None, None, None) == 0
    p.n = 64                                               # n != 2F
    assert lib.pcr_pair_head_f32(ctypes.byref(p), None, None, None) == 1


def test_parameter_block_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of pcr_pair_head_params as the host compiler lays the header out against the ctypes mirror"""
    from pcr_amd import abi, build
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    clang = next(c for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "llvm", "bin", "clang"))
                 if os.path.exists(c))
    ct = abi.PairHeadParams
    names = [n for n, _ in ct._fields_]
    assert names == ["M", "F", "n", "groups", "P", "emb", "u", "v", "pairs", "w2p", "gn1_g", "gn1_b", "gn2_g", "gn2_b",
                     "w_out", "b_out", "logits"]
    assert ct.ELEM == dict({k: torch.float32 for k in names[5:]}, pairs=torch.int32)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pcr.h"', 'int main(void) {',
             '  printf(". %zu 0\\n", sizeof(pcr_pair_head_params));']
    for f in names:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(pcr_pair_head_params, %s), sizeof(((pcr_pair_head_params *)0)->%s));'
                     % (f, f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run([clang, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    seen = 0
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        f, off, size = line.split()
        if f == ".":
            assert ctypes.sizeof(ct) == int(off)
            continue
        d = getattr(ct, f)
        assert (d.offset, d.size) == (int(off), int(size)), (f, d.offset, d.size, off, size)
        seen += 1
    assert seen == len(names)
