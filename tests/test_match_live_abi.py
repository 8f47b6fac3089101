"""CPU: the gated launches' part of the C ABI (include/pcr.h, pcr_live): the four entry points are exported and carried by
pcr_amd/abi.py, pcr_live is laid out as the header says, and the addition did not move the ABI number."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

ENTRY_POINTS = ("pcr_attn_live_ok", "pcr_attn_kv_live_f32", "pcr_attn_apply_live_f32", "pcr_pool_head_live_f32")


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcr.h")).read(), flags=re.S)


def test_the_gated_entry_points_are_declared_and_exported(lib):
    text = header()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared in pcr.h" % name
        assert hasattr(lib, name), "libpcr_hip.so does not export %s" % name
    assert lib.pcr_abi_version() == 17                       # additive: the number stays


def test_the_binding_carries_them():
    from pcr_amd import abi
    assert abi.SIGNATURES["pcr_attn_live_ok"] == "i <AttnParams>"
    assert abi.SIGNATURES["pcr_attn_kv_live_f32"] == "s <AttnParams><LiveParams>S"
    assert abi.SIGNATURES["pcr_attn_apply_live_f32"] == "s <AttnParams><LiveParams>S"
    assert abi.kinds(abi.SIGNATURES["pcr_pool_head_live_f32"])[1][:2] == ["<HeadParams>", "<LiveParams>"]
    assert abi.BLOCKS["pcr_live"] is abi.LiveParams
    for name in ENTRY_POINTS:
        restype, argtypes = abi.prototype(abi.SIGNATURES[name])
        assert restype is ctypes.c_int and argtypes[0]._type_ in (abi.AttnParams, abi.HeadParams)
    # the un-gated blocks are what they were: the gate travels beside them, not in them
    assert "live" not in " ".join(n for n, _ in abi.AttnParams._fields_ + abi.HeadParams._fields_)


def test_pcr_live_is_laid_out_as_the_header_says(tmp_path):
    from pcr_amd import abi
    from test_abi import _host_clang
    fields = ("count", "period", "offset")
    assert tuple(n for n, _ in abi.LiveParams._fields_) == fields
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pcr.h"', 'int main(void) {',
             '  printf("%zu\\n", sizeof(pcr_live));']
    lines += ['  printf("%%zu %%zu\\n", offsetof(pcr_live, %s), sizeof(((pcr_live *)0)->%s));' % (f, f) for f in fields]
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run([_host_clang(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.LiveParams) == 16
    for i, f in enumerate(fields):
        d = getattr(abi.LiveParams, f)
        assert (d.offset, d.size) == (int(out[1 + 2 * i]), int(out[2 + 2 * i])), f
    assert [getattr(abi.LiveParams, f).offset for f in fields] == [0, 8, 12]
