"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/pcr.h
declares (no compute calls without a GPU); host-side weight packing round-trips; the Python description of the ABI
(pcr_amd/abi.py) agrees with the header, prototype by prototype and field by field."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pcr_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
    assert lib.pcr_abi_version() == 17
    assert lib.pcr_status_string(0) == b"ok"


def header_text():
    """include/pcr.h without comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcr.h")).read(), flags=re.S)


def header_structs(types=False):
    """{struct name: [field names in order]} of every `typedef struct NAME { ... } NAME;` of the header; with types, {struct
    name: {field: what a pointer field points at ("float", "int", "double", "long long", "void"), None for a scalar}}"""
    out = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \w+;", header_text(), flags=re.S):
        names, elem = [], {}
        for decl in body.split(";"):
            ty = re.match(r"\s*(?:const\s+)?(long long|\w+)", decl)
            for d in decl.split(","):
                m = re.search(r"(\*?)\s*(?:const\s+)?(\w+)\s*(?:\[\d+\])?\s*$", d)
                if m:
                    names.append(m.group(2))
                    elem[m.group(2)] = ty.group(1) if m.group(1) else None
        out[name] = elem if types else names
    return out


def header_prototypes():
    """{function: (return kind, [parameter kinds])} in abi.SIGNATURES' letters, except that a status return reads "i"
    (the header says `int` for both) and a pointer to a struct reads <struct name of the header>"""
    text = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", header_text(), flags=re.S)
    scalar = {"int": "i", "float": "f", "long": "l", "pcr_stream_t": "S"}
    out = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?(?:int|long|char)\s*\*?)\s*(pcr_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        kinds = []
        for p in [q.strip() for q in params.split(",")]:
            if p == "void":
                continue
            ty, star, _ = re.match(r"(.*?)(\*?)\s*(\w+)$", re.sub(r"\b(const|struct)\b", "", p).strip()).groups()
            ty = " ".join(ty.split())
            if not star:
                kinds.append(scalar[ty])
            else:
                kinds.append({"float": "F", "int": "I"}.get(ty, "<%s>" % ty if ty.startswith("pcr_") else "P"))
        out[name] = ({"int": "i", "long": "l", "char*": "c"}[ret.replace("const", "").replace(" ", "")], kinds)
    return out


def test_signature_table_matches_the_header():
    from pcr_amd import abi
    protos = header_prototypes()
    assert len(protos) >= 120, len(protos)
    assert sorted(protos) == declared_symbols()          # (the prototype regex missed none of the declared names)
    assert sorted(abi.SIGNATURES) == sorted(protos)
    n_float = n_long = 0
    for name, (ret, want) in protos.items():
        got_ret, got = abi.kinds(abi.SIGNATURES[name])
        # a pointer to one of the eleven parameter blocks names its ctypes mirror; any other struct (the records of a
        # device table) is an untyped pointer
        want = [("<%s>" % abi.BLOCKS[k[1:-1]].__name__ if k[1:-1] in abi.BLOCKS else "P") if k[0] == "<" else k for k in want]
        assert got == want, (name, got, want)
        assert {"s": "i"}.get(got_ret, got_ret) == ret, (name, got_ret, ret)
        n_float += want.count("f")
        n_long += want.count("l")
        restype, argtypes = abi.prototype(abi.SIGNATURES[name])
        assert len(argtypes) == len(want)
    assert (n_float, n_long) == (22, 5)                  # (what the header holds today: the kinds are really told apart)


def test_block_pointer_fields_carry_the_header_element_types():
    """ELEM of every parameter block (what `abi.fill` checks a tensor's dtype against) is the header's pointer type, field
    by field; a scalar field has no entry"""
    import torch
    from pcr_amd import abi
    kinds = {"float": torch.float32, "int": torch.int32, "double": torch.float64, "long long": torch.int64, "void": None}
    fields = header_structs(types=True)
    total = dict.fromkeys(kinds, 0)
    for s, elem in fields.items():
        for f, ty in elem.items():
            if ty is not None:
                assert ty in kinds, (s, f, ty)
                total[ty] += 1
        if s in abi.BLOCKS:
            want = {f: kinds[ty] for f, ty in elem.items() if ty is not None}
            assert abi.BLOCKS[s].ELEM == want, (s, {f: (abi.BLOCKS[s].ELEM.get(f, "scalar"), want.get(f, "scalar"))
                                                    for f in set(want) | set(abi.BLOCKS[s].ELEM)
                                                    if abi.BLOCKS[s].ELEM.get(f, "scalar") != want.get(f, "scalar")})
    # (what the header holds today, the two device-table records included: the regex misses no kind)
    assert total == {"float": 177, "int": 105, "double": 4, "long long": 1, "void": 1}, total


def _host_clang():
    from pcr_amd import build
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "llvm", "bin", "clang")):
        if os.path.exists(cand):
            return cand
    raise AssertionError("no host clang beside %s (the library build needs it too)" % build.hipcc())


def test_parameter_block_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of every field of every parameter block and device-table record, as the host compiler lays the
    header out, against the ctypes mirrors and numpy dtypes of pcr_amd/abi.py"""
    import subprocess
    from pcr_amd import abi
    fields = header_structs()
    assert sorted(fields) == sorted(list(abi.BLOCKS) + list(abi.TABLES))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pcr.h"', 'int main(void) {']
    for s, names in fields.items():
        lines.append('  printf("%s . %%zu 0\\n", sizeof(%s));' % (s, s))
        for f in names:
            lines.append('  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run([_host_clang(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    compared = 0
    seen = {s: [] for s in fields}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, off, size = line.split()
        off, size = int(off), int(size)
        if s in abi.BLOCKS:
            ct = abi.BLOCKS[s]
            if f == ".":
                assert ctypes.sizeof(ct) == off, (s, ctypes.sizeof(ct), off)
                continue
            d = getattr(ct, f)
            assert (d.offset, d.size) == (off, size), (s, f, d.offset, d.size, off, size)
        else:
            dt = abi.TABLES[s]
            if f == ".":
                assert dt.itemsize == off, (s, dt.itemsize, off)
                continue
            assert (dt.fields[f][1], dt.fields[f][0].itemsize) == (off, size), (s, f, dt.fields[f], off, size)
        seen[s].append(f)
        compared += 1
    for s, names in fields.items():                      # the header's names, all of them, in the header's order
        assert seen[s] == names
        have = [n for n, _ in abi.BLOCKS[s]._fields_] if s in abi.BLOCKS else list(abi.TABLES[s].names)
        assert have == names, (s, have, names)
    assert compared >= 250, compared


def test_boundary_refuses_wrong_tensors_before_the_call(lib):
    import torch
    for bad in ((torch.zeros(1, 8, 3), None, None),                                  # a CPU tensor
                (torch.zeros(1, 8, 3, dtype=torch.float64), None, None),             # float64 in a float * slot
                (None, None, torch.zeros(1, 4, dtype=torch.int64))):                 # int64 in an int * slot
        with pytest.raises(ctypes.ArgumentError):
            lib.pcr_fps_f32(*bad, 1, 8, 4, None)
    assert lib.pcr_fps_f32(None, None, None, 1, 8, 4, None) == 1
    with pytest.raises(ctypes.ArgumentError):                                        # a byref of the wrong block
        from pcr_amd import abi
        lib.pcr_sa_mlp_f32(ctypes.byref(abi.HeadParams()), None)
    # plain Python numbers go in as the header types them: a float in a float slot, a stride past 2^31 in a long slot
    assert lib.pcr_ball_query_f32(None, None, None, 1, 8, 4, 0.0, 0.5, 4, None) == 1
    assert lib.pcr_reduce_parts_f32(None, 2, (1 << 31) + 5, 1, 1, 1, None, None) == 1
    assert lib.pcr_ball_query_rows_ok(1024, 32, 0.0) == 1 and lib.pcr_ball_query_rows_ok(1024, 32, 0.25) == 0
    from pcr_amd import _lib
    with pytest.raises(_lib.PcrError, match="pcr_fps_f32 failed: "):
        _lib.run.pcr_fps_f32(None, None, None, 1, 8, 4, None)


def test_checked_route_calls_through_load(lib, monkeypatch):
    """`run.pcr_x` reaches the library through `_lib.load()` on every call, as `check(load().pcr_x(...))` did: the GPU tests
    that put a spy in load()'s place (tests/test_gpu_sa_xyz_tables.py) must see the package's launches"""
    from pcr_amd import _lib
    seen = []

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    with pytest.raises(_lib.PcrError, match="pcr_fps_f32 failed: "):
        _lib.run.pcr_fps_f32(None, None, None, 1, 8, 4, None)
    assert seen == ["pcr_fps_f32"]


def test_weight_packing_layout(lib):
    g = np.random.default_rng(0)
    for cout, cin in ((32, 3), (64, 67), (128, 131), (9, 256), (1, 1)):
        w = g.standard_normal((cout, cin)).astype(np.float32)
        n = lib.pcr_packed_weight_floats(cout, cin)
        cp, op = (cin + 7) // 8 * 8, (cout + 31) // 32 * 32
        assert n == cp * op
        out = np.full(n, np.nan, np.float32)
        assert lib.pcr_pack_weight_f32(w.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p)) == 0
        img = out.reshape(cp // 8, op, 2, 4)
        full = np.zeros((op, cp), np.float32)
        full[:cout, :cin] = w
        # element (kb, o, h, j) holds W[o][kb*8 + 2*j + h]
        back = img.transpose(1, 0, 3, 2).reshape(op, cp)
        assert np.array_equal(back, full)


def test_bf16_weight_image_layout_and_split(lib):
    """pcr_pack_weight_bf16x2_f32: element j of lane l (h = l // 32) of step s, cout block cb, part p holds
    W[32 cb + l % 32][16 s + kpos(h, j)], kpos = 4 h + j (j < 4) | 8 + 4 h + j - 4 (the accumulator order, pcr.h), as
    bf16 hi (p = 0) / lo (p = 1); hi + lo reproduces the weight to 2^-16 relative"""
    lib.pcr_packed_weight_bf16_floats.restype = ctypes.c_long
    g = np.random.default_rng(1)
    for cout, cin in ((32, 32), (64, 67), (130, 24), (1, 1)):
        w = g.standard_normal((cout, cin)).astype(np.float32)
        n = lib.pcr_packed_weight_bf16_floats(cout, cin)
        S, ncb = (cin + 15) // 16, (cout + 31) // 32
        assert n == S * ncb * 2 * 64 * 4
        out = np.zeros(n, np.float32)
        assert lib.pcr_pack_weight_bf16x2_f32(w.ctypes.data_as(ctypes.c_void_p), cout, cin,
                                              out.ctypes.data_as(ctypes.c_void_p)) == 0
        img = out.view(np.uint16).reshape(S, ncb, 2, 64, 8)
        as_f32 = (img.astype(np.uint32) << 16).view(np.float32)
        full = np.zeros((ncb * 32, S * 16), np.float32)
        full[:cout, :cin] = w
        # (s, cb, part, lane = 32 h + r, j) -> row 32 cb + r, column 16 s + kpos(h, j)
        a6 = as_f32.reshape(S, ncb, 2, 2, 32, 8)
        back = np.zeros((2, ncb * 32, S * 16), np.float32)
        for h in range(2):
            for j in range(8):
                col = (4 * h + j) if j < 4 else (8 + 4 * h + j - 4)
                back[:, :, col::16] = a6[:, :, :, h, :, j].transpose(2, 1, 3, 0).reshape(2, ncb * 32, S)
        hi, lo = back[0], back[1]
        assert np.all(np.abs(hi - full) <= np.abs(full) * 2.0 ** -8 + 1e-38)
        assert np.all(np.abs(hi + lo - full) <= np.abs(full) * 2.0 ** -16)
    assert lib.pcr_pack_weight_bf16x2_f32(None, 4, 4, None) == 1


def test_invalid_arguments_return_status_not_crash(lib):
    assert lib.pcr_fps_f32(None, None, None, 1, 8, 4, None) == 1
    assert lib.pcr_knn_f32(None, None, None, None, 1, 8, 4, 101, None) == 1
    assert lib.pcr_pack_weight_f32(None, 4, 4, None) == 1
    assert lib.pcr_sa_mlp_f32(None, None) == 1


def test_product_path_has_no_cpu_fallback():
    import torch
    from mmdet3d import ops
    from pcr_amd._lib import PcrError
    with pytest.raises(PcrError):
        ops.furthest_point_sample(torch.zeros(1, 8, 3), 4)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "point-cloud-reid_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert "model_oracle" not in src and "point_ops as P" not in src and "import oracle" not in src, f
                assert "pcr_oracle" not in src, f


def test_no_wide_buffer_store_with_a_register_scalar_offset(lib, tmp_path):
    """gfx950 hazard found in round 4: a 12- / 16-byte buffer store whose scalar-offset field is a REGISTER
    lets this compiler schedule a write to the store's data registers directly behind it (its hazard recogniser
    assumes the store-data hazard does not exist in that form), and the hardware then stores the overwritten value now
    and then.  No kernel of the library may contain such a store: disassemble every gfx950 code object of the built
    library and look."""
    import glob
    import re
    import shutil
    import subprocess
    from pcr_amd import _lib
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not (os.path.exists(objdump) and os.path.exists(_lib.SO_PATH)):
        pytest.skip("needs the built library and llvm-objdump")
    so = shutil.copy(_lib.SO_PATH, str(tmp_path / "lib.so"))
    subprocess.run([objdump, "--offloading", so], cwd=str(tmp_path), check=True, capture_output=True)
    objs = glob.glob(str(tmp_path / "lib.so.*gfx950"))
    assert objs, "no gfx950 code object in the library"
    wide, bad = 0, []
    pat = re.compile(r"buffer_store_dwordx[34]\s+v\[\d+:\d+\],\s*\S+,\s*s\[\d+:\d+\],\s*(\S+)")
    for o in objs:
        text = subprocess.run([objdump, "-d", o], check=True, capture_output=True, text=True).stdout
        for m in pat.finditer(text):
            wide += 1
            if re.match(r"s\d+", m.group(1)):
                bad.append(m.group(0))
    assert wide > 0                      # (the pattern still matches this toolchain's syntax)
    assert not bad, bad[:3]
