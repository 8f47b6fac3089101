"""CPU: the section-A11 entry points (the updater as configured, the scene log) exist, keep the ABI number, have the
ranges the header states and refuse what they must without a launch; `UpdateRules` and `ReIDNet.track_step` refuse the
combinations of arguments that have no meaning."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("pcr_bank_rules_ok", "pcr_bank_plan_rules_i32", "pcr_scene_log_ok", "pcr_scene_log_append_i32")
INVALID = 1
CONFIG = dict(match=dict(output=True, active=True, decom=False), det_newborn=dict(output=True, active=True, decom=False),
              det_false_positive=dict(output=False, active=False, decom=True),
              track_false_positive=dict(output=False, active=False, decom=True),
              track_false_negative=dict(output=True, active=True, decom=False))


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def header_int(name):
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_new_symbols_are_exported_declared_and_abi_is_17(lib):
    from pcr_amd import abi
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libpcr_hip.so does not export %s" % s
        assert re.search(r"\b%s\s*\(" % s, header), "include/pcr.h does not declare %s" % s
        assert s in abi.SIGNATURES
    assert lib.pcr_abi_version() == 17
    for name, value in (("PCR_RULE_OUTPUT", 1), ("PCR_RULE_ACTIVE", 2), ("PCR_RULE_DECOM", 4), ("PCR_TRK_KEEP", 0),
                        ("PCR_TRK_MISS", 1)):
        assert header_int(name) == value


def test_blocks_match_the_header_layout(tmp_path):
    """the two blocks are tagged structs (as A10's), which tests/test_abi.py's layout probe does not see: the same probe
    here, sizeof / offsetof of every field as the host compiler lays the header out against the ctypes mirrors"""
    import subprocess
    from pcr_amd import abi
    from test_abi import _host_clang, header_text
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pcr.h"', 'int main(void) {']
    blocks = {"pcr_bank_rules": abi.BankRulesParams, "pcr_scene_log": abi.SceneLogParams}
    for s, ct in blocks.items():
        body = re.search(r"struct %s \{(.*?)\};" % s, header_text(), flags=re.S).group(1)
        names = [m.group(1) for d in body.replace(";", ",").split(",") for m in [re.search(r"(\w+)\s*(?:\[\d+\])?\s*$", d)] if m]
        assert names == [n for n, _ in ct._fields_], (s, names)
        lines.append('  printf("%s . %%zu 0\\n", sizeof(%s));' % (s, s))
        for f in names:
            lines.append('  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, f, s, f, s, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.run([_host_clang(), "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    compared = 0
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, off, size = line.split()
        ct = blocks[s]
        if f == ".":
            assert ctypes.sizeof(ct) == int(off), (s, ctypes.sizeof(ct), off)
            continue
        d = getattr(ct, f)
        assert (d.offset, d.size) == (int(off), int(size)), (s, f, d.offset, d.size, off, size)
        compared += 1
    assert compared == len(abi.BankRulesParams._fields_) + len(abi.SceneLogParams._fields_)


def test_ok_ranges(lib):
    top, dec, rows = header_int("PCR_ASSOC_MAX_OBJECTS"), header_int("PCR_ASSOC_MAX_DECISIONS"), header_int("PCR_LOG_MAX_ROWS")
    ok = lib.pcr_bank_rules_ok
    assert ok(1, 0, 9, 0, 0) == 1 and ok(top, top, 7, dec, dec) == 1 and ok(40, 30, 9, 2, 1) == 1
    assert ok(0, 4, 9, 2, 1) == 0 and ok(top + 1, 4, 9, 2, 1) == 0 and ok(4, -1, 9, 2, 1) == 0 and ok(4, top + 1, 9, 2, 1) == 0
    for W in (-1, 0, 6, 8, 10):
        assert ok(4, 4, W, 2, 1) == 0
    for n in (-1, dec + 1):
        assert ok(4, 4, 9, n, 1) == 0 and ok(4, 4, 9, 1, n) == 0
    ok = lib.pcr_scene_log_ok
    assert ok(1, 1, 7) == 1 and ok(rows, 2 * top, 9) == 1 and ok(5000, 70, 9) == 1
    assert ok(0, 4, 9) == 0 and ok(rows + 1, 4, 9) == 0 and ok(8, 0, 9) == 0 and ok(8, 2 * top + 1, 9) == 0 and ok(8, 4, 8) == 0


def _rules_block(C=4, D=3, dd=2, td=2):
    """a block whose pointers are all non-NULL host addresses: a call that is refused must not come as far as a launch"""
    from pcr_amd import abi
    p = abi.BankRulesParams()
    p.C, p.D, p.W, p.dd, p.td, p.frame_limit = C, D, 9, dd, td, 3
    p.match_rule = 3
    for i in range(4):
        p.det_rule[i], p.trk_rule[i], p.trk_kind[i] = 3, 3, i % 2
    keep = (ctypes.c_int * 64)()
    for name, _ in abi.BankRulesParams._fields_:
        if name in abi.BankRulesParams.ELEM:
            setattr(p, name, ctypes.addressof(keep))
    return p, keep


def test_plan_rules_refuses_invalid_arguments_without_a_launch(lib):
    from pcr_amd import abi
    call = lambda p: lib.pcr_bank_plan_rules_i32(ctypes.byref(p), None)
    assert lib.pcr_bank_plan_rules_i32(None, None) == INVALID
    assert call(abi.BankRulesParams()) == INVALID                                 # all NULL, C == 0
    for name in abi.BankRulesParams.ELEM:
        if name == "carry":
            continue                                                              # (NULL = identity)
        p, keep = _rules_block()
        setattr(p, name, None)
        assert call(p) == INVALID, name
    for field, value in (("dd", 5), ("td", 5), ("dd", -1), ("frame_limit", 0), ("W", 8), ("C", 0), ("match_rule", 6),
                         ("match_rule", 8)):
        p, keep = _rules_block()
        setattr(p, field, value)
        assert call(p) == INVALID, (field, value)
    for field, i in (("det_rule", 0), ("det_rule", 1), ("trk_rule", 1)):
        p, keep = _rules_block()
        getattr(p, field)[i] = 2 | 4                                               # ACTIVE | DECOM
        assert call(p) == INVALID, (field, i)
    p, keep = _rules_block()
    p.trk_kind[1] = 2
    assert call(p) == INVALID


def test_log_append_refuses_invalid_arguments_without_a_launch(lib):
    from pcr_amd import abi
    call = lambda p: lib.pcr_scene_log_append_i32(ctypes.byref(p), None)
    assert lib.pcr_scene_log_append_i32(None, None) == INVALID
    keep = (ctypes.c_int * 64)()

    def block():
        p = abi.SceneLogParams()
        p.rows_max, p.R, p.W = 8, 4, 9
        for name in abi.SceneLogParams.ELEM:
            setattr(p, name, ctypes.addressof(keep))
        return p
    for name in abi.SceneLogParams.ELEM:
        p = block()
        setattr(p, name, None)
        assert call(p) == INVALID, name
    for field, value in (("rows_max", 0), ("R", 0), ("W", 5)):
        p = block()
        setattr(p, field, value)
        assert call(p) == INVALID, (field, value)


def test_update_rules_maps_names_and_refuses(lib):
    from pcr_amd import tracks as T
    from pcr_amd._lib import PcrError
    r = T.UpdateRules(CONFIG, ["det_false_positive", "det_newborn"], ["track_false_negative", "track_false_positive"])
    assert r.match_rule == 3 and r.det_rule == (4, 3) and r.trk_rule == (3, 4)
    assert r.trk_kind == (T.TRK_MISS, T.TRK_KEEP)
    r = T.UpdateRules(CONFIG, ["det_newborn"], [])
    assert r.det_rule == (3,) and r.trk_rule == () and r.trk_kind == ()
    with pytest.raises(PcrError, match="no entry for 'det_newborn'"):
        T.UpdateRules({k: v for k, v in CONFIG.items() if k != "det_newborn"}, ["det_newborn"], [])
    with pytest.raises(PcrError, match="no entry for 'match'"):
        T.UpdateRules({k: v for k, v in CONFIG.items() if k != "match"}, ["det_newborn"], [])
    with pytest.raises(PcrError, match="no entry for 'det_d0'"):
        T.UpdateRules(CONFIG, ["det_d0"], [])
    with pytest.raises(PcrError, match="unknown key 'track_unmatched'"):
        T.UpdateRules(dict(CONFIG, track_unmatched=CONFIG["match"]), ["det_newborn"], [])
    with pytest.raises(PcrError, match="dict\\(output=, active=, decom=\\)"):
        T.UpdateRules(dict(CONFIG, match=dict(output=True, active=True)), ["det_newborn"], [])
    with pytest.raises(PcrError, match="both active and decom"):
        T.UpdateRules(dict(CONFIG, det_false_positive=dict(output=False, active=True, decom=True)), ["det_newborn"], [])


def test_track_step_refuses_meaningless_combinations():
    """the refusals come before anything touches a device: a bank that is no bank is never looked at"""
    from mmdet3d.models.ReIDNet import ReIDNet
    from pcr_amd import tracks as T
    from pcr_amd._lib import PcrError
    bank = T.TrackBank.__new__(T.TrackBank)
    bank.capacity, bank.max_dets, bank.box_width = 8, 4, 9
    step = lambda **kw: ReIDNet.track_step(None, bank, None, None, None, None, **kw)
    decisions = dict(detection=("det_newborn",), tracking=())
    with pytest.raises(PcrError, match="pass decisions= with it"):
        step(update_config=CONFIG)
    for extra in (dict(propagate=False), dict(force_truth=True, truth=None)):
        with pytest.raises(PcrError):
            step(update_config=CONFIG, decisions=decisions, **extra)
    with pytest.raises(PcrError, match="born / kill"):
        step(update_config=CONFIG, decisions=decisions, born=object())
    with pytest.raises(PcrError, match="born= / kill=, propagate= or force_truth="):
        step(update_config=CONFIG, decisions=decisions, propagate=False)
    with pytest.raises(PcrError, match="pass update_config= with it"):
        step(log=object())
    with pytest.raises(PcrError, match="SceneLog of 12 rows per frame"):
        step(update_config=CONFIG, decisions=decisions, log=object())
