"""CPU: the validation table of include/pcr.h section A13 as tests/match_ref.py restates it, and the dicts pcr_amd/matchbook.py
derives from a table, against pcr_amd.metrics on the same rows -- float equality, NaN with NaN -- and against the values
recorded from the reference's MatchingEval (tests/golden/eval_tables.npz, eval_metric.npz).  Planted faults show that the
equality would catch a transposed table, a swapped pair, a wrong edge and a row beyond the count.  No kernel runs here:
tests/test_gpu_matchbook.py holds the launches to the same restatement."""
import ctypes
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import match_ref as R
from conftest import ROOT
from pcr_amd import matchbook as MB
from pcr_amd import metrics
from test_oracle_model import load_golden

CLS_TO_IDX = {"car": 0, "truck": 1, "bus": 2, "pedestrian": 5, "cone": 9, "nothing": 40}
NUM_CLASSES = 10


@pytest.fixture(scope="module")
def lib():
    from pcr_amd import build, _lib
    build.build()
    return _lib.load()


def same(a, b):
    """float equality with NaN equal to NaN, ints equal, dicts key for key"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(map(str, a)) == sorted(map(str, b)), (sorted(map(str, a)), sorted(map(str, b)))
        for k in a:
            same(a[k], b[k])
        return
    assert type(a) is type(b) and ((a != a and b != b) or a == b), (a, b)


def differ(a, b):
    try:
        same(a, b)
    except AssertionError:
        return True
    return False


def host_result(rows, with_classes=True):
    r = {k: torch.from_numpy(np.asarray(v)) for k, v in rows.items()}
    res = [dict(val_match_preds=r["logit"], val_match_gt=r["gt"], match_classes=r["cls"], num_points=r["num_points"],
                val_vis_gt_all=r["vis"])]
    kw = dict(cls_to_idx=CLS_TO_IDX, num_classes=NUM_CLASSES) if with_classes else {}
    return metrics.evaluate(res, **kw), metrics.evaluate_tables(res)


def rule_agrees(logit):
    """the book's decision (logit > 0) is the host route's (sigmoid(logit) > 0.5 in float32) on these logits"""
    t = torch.from_numpy(np.asarray(logit, np.float32))
    return torch.equal(metrics.decisions(t), (t > 0).float())


# ---- against the goldens -------------------------------------------------------------------------------------------------
def test_eval_tables_golden_through_the_table():
    g = load_golden("eval_tables")
    assert float(np.abs(g["logits"]).min()) >= 7.6e-4 and rule_agrees(g["logits"])
    P = len(g["logits"])
    zeros = np.zeros((P, 2), np.int64)
    got = {}
    for name, gt, col in (("points", "gt", "vis"), ("distance", "gt", "dist"), ("visibility", "gt_fp", "vis")):
        rows = dict(logit=g["logits"], gt=g[gt], cls=zeros, num_points=g["num_points"], vis=g[col])
        table, info = R.table_of(**rows)
        assert info == 0 and table[:6].sum() == P
        host = host_result(rows, with_classes=False)
        for derive in (MB, R):
            same(derive.metrics_of(table), host[0])
            same(derive.tables_of(table), host[1])
        got[name] = MB.tables_of(table)["results_per_" + name]
    for name, tables in got.items():
        flat = metrics.flatten_tables(tables)
        keys = json.loads(str(g[name + "_keys"]))
        assert sorted(flat) == keys, name
        for k, w in zip(keys, g[name + "_vals"]):
            v = float(flat[k])
            assert (v != v and w != w) or abs(v - w) < 1e-6, (name, k, v, w)


def test_eval_metric_golden_through_the_table():
    g = load_golden("eval_metric")
    assert rule_agrees(g["logits"])
    P = len(g["logits"])
    ones = np.ones((P, 2), np.int64)
    table, info = R.table_of(g["logits"], g["gt"], ones, ones, ones)
    assert info == 0
    logits, gt = torch.from_numpy(g["logits"]), torch.from_numpy(g["gt"])
    for derive in (MB, R):
        out = derive.metrics_of(table)
        assert out["val_match_acc"] == metrics.match_accuracy(logits, gt)
        assert abs(out["val_match_acc"] - float(g["val_match_acc"])) < 1e-7
        for k, v in metrics.f1_precision_recall(metrics.decisions(logits), gt).items():
            assert out[k] == v and abs(out[k] - float(g[k])) < 1e-6, k


# ---- a random case with every edge planted ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    rows = R.planted_rows(1000, seed=11, num_classes=NUM_CLASSES)
    assert rule_agrees(rows["logit"])
    assert {0, 1, 127, 128, 129} <= set(rows["num_points"].ravel().tolist())
    assert {-1, 0, 5, 10, 59} <= set(rows["vis"].ravel().tolist())
    assert (rows["cls"] >= NUM_CLASSES).any() and (rows["gt"] == -1).any()
    return rows, host_result(rows)


def test_three_batches_add_up_and_the_dicts_equal_the_host_route(planted):
    rows, host = planted
    whole, info = R.table_of(**rows)
    assert info == 0 and whole[:6].sum() == 1000
    parts = np.zeros_like(whole)
    for lo, hi in ((0, 300), (300, 301), (301, 1000)):
        t, i = R.table_of(**{k: v[lo:hi] for k, v in rows.items()})
        assert i == 0
        parts += t
    assert np.array_equal(parts, whole)
    for derive in (MB, R):
        same(derive.metrics_of(whole, CLS_TO_IDX, NUM_CLASSES), host[0])
        same(derive.tables_of(whole), host[1])
    assert "val_match_acc_FP" in host[0] and "val_match_acc_car" in host[0] and "val_match_acc_nothing" not in host[0]
    assert "val_match_acc_both_ge_65536_pts" in host[0]


def test_a_count_leaves_the_rows_beyond_it_out(planted):
    rows, _ = planted
    for count in (0, 1, 999, 1000, 5000, -3):
        n = min(max(count, 0), 1000)
        got, _ = R.table_of(count=count, **rows)
        want, _ = R.table_of(**{k: v[:n] for k, v in rows.items()})
        assert np.array_equal(got, want), count


@pytest.mark.parametrize("fault", ["swap_cells", "swap_lohi", "count", "edge_lt"])
def test_planted_faults_are_caught(planted, fault):
    rows, _ = planted
    head = {k: v[:700] for k, v in rows.items()}
    host = host_result(head)
    good, _ = R.table_of(count=700, **rows)
    same(MB.metrics_of(good, CLS_TO_IDX, NUM_CLASSES), host[0])
    same(R.tables_of(good), host[1])
    if fault == "edge_lt":
        bad_tables = R.tables_of(good, fault=fault)
        assert differ(bad_tables["results_per_distance"], host[1]["results_per_distance"])
        return
    bad, _ = R.table_of(count=700, fault=fault, **rows)
    assert not np.array_equal(bad, good)
    if fault == "swap_lohi":
        assert differ(MB.tables_of(bad)["results_per_points"], host[1]["results_per_points"])
        assert differ(MB.metrics_of(bad, CLS_TO_IDX, NUM_CLASSES), host[0])      # (the both_ge buckets)
    else:
        assert differ(MB.metrics_of(bad, CLS_TO_IDX, NUM_CLASSES), host[0])
        assert differ(MB.tables_of(bad), host[1])


# ---- flags, the reduce, the refusals ------------------------------------------------------------------------------------------
def _book_of(table, info):
    book = MB.MatchBook("cpu", num_classes=NUM_CLASSES, cls_to_idx=CLS_TO_IDX)
    book.table.copy_(torch.from_numpy(table))
    book.flags.fill_(info)
    return book


@pytest.mark.parametrize("what,bit", [("cls_high", R.INFO_CLS), ("cls_low", R.INFO_CLS), ("vis_high", R.INFO_VIS),
                                      ("vis_low", R.INFO_VIS), ("pts", R.INFO_PTS), ("nan", R.INFO_NAN), ("gt", R.INFO_GT)])
def test_rows_outside_the_rules_set_their_bit_and_metrics_raises(what, bit):
    from pcr_amd._lib import PcrError
    rows = {k: v.copy() for k, v in R.planted_rows(40, seed=3).items()}
    clean, info = R.table_of(**rows)
    assert info == 0
    plant = dict(cls_high=("cls", 63), cls_low=("cls", -2), vis_high=("vis", 63), vis_low=("vis", -2), pts=("num_points", -1),
                 nan=("logit", np.nan), gt=("gt", 0.5))[what]
    if rows[plant[0]].ndim == 2:
        rows[plant[0]][7, 1] = plant[1]
    else:
        rows[plant[0]][7] = plant[1]
    table, info = R.table_of(**rows)
    assert info == bit
    if what == "gt":
        assert table[:6].sum() == 39                       # the row contributes nothing
    else:
        assert table[:6].sum() == 40
    book = _book_of(table, info)
    assert book.info == bit and MB.info_names(info) == [what.split("_")[0]]
    with pytest.raises(PcrError, match="info = %d" % bit):
        book.metrics()
    with pytest.raises(PcrError):
        book.tables()
    assert "val_match_acc" in book.metrics(strict=False)
    same(_book_of(clean, 0).metrics(), MB.metrics_of(clean, CLS_TO_IDX, NUM_CLASSES))


def test_objects_rule_ties_nans_and_period():
    logits = np.asarray([[1, 3, 3, 0], [2, 2, 2, 2], [0, np.nan, 5, np.nan], [-1, -2, -3, -0.5]], np.float32)
    want = torch.from_numpy(logits).argmax(dim=1).tolist()
    assert want[:2] == [1, 0] and want[3] == 3
    got, info = R.objects_of(cls_logits=logits, cls_gt=np.asarray(want))
    assert got.tolist() == [4, 4, 0, 0] and info == R.INFO_NAN
    got, info = R.objects_of(cls_logits=logits, cls_gt=np.asarray([2, 1, 1, 3]), fp_logits=np.asarray([1, -1, 0, 2.0]),
                             fp_gt=np.asarray([1, 0, 0, 0.0]), count=1, period=2)
    assert got.tolist() == [1, 2, 2, 2]                    # objects 0 and 2 take part; object 2 is right (first NaN)
    table = np.zeros(MB.TABLE, np.int64)
    table[MB.OBJ:] = [3, 4, 1, 3]
    out = MB.metrics_of(table)
    assert out["val_cls_acc"] == 0.75 and out["val_fp_acc"] == float(np.float32(1) / np.float32(3))
    same({k: out[k] for k in ("val_cls_acc", "val_fp_acc")}, {k: R.metrics_of(table)[k] for k in ("val_cls_acc", "val_fp_acc")})
    # the host route's own two lines on the same objects
    r = dict(val_cls_preds=torch.from_numpy(logits), val_cls_gt=torch.tensor(want),
             val_fp_preds=torch.tensor([1, -1, 0, 2.0]), val_fp_gt=torch.tensor([1, 0, 0, 0.0]))
    full, _ = R.objects_of(cls_logits=logits, cls_gt=np.asarray(want), fp_logits=np.asarray([1, -1, 0, 2.0]),
                           fp_gt=np.asarray([1, 0, 0, 0.0]))
    table[MB.OBJ:] = full
    host = metrics.object_head_accuracy(r)
    assert MB.metrics_of(table)["val_cls_acc"] == host["val_cls_acc"] and MB.metrics_of(table)["val_fp_acc"] == host["val_fp_acc"]


def test_counts_beyond_float32_are_derived_in_float64():
    table = np.zeros(MB.TABLE, np.int64)
    table[:6] = [1, (1 << 24) + 1, 3, 5, 0, 0]
    out = MB.metrics_of(table)
    assert out["counts_beyond_f32"] is True
    assert out["val_match_acc"] == ((1 << 24) + 4) / ((1 << 24) + 10)
    table[1] = 100
    assert "counts_beyond_f32" not in MB.metrics_of(table)


WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, os.path.join(%(root)r, "point-cloud-reid_amd"))
    sys.path.insert(0, os.path.join(%(root)r, "tests"))
    import numpy as np, torch, torch.distributed as dist
    import match_ref as R
    from pcr_amd import matchbook as MB, shard
    rank, local, world = shard.init(backend="gloo")
    assert world == 2 and shard.is_dist()
    rows = R.planted_rows(200, seed=5)
    rows["vis"][150, 0] = 63                                    # rank 1's half holds a row outside the range
    lo, hi = shard.shard_range(200, rank, world)
    table, info = R.table_of(**{k: v[lo:hi] for k, v in rows.items()})
    assert info == (0 if rank == 0 else R.INFO_VIS)
    book = MB.MatchBook("cpu")
    book.table.copy_(torch.from_numpy(table)); book.flags.fill_(info)
    book.reduce()
    whole, winfo = R.table_of(**rows)
    assert np.array_equal(book.table.numpy(), whole) and book.info == winfo == R.INFO_VIS
    dist.barrier()
    dist.destroy_process_group()
    sys.stdout.write("rank %%d ok\\n" %% rank); sys.stdout.flush()
""")


def test_two_rank_gloo_reduce_of_two_half_tables_is_the_whole_table(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % dict(root=ROOT))
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rank 0 ok" in r.stdout and "rank 1 ok" in r.stdout


def test_add_refuses_what_the_kernel_cannot_read(lib):
    from pcr_amd._lib import PcrError
    book = MB.MatchBook("cpu")
    rows = {k: torch.from_numpy(v) for k, v in R.planted_rows(8, seed=1).items()}
    bad = [("logit", rows["logit"].double(), "logit must be a torch.float32"),
           ("gt", rows["gt"].long(), "gt must be a torch.float32"),
           ("gt", rows["gt"][:7], "gt must be"),
           ("cls", rows["cls"].float(), "cls must be a torch.int32"),
           ("num_points", rows["num_points"][:, :1], "num_points must be"),
           ("vis", rows["vis"].reshape(4, 4), "vis must be"),
           ("logit", rows["logit"].reshape(8, 1), "logit must be")]
    for key, value, msg in bad:
        with pytest.raises(PcrError, match=msg):
            book.add(**dict(rows, **{key: value}))
    with pytest.raises(PcrError, match="count must"):
        book.add(count=torch.zeros(2, dtype=torch.int32), **rows)
    with pytest.raises(PcrError, match="no CPU"):          # host tensors: the last refusal, after everything else fits
        book.add(**rows)
    with pytest.raises(PcrError, match="no CPU"):
        book.add(dict(val_match_preds=rows["logit"], val_match_gt=rows["gt"], match_classes=rows["cls"],
                      num_points=rows["num_points"], val_vis_gt_all=rows["vis"].unsqueeze(2)))
    with pytest.raises(PcrError, match="has no 'num_points'"):
        book.add(dict(val_match_preds=rows["logit"], val_match_gt=rows["gt"], match_classes=rows["cls"],
                      val_vis_gt_all=rows["vis"]))
    with pytest.raises(PcrError, match="add needs"):
        book.add(logit=rows["logit"], gt=rows["gt"])
    with pytest.raises(PcrError, match="come together"):
        book.add_objects(cls_logits=torch.zeros(4, 3))
    with pytest.raises(PcrError, match="no CPU"):
        book.add_objects(fp_logits=torch.zeros(4), fp_gt=torch.zeros(4))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_symbols_status_and_table_constants(lib):
    from pcr_amd import abi
    for name in ("pcr_match_ok", "pcr_match_record_i64", "pcr_match_record_objects_i64"):
        assert hasattr(lib, name) and name in abi.SIGNATURES
    assert lib.pcr_match_ok(0, 0, 1) == 1 and lib.pcr_match_ok(1 << 30, 1 << 30, 4096) == 1
    assert lib.pcr_match_ok(-1, 0, 1) == 0 and lib.pcr_match_ok(0, 0, 0) == 0 and lib.pcr_match_ok(0, 0, 4097) == 0
    assert lib.pcr_match_record_i64(None, None) == 1
    assert lib.pcr_match_record_i64(ctypes.byref(abi.MatchParams()), None) == 1            # no table
    assert lib.pcr_match_record_objects_i64(None, None, None, None, None, None, None, 4, 3, 4, None) == 1
    text = open(os.path.join(ROOT, "include", "pcr.h")).read()
    import re
    consts = {k: int(v) for k, v in re.findall(r"#define PCR_MATCH_(\w+) (\d+)", text)}
    for mod in (MB, R):
        assert (mod.ALL, mod.CLS0, mod.CLSMAX, mod.PTS, mod.VIS, mod.OBJ, mod.TABLE, mod.CELLS, mod.KEY_BINS, mod.PTS_BINS) == \
            tuple(consts[k] for k in ("ALL", "CLS0", "CLSMAX", "PTS", "VIS", "OBJ", "TABLE", "CELLS", "KEY_BINS", "PTS_BINS"))
    assert MB.INFO == {k.lower(): consts["INFO_" + k] for k in ("NAN", "GT", "CLS", "PTS", "VIS")}
    assert MB.OBJECTS == {k.lower(): consts[k] for k in ("CLS_CORRECT", "CLS_TOTAL", "FP_CORRECT", "FP_TOTAL")}


def test_parameter_block_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of pcr_match as the host compiler lays the header out against the ctypes mirror"""
    from pcr_amd import abi, build
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    clang = next(c for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "llvm", "bin", "clang"))
                 if os.path.exists(c))
    ct = abi.MatchParams
    names = [n for n, _ in ct._fields_]
    assert names == ["P", "logit", "gt", "cls", "num_points", "vis", "count", "table", "info"]
    assert ct.ELEM == dict(logit=torch.float32, gt=torch.float32, cls=torch.int32, num_points=torch.int32, vis=torch.int32,
                           count=torch.int32, table=torch.int64, info=torch.int32)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pcr.h"', 'int main(void) {',
             '  printf(". %zu 0\\n", sizeof(pcr_match));']
    for f in names:
        lines.append('  printf("%s %%zu %%zu\\n", offsetof(pcr_match, %s), sizeof(((pcr_match *)0)->%s));' % (f, f, f))
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


def test_run_epochs_calls_on_epoch_after_each_epoch():
    from pcr_amd import loader as LD

    class Trainer:
        epoch = 0

        def step(self, batch):
            return dict(loss=torch.tensor(float(batch)))

    class Loader:
        def epoch(self, ep):
            return [ep, ep + 0.5]
    seen = []
    outs = LD.run_epochs(Trainer(), Loader(), 2, start_epoch=3, on_epoch=lambda ep, tr: seen.append((ep, tr.epoch)))
    assert seen == [(3, 4), (4, 5)] and len(outs) == 4
    assert len(LD.run_epochs(Trainer(), Loader(), 1)) == 2
