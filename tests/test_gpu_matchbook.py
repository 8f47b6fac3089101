"""GPU: the validation book (include/pcr.h section A13, csrc/match_kernels.hip, pcr_amd/matchbook.py) -- the record launches
bit for bit against tests/match_ref.py at the sizes where they can go wrong (one row, a wave more or less, several
workgroups, the strided grid, every row in one bin, the largest point count), a device-side count, accumulation, the
object heads' ties, a captured validate_step replayed over three batches, and evaluate_model(book=) against the host route
on the toy crop directory of tests/test_gpu_evaluate.py."""
import os

import numpy as np
import pytest
import torch

import match_ref as R
from pcr_amd import evaluate as EV
from pcr_amd import matchbook as MB
from pcr_amd._lib import PcrError
from test_matchbook_cpu import same

pytestmark = pytest.mark.gpu
DEV = "cuda"
COLS = ("logit", "gt", "cls", "num_points", "vis")


def dev(rows, narrow=True):
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in rows.items()}
    if narrow:
        for k in ("cls", "num_points", "vis"):
            out[k] = out[k].to(torch.int32)
    return out


def dev_count(c):
    return None if c is None else torch.tensor([c], dtype=torch.int32, device=DEV)


def launch(rows, count=None, book=None):
    """one record launch -> (table, info) on the host"""
    book = MB.MatchBook(DEV) if book is None else book
    book.add(count=dev_count(count), **dev(rows))
    return book.table.cpu().numpy(), book.info


@pytest.fixture(scope="module")
def planted():
    return R.planted_rows(1000, seed=11)


def head(rows, n):
    return {k: v[:n] for k, v in rows.items()}


# ---- 1. the record launch against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 1000])
def test_record_equals_the_restatement_with_and_without_a_count(planted, P):
    rows = head(planted, P)
    for count in (0, 1, P - 1, None):
        got, info = launch(rows, count)
        want, winfo = R.table_of(count=count, **rows)
        assert np.array_equal(got, want) and info == winfo == 0, (P, count)
        assert got[:6].sum() == (P if count is None else count)
    got, _ = launch(rows, P + 7)                              # a count beyond the batch is the batch
    assert np.array_equal(got, R.table_of(**rows)[0])
    got, _ = launch(rows, -2)
    assert not got.any()


def test_every_row_in_one_bin(planted):
    one = {k: np.repeat(v[3:4], 1000, axis=0) for k, v in planted.items()}
    got, info = launch(one)
    want, _ = R.table_of(**one)
    assert np.array_equal(got, want) and info == 0
    assert sorted(got[got != 0].tolist()) == [1000] * 5      # ALL, CLS0, CLSMAX, PTS, VIS: one counter each


def test_the_strided_grid(planted):
    """more rows than the capped grid holds at once: 300 copies of the planted rows"""
    many = {k: np.concatenate([v] * 300, axis=0) for k, v in planted.items()}
    got, info = launch(many)
    assert np.array_equal(got, 300 * R.table_of(**planted)[0]) and info == 0
    got, _ = launch(many, 299001)
    assert np.array_equal(got, 299 * R.table_of(**planted)[0] + R.table_of(**head(planted, 1))[0])


def test_the_largest_point_counts():
    rows = R.planted_rows(64, seed=2)
    top = 2 ** 31 - 1
    rows["num_points"][0] = (top, top)
    rows["num_points"][1] = (top, 0)
    rows["num_points"][2] = (1, top)
    rows["num_points"][3] = (2 ** 30, 2 ** 30 - 1)
    got, info = launch(rows)
    want, _ = R.table_of(**rows)
    assert np.array_equal(got, want) and info == 0
    pts = got[MB.PTS:MB.VIS].reshape(32, 32, 6)
    assert pts[31, 31].sum() >= 1 and pts[0, 31].sum() >= 1 and pts[1, 31].sum() >= 1 and pts[30, 31].sum() >= 1
    t = MB.tables_of(got)["results_per_points"]               # the top bin is the reference's last edge: 30 buckets
    assert max(k[1] for k in t["at_least_one"]) == 30


@pytest.mark.parametrize("column,value,bit", [("cls", 63, "cls"), ("cls", -2, "cls"), ("vis", 63, "vis"), ("vis", -2, "vis"),
                                              ("num_points", -1, "pts"), ("logit", np.nan, "nan"), ("gt", 0.5, "gt")])
def test_rows_outside_the_rules_set_their_bit(column, value, bit):
    rows = R.planted_rows(130, seed=4)
    if rows[column].ndim == 2:
        rows[column][129, 0] = value
    else:
        rows[column][129] = value
    book = MB.MatchBook(DEV)
    got, info = launch(rows, book=book)
    want, winfo = R.table_of(**rows)
    assert np.array_equal(got, want) and info == winfo == MB.INFO[bit]
    with pytest.raises(PcrError, match="info = %d" % MB.INFO[bit]):
        book.metrics()
    assert book.metrics(strict=False)["val_match_acc"] == MB.metrics_of(want)["val_match_acc"]
    got, info = launch(rows, 129)                             # beyond the count the row is not even read
    assert info == 0 and np.array_equal(got, R.table_of(**head(rows, 129))[0])


# ---- 2. the book -------------------------------------------------------------------------------------------------------------
def test_three_adds_equal_one_and_reset_empties(planted):
    book = MB.MatchBook(DEV, num_classes=10, cls_to_idx={"car": 0, "bus": 2})
    for lo, hi in ((0, 300), (300, 301), (301, 1000)):
        book.add(**dev({k: v[lo:hi] for k, v in planted.items()}, narrow=False))       # int64 columns, as forward_test's
    whole, _ = R.table_of(**planted)
    assert np.array_equal(book.table.cpu().numpy(), whole) and book.info == 0 and book.num_pairs == 1000
    same(book.metrics(), R.metrics_of(whole, {"car": 0, "bus": 2}, 10))
    same(book.tables(), R.tables_of(whole))
    m, t = book.results()
    same(m, book.metrics()), same(t, book.tables())
    book.reset()
    assert not book.table.any() and book.info == 0
    d = dev(planted, narrow=False)                           # the dict form, the visibility column as (P, 2, 1)
    book.add(dict(val_match_preds=d["logit"], val_match_gt=d["gt"], match_classes=d["cls"], num_points=d["num_points"],
                  val_vis_gt_all=d["vis"].unsqueeze(2), val_cls_preds=None))
    assert np.array_equal(book.table.cpu().numpy(), whole)
    book.reduce()                                             # one rank: nothing to do
    assert np.array_equal(book.table.cpu().numpy(), whole)


def test_two_runs_give_the_same_table(planted):
    many = {k: np.concatenate([v] * 8, axis=0) for k, v in planted.items()}
    a, _ = launch(many)
    b, _ = launch(many)
    assert np.array_equal(a, b) and a[:6].sum() == 8000


def test_objects_ties_go_to_the_lowest_index():
    g = np.random.default_rng(6)
    M, C = 300, 7
    logits = g.integers(-2, 3, size=(M, C)).astype(np.float32)          # few distinct values: most rows hold a tie
    assert (np.sort(logits, axis=1)[:, -1] == np.sort(logits, axis=1)[:, -2]).sum() > 100
    arg = torch.from_numpy(logits).argmax(dim=1).numpy()
    cls_gt = np.where(g.random(M) < 0.5, arg, (arg + 1) % C)
    fp_logits = g.standard_normal(M).astype(np.float32)
    fp_logits[:5] = 0.0
    fp_gt = (g.random(M) < 0.5).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)                              # noqa: E731
    for count, period in ((None, None), (100, 150), (0, 150), (150, 150), (7, 300)):
        book = MB.MatchBook(DEV)
        book.add_objects(cls_logits=t(logits), cls_gt=t(cls_gt), fp_logits=t(fp_logits), fp_gt=t(fp_gt), count=dev_count(count),
                         period=period)
        want, winfo = R.objects_of(logits, cls_gt, fp_logits, fp_gt, count=count, period=period)
        got = book.table.cpu().numpy()
        assert np.array_equal(got[MB.OBJ:], want) and book.info == winfo == 0, (count, period)
        assert not got[:MB.OBJ].any()
    assert want[1] == want[3] == 7                            # (count 7 of a flat list of 300)
    # the host route's two lines on all objects
    from pcr_amd import metrics
    book = MB.MatchBook(DEV)
    book.add_objects(cls_logits=t(logits), cls_gt=t(cls_gt))
    book.add_objects(fp_logits=t(fp_logits), fp_gt=t(fp_gt))
    host = metrics.object_head_accuracy(dict(val_cls_preds=torch.from_numpy(logits), val_cls_gt=torch.from_numpy(cls_gt),
                                             val_fp_preds=torch.from_numpy(fp_logits), val_fp_gt=torch.from_numpy(fp_gt)))
    out = book.metrics()
    assert out["val_cls_acc"] == host["val_cls_acc"] and out["val_fp_acc"] == host["val_fp_acc"]
    nan = logits.copy()
    nan[4, 2] = nan[4, 5] = np.nan
    book.reset()
    book.add_objects(cls_logits=t(nan), cls_gt=t(cls_gt))
    want, winfo = R.objects_of(nan, cls_gt)
    assert np.array_equal(book.table.cpu().numpy()[MB.OBJ:], want) and book.info == winfo == MB.INFO["nan"]


# ---- 3. the validation step -----------------------------------------------------------------------------------------------
N = 128


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """the toy crop directory of tests/test_gpu_evaluate.py, its validation set, a CropStore over it and the toy
    Point-Transformer; the head's bias is moved into the widest gap near the median logit so that both decisions occur"""
    import bench
    from pcr_amd.store import CropStore
    from test_evaluate import VAL_CFG, write_toy_crops
    crops = str(tmp_path_factory.mktemp("book") / "crops")
    os.makedirs(crops)
    write_toy_crops(crops)
    val = dict(VAL_CFG, subsample_sparse=N)
    ds, table = EV.build_val_set(val, crops)
    store = CropStore.from_directory(crops, table, device=DEV, pair_rule=False)
    model, _ = bench.build_pt_model([N, 64, 32])
    kw = dict(rank=0, world=1, cls_to_idx=val["cls_to_idx"], num_classes=table.num_classes, store=store)
    srt = torch.sort(EV.evaluate_model(model, ds, 16, seed=5, **kw)["logits"]).values
    lo = len(srt) // 2 - 10
    j = int((srt[lo + 1:lo + 21] - srt[lo:lo + 20]).argmax())
    with torch.no_grad():
        model.match_head[1].bias.sub_(0.5 * float(srt[lo + j] + srt[lo + j + 1]))
    return model, ds, store, kw, crops


def static_batch(batch):
    """one tensor per key with the batch's samples as views: what a captured step reads"""
    held = {k: torch.stack(v).clone() for k, v in batch.items()}
    return held, {k: list(t.unbind(0)) for k, t in held.items()}


def test_a_captured_validate_step_replayed_over_three_batches(toy):
    model, ds, store, kw, _ = toy
    B, seed = 8, 5
    spans = ((0, B), (B, 2 * B), (2 * B, 2 * B + 5))
    batches = [store.val_batch(lo, hi, seed, n=N) for lo, hi in spans]
    eager = MB.MatchBook(DEV)
    with torch.no_grad():
        for b in batches:
            model.validate_step(b, eager)                    # (also the warm-up: nothing is loaded inside the capture)
        torch.cuda.synchronize()
        assert eager.info == 0 and eager.num_pairs == 2 * B + 5
        book, count = MB.MatchBook(DEV), dev_count(B)
        held, views = static_batch(batches[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                        # a device-to-host copy in here would fail the capture
            assert model.validate_step(views, book, count) is None
        assert not book.table.any()
        for (lo, hi), b in zip(spans, batches):
            b = EV._padded(b, B)
            for k, t in held.items():
                t.copy_(torch.stack(b[k]))
            count.fill_(hi - lo)
            graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(book.table, eager.table) and book.info == 0
    same(book.metrics(), eager.metrics())


def test_evaluate_model_with_a_book_equals_the_host_route(toy):
    model, ds, store, kw, _ = toy
    bs = 16
    assert len(ds) % bs != 0 and len(ds) > bs                 # the last batch is padded and carries a count
    host = None
    for seed in (5, 6, 7, 8):                                 # a logit in (0, 1e-6] is where the two decision rules part
        host = EV.evaluate_model(model, ds, bs, seed=seed, **kw)
        x = host["logits"]
        if not bool(((x > 0) & (x <= 1e-6)).any()):
            break
    else:
        raise AssertionError("every seed puts a logit into (0, 1e-6]")
    assert {"logits", "targets", "tables", "num_pairs", "world", "val_match_acc", "val_match_acc_car"} <= set(host)
    assert 0.2 < float((host["logits"] > 0).float().mean()) < 0.8
    book = MB.MatchBook(DEV)
    seen = []
    got = EV.evaluate_model(model, ds, bs, seed=seed, book=book, on_batch=lambda b0, batch, res: seen.append((b0, res)), **kw)
    assert seen == [(b0, None) for b0 in range(0, len(ds), bs)]
    assert set(got) == set(host) - {"logits", "targets"}
    assert got["num_pairs"] == host["num_pairs"] == len(ds) == book.num_pairs
    for k in got:
        same(got[k], host[k])
    assert {"results_per_points", "results_per_distance", "results_per_visibility"} == set(got["tables"])
    # keep_logits: forward_test's route feeding the same book
    kept = EV.evaluate_model(model, ds, bs, seed=seed, book=book, keep_logits=True, **kw)
    assert torch.equal(kept["logits"], host["logits"]) and torch.equal(kept["targets"], host["targets"])
    assert set(kept) == set(host)
    for k in got:
        same(kept[k], host[k])
    # a book with one batch size equals a book with another; without book= the call is what it was
    other = EV.evaluate_model(model, ds, 24, seed=seed, book=MB.MatchBook(DEV), **kw)
    same(other["tables"], got["tables"])
    again = EV.evaluate_model(model, ds, bs, seed=seed, **kw)
    assert torch.equal(again["logits"], host["logits"]) and set(again) == set(host)
    with pytest.raises(ValueError):
        EV.evaluate_model(model, ds, bs, seed=seed, keep_logits=True, **kw)


def test_evaluate_checkpoint_passes_a_device_book_through(toy, tmp_path):
    from conftest import ROOT
    from pcr_amd import testing as T
    from test_evaluate import VAL_CFG
    from test_gpu_evaluate import CONFIG, DATA
    crops = toy[4]
    (tmp_path / "data.py").write_text(DATA % (dict(VAL_CFG, subsample_sparse=N),))
    (tmp_path / "exp.py").write_text(CONFIG)
    sd = T.seeded_state_dict(T.load_manifest(os.path.join(ROOT, "tests", "golden", "pt_manifest.json")), 0)
    ckpt = str(tmp_path / "epoch_1.pth")
    torch.save({"meta": {"epoch": 1}, "state_dict": sd}, ckpt)
    run = lambda **k: EV.evaluate_checkpoint(str(tmp_path / "exp.py"), ckpt, crops, device_store=True, **k)     # noqa: E731
    a, b = run(), run(device_book=True)
    assert "logits" in a and "logits" not in b and a["num_pairs"] == b["num_pairs"] and b["checkpoint_meta"] == {"epoch": 1}
    assert not bool(((a["logits"] > 0) & (a["logits"] <= 1e-6)).any())      # (the two decision rules are one here)
    for k in b:
        same(b[k], a[k])
