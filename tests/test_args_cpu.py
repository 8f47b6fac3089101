"""CPU: the tracker-side wrappers refuse a bad argument in one way (pcr_amd/_lib.py `tensor` / `out_tensor`, pcr_amd/abi.py
`fill`): always a PcrError that names the entry and the argument, what is wrong with the call before where a tensor lives --
so every refusal but the last is met here on host tensors -- and never an `assert`, which python -O would drop."""
import ast
import os
import re

import pytest
import torch

from conftest import ROOT

from pcr_amd import abi
from pcr_amd._lib import PcrError, out_tensor, tensor

MODULES = ("associate", "tracks", "truth", "identity", "retrieval", "nms", "crops", "store")
C, D, G, T, Q, K = 4, 3, 2, 3, 2, 1                       # the smallest sizes that tell every field's count apart

i32 = lambda *s: torch.zeros(s, dtype=torch.int32)        # noqa: E731
f32 = lambda *s: torch.zeros(s, dtype=torch.float32)      # noqa: E731
f64 = lambda *s: torch.zeros(s, dtype=torch.float64)      # noqa: E731
i64 = lambda *s: torch.zeros(s, dtype=torch.int64)        # noqa: E731


def strided(t):
    """the same shape, dtype and values, every second element of a buffer twice as long in the last dimension"""
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)
    v = wide[..., ::2]
    assert v.shape == t.shape and (not v.is_contiguous() or v.numel() <= 1)
    return v


def refused(call, pattern):
    with pytest.raises(PcrError, match=pattern):
        call()


# ---- the filler on a real block: pcr_ident_close holds all four typed kinds ------------------------------------------------
ROWS, IDS, MR, MC = 4, 3, 2, 3
CLOSE_SIZES = dict(cooc=ROWS * IDS, gt_track=ROWS * 8, totals=8, dist_sum=1, flags=ROWS + IDS, counts=4, row_list=MR,
                   col_list=MC, cost=MR * MC, col4row=MR, info=1, id_map=ROWS, table=16, dist_total=1)


def close_tensors():
    return dict(cooc=i32(ROWS, IDS), gt_track=i32(ROWS, 8), totals=i32(8), dist_sum=f64(1), flags=i32(ROWS + IDS),
                counts=i32(4), row_list=i32(MR), col_list=i32(MC), cost=f32(MR, MC), col4row=i32(MR), info=i32(1),
                id_map=i32(ROWS), table=i64(16), dist_total=f64(1))


def close_fill(required=(), sizes=CLOSE_SIZES, **changed):
    return abi.fill(abi.IdentCloseParams(), dict(close_tensors(), **changed), sizes, required=required, who="here")


# (the filler's step, a change to a right call, the refusal), in the order of the steps
FILL_REFUSALS = (
    (1, dict(bogus=i32(1)), r"^here: unknown tensor 'bogus'"),
    (1, dict(gt_rows=i32(1)), r"^here: unknown tensor 'gt_rows'"),                   # a scalar field is no pointer field
    (2, dict(cooc=[0] * 12), r"^here: cooc must be a tensor"),
    (3, dict(flags=None), r"^here: flags is missing"),
    (4, dict(cooc=i64(ROWS, IDS)), r"^here: cooc must be a torch\.int32 tensor, got torch\.int64"),
    (4, dict(cost=f64(MR, MC)), r"^here: cost must be a torch\.float32 tensor, got torch\.float64"),
    (4, dict(dist_sum=f32(1)), r"^here: dist_sum must be a torch\.float64 tensor, got torch\.float32"),
    (4, dict(table=i32(16)), r"^here: table must be a torch\.int64 tensor, got torch\.int32"),
    (5, dict(totals=i32(9)), r"^here: totals must be contiguous and hold 8 elements, got \(9,\)"),
    (5, dict(id_map=strided(i32(ROWS))), r"^here: id_map must be contiguous and hold 4 elements, got \(4,\)"),
    (6, dict(), r"^pcr_amd ops run only on an MI355X device tensor .* no CPU"),    # the device comes last
)


def test_the_filler_refuses_in_its_order():
    assert set(abi.IdentCloseParams.ELEM.values()) == {torch.int32, torch.float32, torch.float64, torch.int64}
    for _, changed, pattern in FILL_REFUSALS:
        refused(lambda: close_fill(required=("flags",), **changed), pattern)
    # a call that is wrong in two ways meets the refusal of the earlier step, whichever field holds it
    pairs = [(a, b) for a in FILL_REFUSALS for b in FILL_REFUSALS if a[0] < b[0] and not set(a[1]) & set(b[1])]
    assert len(pairs) >= 40
    for (_, a, pattern), (_, b, _) in pairs:
        refused(lambda: close_fill(required=("flags",), **dict(a, **b)), pattern)
        refused(lambda: close_fill(required=("flags",), **dict(b, **a)), pattern)


def test_the_filler_leaves_unnamed_fields_and_empty_sizes_to_the_library():
    refused(lambda: close_fill(flags=None, cost=None), "no CPU")                       # not required: None is NULL
    refused(lambda: close_fill(required=("flags",), sizes=dict(CLOSE_SIZES, flags=0), flags=None), "no CPU")
    refused(lambda: close_fill(required=("flags",), sizes=dict(CLOSE_SIZES, flags=0), flags=i32(0)), "no CPU")
    # an untyped pointer takes any dtype; its size is still held
    multi = lambda ws: abi.fill(abi.AssocMultiParams(), dict(ws=ws), dict(ws=8), who="here")      # noqa: E731
    for ws in (torch.zeros(8, dtype=torch.uint8), f32(8), i64(8)):
        refused(lambda: multi(ws), "no CPU")
    refused(lambda: multi(f32(9)), "ws must be contiguous and hold 8 elements")
    assert abi.AssocMultiParams.ELEM["ws"] is None


def test_the_filler_writes_addresses_and_nulls(monkeypatch):
    """what it writes, checked without a device: `_lib.require_cuda` is the one step a host tensor cannot pass, so it is
    taken out for this test alone (the -m gpu case in tests/test_gpu_truth.py runs the real thing)"""
    from pcr_amd import _lib
    monkeypatch.setattr(_lib, "require_cuda", lambda *ts: None)
    t = dict(close_tensors(), flags=None, cost=f32(0))
    p = abi.fill(abi.IdentCloseParams(), t, dict(CLOSE_SIZES, cost=0), who="here")
    assert isinstance(p, abi.IdentCloseParams)
    for k, x in t.items():
        assert getattr(p, k) == (x.data_ptr() if x is not None and x.numel() else None), k


# ---- the same three mistakes through the public wrapper of every other filled block -----------------------------------------
def truth_call(**changed):
    from pcr_amd import truth
    t = dict(ids=i32(C), slot_gt=i32(C), slot_tte=i32(C), gt_last=i32(8), stats=i32(truth.STATS), col4row=i32(D),
             row4col=i32(G), info=i32(1), cost=f32(D, G), thresh=f32(1), gt_labels=i32(G), gt_ids=i32(G), gt_tte=i32(G),
             det_labels=i32(D), track_to_det=i32(C), det_to_track=i32(D), det_gt=i32(D), true_t2d=i32(C), true_d2t=i32(D),
             det_truth=i32(D), track_truth=i32(C))
    return lambda: truth.decide(dict(t, **changed), 8)


def bank_call(**changed):
    from pcr_amd import tracks
    state = dict(lengths=i32(C), boxes=f32(C, 9), scores=f32(C), labels=i32(C), ids=i32(C), steps=i32(C), misses=i32(C),
                 next_id=i32(1), info=i32(1))
    args = dict(track_to_det=i32(C), det_to_track=i32(D), det_labels=i32(D), det_lengths=i32(D), det_boxes=f32(D, 9),
                det_scores=f32(D), src=i32(C), det_slot=i32(D), det_id=i32(D), born=i32(D), kill=i32(C), carry=f32(3, 4))
    for k, v in changed.items():
        (state if k in state else args)[k] = v
    return lambda: tracks.plan(state, **args)


def rank_call(**changed):
    from pcr_amd import retrieval
    a = dict(scores=f32(Q, G), query_ids=i32(Q), gallery_ids=i32(G), exclude=i32(Q))
    a.update(changed)
    return lambda: retrieval.rank_gallery(a["scores"], a["query_ids"], a["gallery_ids"], topk=K, exclude=a["exclude"])


def rank_acc_call(**changed):
    from pcr_amd import retrieval
    res = dict(n_true=i32(Q), first_hit=i32(Q), info=i32(Q), ap=f32(Q))
    valid = changed.pop("valid", i32(1))
    return lambda: retrieval.RankBook(ranks=(1,), device="cpu").add(dict(res, **changed), valid=valid, gallery=G)


def multi_call(**changed):
    from pcr_amd import associate
    a = dict(logits=f32(T * D), pairs=i32(T * D, 2), count=i32(1), det_decisions=f32(1, D), track_decisions=f32(1, T),
             dist=f32(T, D))
    a.update(changed)
    return lambda: associate.association_cost_multi(a["logits"], a["pairs"], a["count"], T, D, a["det_decisions"],
                                                    a["track_decisions"], dist=a["dist"])


def decode_call(**changed):
    from pcr_amd import associate
    a = dict(cost=f32(T + D, D + T), col4row=i32(T + D), row4col=i32(D + T), solver_info=i32(1))
    a.update(changed)
    return lambda: associate.decode_assignment(a["cost"], (a["col4row"], a["row4col"], a["solver_info"]), T, D, 1, 1)


WRAPPERS = (      # (call, a field of a wrong dtype, one of a wrong size, one that is strided)
    (truth_call, dict(cost=f64(D, G)), dict(slot_gt=i32(C + 1)), dict(gt_tte=strided(i32(G)))),
    (bank_call, dict(scores=f64(C)), dict(det_labels=i32(D + 1)), dict(src=strided(i32(C)))),
    (rank_call, dict(query_ids=i64(Q)), dict(gallery_ids=i32(G + 1)), dict(exclude=strided(i32(Q)))),
    (rank_acc_call, dict(ap=f64(Q)), dict(first_hit=i32(Q + 1)), dict(info=strided(i32(Q)))),
    (multi_call, dict(logits=f64(T * D)), dict(dist=f32(T, D + 1)), dict(det_decisions=strided(f32(1, D)))),
    (decode_call, dict(col4row=i64(T + D)), dict(row4col=i32(D + T + 1)), dict(col4row=strided(i32(T + D)))),
)


@pytest.mark.parametrize("call,dtype,size,stride", WRAPPERS, ids=[w[0].__name__[:-5] for w in WRAPPERS])
def test_every_filled_block_refuses_through_its_wrapper(call, dtype, size, stride):
    (k, bad), = dtype.items()
    refused(call(**dtype), r": %s must be a torch\.\w+ tensor, got %s" % (k, re.escape(str(bad.dtype))))
    (k, bad), = size.items()
    refused(call(**size), r": %s must (be contiguous and hold \d+ elements|be \([\d, *]+\)), got %s"
            % (k, re.escape(str(tuple(bad.shape)))))
    (k, bad), = stride.items()
    refused(call(**stride), r": %s must be contiguous" % k)
    refused(call(), "no CPU")                                # right in every respect but the device: that comes last


# ---- the functions that used to assert ---------------------------------------------------------------------------------------
def test_former_assert_sites_raise_pcr_error_naming_the_argument():
    from pcr_amd import associate as A
    from pcr_amd import crops
    pairs, count, logits = i32(T * D, 2), i32(1), f32(T * D)
    cases = (
        # compare_pairs
        (lambda: A.compare_pairs(i32(T, 1), i32(D)), r"compare_pairs: track_labels must be \(\*,\), got \(3, 1\)"),
        (lambda: A.compare_pairs(i32(T), i32(D), track_lengths=i32(T + 1)), r"track_lengths must be \(3,\), got \(4,\)"),
        (lambda: A.compare_pairs(i32(T), i32(D), det_lengths=i32(D, 1)), r"det_lengths must be \(3,\)"),
        (lambda: A.compare_pairs(i32(T), i32(D), out=(i32(T * D + 1, 2), count)), r"out\[0\] \(pairs\) must be \(9, 2\)"),
        (lambda: A.compare_pairs(i32(T), i32(D), out=(strided(pairs), count)), r"out\[0\] \(pairs\) must be contiguous"),
        (lambda: A.compare_pairs(i32(T), i32(D), out=(pairs, i32(2))), r"out\[1\] \(count\) must be \(1,\)"),
        # association_cost
        (lambda: A.association_cost(logits, i32(T * D, 3), count, T, D), r"association_cost: pairs must be \(\*, 2\)"),
        (lambda: A.association_cost(logits, strided(pairs), count, T, D), r"pairs must be contiguous"),
        (lambda: A.association_cost(f32(T * D + 1), pairs, count, T, D), r"logits must be \(9,\)"),
        (lambda: A.association_cost(logits, pairs, i32(2), T, D), r"count must hold 1 elements"),
        (lambda: A.association_cost(logits, pairs, count, T, D, track_miss=f32(T + 1)), r"track_miss must be \(3,\)"),
        (lambda: A.association_cost(logits, pairs, count, T, D, det_new=strided(f32(D))), r"det_new must be contiguous"),
        (lambda: A.association_cost(logits, pairs, count, T, D, dist=f32(D + 1, T)), r"dist must be \(3, 3\)"),
        (lambda: A.association_cost(logits, pairs, count, T, D, out=f32(T + D, T + D + 1)), r"out must be \(6, 6\)"),
        # linear_assignment
        (lambda: A.linear_assignment(f32(4)), r"linear_assignment: cost must be a \(B, R, C\) or \(R, C\) tensor"),
        (lambda: A.linear_assignment(f32(4, 3).t()), r"cost must be contiguous"),
        (lambda: A.linear_assignment(f32(2, 3, 4), out=(i32(2, 3), i32(2, 4), i32(1))), r"out must hold col4row \(2, 3\)"),
        (lambda: A.linear_assignment(f32(3, 4), out=(strided(i32(1, 3)), i32(1, 4), i32(1))), r"out\[0\] \(col4row\) must be contiguous"),
        (lambda: A.linear_assignment(f32(3, 4), True, out=(i32(1, 3), i32(1, 4), i32(1), f32(1, 3), f32(1, 3))),
         r"out must hold .* u \(1, 3\) and v \(1, 4\)"),
        # box_frames
        (lambda: crops.box_frames(f32(5, 6)), r"pcr_amd\.crops: boxes must be \(\*, 7\), got \(5, 6\)"),
        (lambda: crops.box_frames(f32(7, 5).t()), r"boxes must be contiguous"),
        (lambda: crops.box_frames(f32(5, 7), out=f32(5, 3)), r"out must be \(5, 2\)"),
        # crops_from_boxes
        (lambda: crops.crops_from_boxes(f32(16, 2), f32(5, 7), 8), r"points must be \(P, C >= 3\), got \(16, 2\)"),
        (lambda: crops.crops_from_boxes(f32(16), f32(5, 7), 8), r"points must be \(\*, \*\)"),
        (lambda: crops.crops_from_boxes(f32(4, 16).t(), f32(5, 7), 8), r"points must be contiguous"),
        (lambda: crops.crops_from_boxes(f32(16, 4), f32(5, 8), 8), r"boxes must be \(\*, 7\)"),
        (lambda: crops.crops_from_boxes(f32(16, 4), f32(7, 5).t(), 8), r"boxes must be contiguous"),
        (lambda: crops.crops_from_boxes(f32(16, 4), f32(5, 7), 8, rand=i32(5, 9)), r"rand must be \(5, 8\)"),
        (lambda: crops.crops_from_boxes(f32(16, 4), f32(5, 7), 8, out=(f32(5, 8, 2), i32(5))), r"out\[0\] \(clouds\) must be"),
        (lambda: crops.crops_from_boxes(f32(16, 4), f32(5, 7), 8, out=(f32(5, 8, 3), strided(i32(5)))),
         r"out\[1\] \(lengths\) must be contiguous"),
    )
    for call, pattern in cases:
        refused(call, pattern)
    # and right in every respect but the device, each of them refuses the host tensor
    for call in (lambda: A.compare_pairs(i32(T), i32(D)), lambda: A.association_cost(logits, pairs, count, T, D),
                 lambda: A.linear_assignment(f32(3, 4)), lambda: crops.box_frames(f32(5, 7)),
                 lambda: crops.crops_from_boxes(f32(16, 4), f32(5, 7), 8)):
        refused(call, "no CPU")


def test_the_plain_argument_checker():
    t = tensor(i64(3), "f", "x", torch.int32, shape=(3,), cast_int64=True)
    assert t.dtype == torch.int32 and t.shape == (3,)
    refused(lambda: tensor(i64(3), "f", "x", torch.int32, shape=(3,)), r"^f: x must be a torch\.int32 tensor, got torch\.int64")
    v = strided(f32(2, 3))
    got = tensor(v, "f", "x", torch.float32, shape=(None, 3), copy=True)
    assert got.is_contiguous() and got.shape == v.shape
    same = f32(2, 3)
    assert tensor(same, "f", "x", torch.float32, numel=6, copy=True) is same
    assert tensor(None, "f", "x", torch.float32, optional=True) is None
    refused(lambda: tensor(None, "f", "x", torch.float32), "^f: x must be a tensor")
    refused(lambda: tensor(f32(2, 3), "f", "x", torch.float32, numel=5), r"^f: x must hold 5 elements, got \(2, 3\)")
    # the order: tensor, dtype, shape, contiguity
    refused(lambda: tensor(strided(f64(2, 3)), "f", "x", torch.float32, shape=(3, 3)), "must be a torch.float32 tensor")
    refused(lambda: tensor(strided(f32(2, 3)), "f", "x", torch.float32, shape=(3, 3)), r"must be \(3, 3\)")
    buf = i32(4, 2)
    assert out_tensor(buf, "f", "out", torch.int32, (4, 2), "cpu") is buf
    new = out_tensor(None, "f", "out", torch.int32, (4, 2), "cpu")
    assert new.shape == (4, 2) and new.dtype == torch.int32
    refused(lambda: out_tensor(buf, "f", "out", torch.int32, (2, 4), "cpu"), r"^f: out must be \(2, 4\), got \(4, 2\)")


def test_no_wrapper_module_validates_with_assert():
    """python -O drops `assert`: a check that must survive it is an `if ... raise`"""
    for m in MODULES:
        path = os.path.join(ROOT, "point-cloud-reid_amd", "pcr_amd", m + ".py")
        tree = ast.parse(open(path).read(), path)
        found = [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]
        assert not found, "%s asserts at line %s" % (path, found)
