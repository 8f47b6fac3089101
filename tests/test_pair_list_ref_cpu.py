"""CPU: the float64 restatements of training on a pair list (tests/pair_list_ref.py) hold each other -- the indexed
decomposition against the gathered form, against autograd, its per-slot records and query gradients against autograd with
A and ks as leaves, index_sum against a Python loop -- planted faults make the checks fail, the ones the per-launch GPU
tests are there for by more than the bounds test_gpu_pair_list_ops.py holds the kernels to, ReIDNet refuses cartesian
sampling with an auxiliary loss, and the golden files of the reference's cartesian train_step
(tools/make_cartesian_golden.py) say what the cartesian rule says."""
import copy
import json

import numpy as np
import pytest
import torch

import pair_list_ref as PL
import test_gpu_pair_list_ops as G          # case tables, inputs and references: plain CPU data
import train_attn_ref as R
from conftest import load_golden

F64 = torch.float64
EPS = 1e-6
M, CAP, D, H, LN = 5, 7, 64, 2, 33
# a self-pair, object 1 the template of three slots, object 3 in no slot, two dead slots that name object 4 only
PAIRS = [[0, 1], [2, 2], [2, 1], [0, 2], [1, 0], [4, 4], [4, 4]]
COUNT = 5


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(M, D, LN, generator=g, dtype=F64) for _ in range(3))
    dout = torch.randn(2 * CAP, D, LN, generator=g, dtype=F64)
    qi, si = PL.slot_lists(PAIRS, COUNT, M)
    return q, k, v, dout, qi, si


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_slot_lists_put_direction_two_behind_direction_one_and_kill_dead_slots():
    qi, si = PL.slot_lists(PAIRS, COUNT, M)
    assert qi.tolist() == [0, 2, 2, 0, 1, -1, -1, 1, 2, 1, 2, 0, -1, -1]
    assert si.tolist() == [1, 2, 1, 2, 0, -1, -1, 0, 2, 2, 0, 1, -1, -1]
    qi, si = PL.slot_lists([[0, 5], [1, 1]], None, 5)                     # an index outside [0, M): dead
    assert qi.tolist() == [-1, 1, -1, 1] and si.tolist() == [-1, 1, -1, 1]


def test_indexed_form_equals_gathered_form_in_float64():
    q, k, v, dout, qi, si = _inputs()
    ga = PL.linattn_pairs_gathered(q, k, v, qi, si, H, EPS, dout)
    ix = PL.linattn_pairs_indexed(q, k, v, qi, si, H, EPS, dout)
    for name, a, b in zip(("out", "dq", "dk", "dv"), ix, ga):
        assert _close(a, b), name
    dead = qi < 0
    assert dead.sum() == 4 and float(ix[0][dead].abs().max()) == 0.0
    for g_ in ix[1:4]:                                                    # objects 3 and 4: exactly nothing
        assert float(g_[3].abs().max()) == 0.0 and float(g_[4].abs().max()) == 0.0


def test_indexed_form_equals_autograd_of_the_gathered_forward():
    q, k, v, dout, qi, si = _inputs(1)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    alive = qi >= 0
    out = R.linattn_ref(qa[qi[alive]], ka[si[alive]], va[si[alive]], H, EPS)[0]
    out.backward(dout[alive])
    ix = PL.linattn_pairs_indexed(q, k, v, qi, si, H, EPS, dout)
    assert _close(ix[0][alive], out.detach())
    for a, b in zip(ix[1:4], (qa.grad, ka.grad, va.grad)):
        assert _close(a, b)


@pytest.mark.parametrize("fault", ["dead", "swap", "one_direction"])
def test_planted_faults_are_caught(fault):
    q, k, v, dout, qi, si = _inputs()
    ga = PL.linattn_pairs_gathered(q, k, v, qi, si, H, EPS, dout)
    bad = PL.linattn_pairs_indexed(q, k, v, qi, si, H, EPS, dout, fault=fault)
    assert not all(_close(a, b) for a, b in zip(bad[:4], ga))
    if fault == "dead":                                                   # object 0 took the dead slots' gradients
        assert not _close(bad[1], ga[1]) or not _close(bad[2], ga[2])


# ------------------------------------------------------------------------------------- the launches, one by one --
RECORD_CASES = [(64, 2, 33, "randn", "fused", EPS), (128, 2, 97, "near_eps", "fused", EPS), (64, 1, 65, "randn", "fused", EPS), (64, 2, 80, "stress", "fused", EPS),
                (64, 2, 33, "randn", "fused", 0.0)]


@pytest.mark.parametrize("case", RECORD_CASES)
def test_slot_records_and_query_gradients_equal_autograd_with_the_state_as_leaves(case):
    """apply_fwd in float64 with q, A and ks of every live slot as leaf tensors: their gradients are the slot's dqs and
    its record [dA | dks], in the kernel's layout"""
    d, Hn, Ln, draw, layout, eps = case
    dh = d // Hn
    inp = {n: t.to(F64) for n, t in G.make_pair_input(case).items()}
    qi, si = G.slot_lists_of_the_launch_cases()
    A, ks = PL.pairs_state_fwd(inp["k"], inp["v"], Hn)
    dqs, rec, (t1, t2) = PL.pairs_apply_bwd(inp["q"], A, ks, qi, si, Hn, eps, inp["dout"])
    alive = PL._alive(qi, si, G.SLOT_M)
    assert int(alive.sum()) == 7
    qg, Ag, kg = (t.clone().requires_grad_(True) for t in (inp["q"][qi[alive]], A[si[alive]], ks[si[alive]]))
    each = torch.arange(7)
    PL.pairs_apply_fwd(qg, Ag, kg, each, each, Hn, eps).backward(inp["dout"][alive])
    assert _close(dqs[alive], qg.grad) and _close(t1 + t2, dqs)
    assert _close(rec[alive][..., :dh * dh], Ag.grad.reshape(7, Hn, dh * dh))
    assert _close(rec[alive][..., dh * dh:], kg.grad)
    assert float(dqs[~alive].abs().max()) == 0.0 and float(rec[~alive].abs().max()) == 0.0
    # and the state backward from the summed records is autograd of the state forward
    drec = PL.index_sum_ref(rec, PL._sum_lists(qi, si, G.SLOT_M)[1], None, G.SLOT_M)
    kk, vv = (inp[n].clone().requires_grad_(True) for n in ("k", "v"))
    A2, ks2 = PL.pairs_state_fwd(kk, vv, Hn)
    torch.autograd.backward([A2, ks2], [drec[..., :dh * dh].reshape(A2.shape), drec[..., dh * dh:]])
    dk, dv, (u1, u2) = PL.pairs_state_bwd(inp["k"], inp["v"], drec, Hn)
    assert _close(dk, kk.grad) and _close(dv, vv.grad) and _close(u1 + u2, dk)
    assert float(dk[3].abs().max()) == 0.0 and float(dv[3].abs().max()) == 0.0


def test_every_launch_case_has_a_finite_reference_and_names_its_bound():
    """the float64 reference and the float32 yardstick of every case the GPU tests run; the stressed draws print how close
    the smallest denominator comes to eps and which outputs the yardstick, not BOUND, bounds"""
    for case in G.APPLY_CASES:
        want = G.pair_want(case)
        assert all(bool(torch.isfinite(want[n]).all()) for n in G.LAUNCH_NAMES), case
        assert all(np.isfinite(b) and b >= G.BOUND for b in want["bound"].values()), case
        yard = [n for n in G.LAUNCH_NAMES if want["bound"][n] > G.BOUND]
        if case[3] == "near_eps":
            assert 1.0 < want["den_min"] < 100.0, (case, want["den_min"])
        if case[3] != "randn" or yard:
            print(json.dumps(dict(case=str(case), den_min_over_eps=want["den_min"], y32=want["y32"], yard=yard)))
        if case[3] == "randn":
            assert not yard, (case, yard)          # a float32 evaluation holds 2e-5 / 8 on plain draws


def _launch_fault_error(case, fault):
    """the error, in the GPU test's own measure and against its own reference, of the named launch output computed with
    the planted mistake -> (error, bound)"""
    d, Hn, Ln, draw, layout, eps = case
    dh = d // Hn
    want = G.pair_want(case)
    inp = {n: t.to(F64) for n, t in G.make_pair_input(case).items()}
    qi, si = G.slot_lists_of_the_launch_cases()
    if fault == "pad_one":
        bad = PL.pairs_state_fwd(inp["k"], inp["v"], Hn, fault)[1]
        return G._launch_err(case, "ks", bad, want), want["bound"]["ks"]
    A, ks = (want["given"][n].to(F64) for n in ("A", "ks"))
    rec = PL.pairs_apply_bwd(inp["q"], A, ks, qi, si, Hn, eps, inp["dout"], fault)[1]
    return G._launch_err(case, "dA", rec[..., :dh * dh], want), want["bound"]["dA"]


@pytest.mark.parametrize("fault,case", [("pad_one", (64, 2, 33, "randn", "fused", EPS)),
                                        ("pad_one", (64, 1, 130, "randn", "fused", EPS)),
                                        ("rec_layout", (64, 2, 33, "randn", "fused", EPS)),
                                        ("rec_layout", (128, 2, 80, "stress", "fused", EPS))])
def test_planted_launch_faults_pass_the_gpu_bound(fault, case):
    err, bound = _launch_fault_error(case, fault)
    assert err > 10 * bound, (fault, case, err, bound)
    assert _launch_fault_error(case, None)[0] == 0.0


def _fn_fault_errors(qkv, dout, Mn, qi, si, D, Hn, fault):
    q, k, v = (qkv[:, n * D:(n + 1) * D].contiguous() for n in range(3))
    want = G.fn_want(q, k, v, dout, qi, si, Hn, EPS)
    bad = PL.linattn_pairs_indexed(q.to(F64), k.to(F64), v.to(F64), qi, si, Hn, EPS, dout.to(F64), fault=fault)
    return {n: float((bad[i] - want[n]).abs().max()) / want["scale"][n] for i, n in enumerate(G.FN_NAMES)}, want["bound"]


@pytest.mark.parametrize("D,Hn,Ln", [(64, 2, 33), (64, 1, 65)])
def test_a_half_dead_slot_that_sends_gradients_back_passes_the_gpu_bound(D, Hn, Ln):
    Mn, qi, si = G.fn_lists("half_dead")
    g = torch.Generator().manual_seed(D + Ln)
    qkv = torch.randn(Mn, 3 * D, Ln, generator=g)
    dout = torch.randn(qi.numel(), D, Ln, generator=g)
    err, bound = _fn_fault_errors(qkv, dout, Mn, qi, si, D, Hn, "half_dead")
    assert err["out"] == 0.0                       # the forward already kills the slot: only the backward shows it
    assert err["dq"] > 10 * bound["dq"] and err["dk"] > 10 * bound["dk"] and err["dv"] > 10 * bound["dv"], (err, bound)
    assert max(_fn_fault_errors(qkv, dout, Mn, qi, si, D, Hn, None)[0].values()) == 0.0


def test_the_fan_in_case_needs_the_second_compaction_round():
    """index sums that stop after 1024 of the 1200 slots miss the bound on every gradient"""
    qkv, dout, qi, si = G.fan_in_case()
    err, bound = _fn_fault_errors(qkv, dout, G.FAN_M, qi, si, G.FAN_D, 2, "round_1024")
    assert all(err[n] > 10 * bound[n] for n in ("dq", "dk", "dv")), (err, bound)
    assert all(b == G.BOUND for b in bound.values()), bound


def _loop_sum(src, idx, count, Mn):
    dst = [[0.0] * src.shape[1] for _ in range(Mn)]
    n = src.shape[0] if count is None else min(max(count, 0), src.shape[0])
    for p in range(n):
        if 0 <= idx[p] < Mn:
            for r in range(src.shape[1]):
                dst[idx[p]][r] += float(src[p, r])
    return torch.tensor(dst, dtype=F64).reshape(Mn, src.shape[1])


@pytest.mark.parametrize("count", [None, 6, 0, 14, -2])                   # cap, < cap, 0, > cap, negative
def test_index_sum_matches_a_python_loop(count):
    g = torch.Generator().manual_seed(3)
    src = torch.randn(9, 4, generator=g, dtype=F64)
    idx = [0, 2, 2, 7, 0, -1, 4, 2, 0]                                    # 7 and -1 outside [0, 5); objects 1 and 3 unnamed
    want = _loop_sum(src, idx, count, 5)
    got = PL.index_sum_ref(src, idx, count, 5)
    assert _close(got, want, 1e-15)
    assert float(got[1].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
    seq = PL.index_sum_seq_f32(src.float().numpy(), idx, count, 5)
    assert np.abs(seq - want.numpy()).max() < 1e-5
    if count in (0, -2):
        assert float(got.abs().max()) == 0.0


def test_index_sum_is_the_backward_of_a_gather():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(5, 3, generator=g, dtype=F64, requires_grad=True)
    idx = torch.tensor([0, 2, 2, 4, 0, 2])
    go = torch.randn(6, 3, generator=g, dtype=F64)
    x[idx].backward(go)
    assert _close(PL.index_sum_ref(go, idx, None, 5), x.grad, 1e-15)


def test_list_loss_counts_live_slots_only():
    logits = torch.tensor([0.3, -1.2, 2.0, 0.7], dtype=F64)
    match = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=F64)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    assert float(PL.list_loss_ref(logits, match, None)) == pytest.approx(float(bce(logits, match)), abs=1e-15)
    assert float(PL.list_loss_ref(logits, match, 2)) == pytest.approx(float(bce(logits[:2], match[:2])), abs=1e-15)
    assert float(PL.list_loss_ref(logits, match, 0)) == 0.0
    assert float(PL.list_loss_ref(logits, match, 9)) == pytest.approx(float(bce(logits, match)), abs=1e-15)


# ---------------------------------------------------------------------------------------------- the model's switches --
def _cfg(**losses):
    import bench
    cfg = copy.deepcopy(bench.PT_MODEL)
    cfg["losses_to_use"] = dict(kl=False, match=True, cls=False, shape=False, fp=False, triplet=False, **losses)
    return cfg


def test_sampling_is_a_constructor_keyword_and_an_attribute():
    from mmdet3d.models import build_model
    assert build_model(_cfg()).sampling is None
    m = build_model(dict(_cfg(), sampling="cartesian"))
    assert m.sampling == "cartesian"
    m._check_losses()
    m.sampling = None
    assert m.sampling is None


@pytest.mark.parametrize("name", ["cls", "fp", "kl", "triplet"])
def test_cartesian_sampling_refuses_the_auxiliary_losses(name):
    from mmdet3d.models import build_model
    from pcr_amd._lib import PcrError
    cfg = _cfg()
    cfg["losses_to_use"][name] = True
    m = build_model(cfg)
    m._check_losses()                                                     # paired sampling: allowed, as before
    m.sampling = "cartesian"
    with pytest.raises(PcrError, match=name):
        m._check_losses()


def test_match_gallery_train_needs_training_mode():
    from mmdet3d.models import build_model
    from pcr_amd._lib import PcrError
    m = build_model(_cfg()).eval()
    with pytest.raises(PcrError, match="eval mode"):
        m.match_gallery_train(torch.zeros(2, 64, 8), torch.zeros(2, 8, 3), torch.zeros(1, 2, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------- the golden files --
@pytest.mark.parametrize("tag", ["pt", "stnet", "baseline"])
def test_cartesian_goldens_say_what_the_rule_says(tag):
    g = load_golden("train_step_cartesian_%s_n128" % tag)
    meta = g["meta"]
    assert meta["pairs"] == 4 and meta["n"] == 128 and meta["id_1"] == [0, 1, 2, 3] and meta["id_2"] == [0, 1, 0, 7]
    assert np.isfinite(float(g["loss"])) and np.isfinite(float(g["loss64"]))
    assert abs(float(g["loss"]) - float(g["loss64"])) < 1e-5
    # the reference's swapped naming: num_preds_* count the TRUTH (three matches among the 16 slots), num_gt_* the predictions
    assert int(g["num_preds_1"]) == 3 and int(g["num_preds_0"]) == 13
    assert int(g["num_gt_0"]) + int(g["num_gt_1"]) == 16
    assert g["logits"].shape == (16,) and float(np.abs(g["logits64"]).min()) >= 1e-3
    assert meta["explicit_vs_cartesian64"] <= 1e-9
    grads = [k for k in g if k.startswith("grad:")]
    assert len(grads) >= 20 and all("grad64:" + k[5:] in g for k in grads)
    assert isinstance(json.loads(str(g["no_grad_params"])), list)
    # the match of slot i b + j is id_1[i] == id_2[j], and the recorded accuracy is that of the recorded logits
    match = np.array([[a == b for b in meta["id_2"]] for a in meta["id_1"]], np.float32).reshape(-1)
    assert match.sum() == 3 and match[0 * 4 + 2] == 1                      # (0, 2): the positive off the diagonal
    assert float(g["match_acc"]) == pytest.approx(float(((g["logits"] > 0) == (match > 0)).mean()), abs=1e-7)
