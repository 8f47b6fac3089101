"""GPU: the launches of training on a pair list (include/pcr.h section C3; csrc/train_pair_kernels.hip).

pcr_index_sum_f32 is held bit for bit to a numpy float32 sum in list order.

The indexed linear attention is held to the float64 restatement of tests/pair_list_ref.py LAUNCH BY LAUNCH
(pcr_linattn_{state,apply}_{fwd,bwd}_f32 called directly on guarded buffers: operands and outputs embedded in tensors full
of a sentinel) and then as the Function train_ops.LinAttnPairs.  Every backward launch, and apply_fwd, reads the float64
reference's records rounded once to float32 (A | ks; drec), so an error of one launch cannot hide behind another.

Bounds.  The kernels are the arithmetic of linattn_*_mfma_kernel tile for tile, which test_gpu_train_attn_ops.py holds to
BOUND = 2e-5 of the tensor's scale at these head widths: the same bound here, or, where it is larger, YARD = 8 times the
error of a float32 CPU evaluation of the reference on the same case (`lin_bound`; computed here on the CPU, never read
off the kernel).  The stressed draws are what need it.  With ONE token dqs and dk are cancellations (train_attn_ref):
their error is held on the scale of the larger cancelling term.  The gradients of the Function are sums over slots in
float32 list order: their error is held on the scale of the sum of the absolute per-slot contributions
(pair_list_ref.linattn_pairs_scales).  LinAttn on gathered tensors, the route the library had before, is printed next to
it and asserts nothing.

Cases, from the code (kAT = 64 tokens per chunk, KT = nl > 32 ? 64 : 32, tiles of 32): (d, H) = (64, 2) -> <32>, wave 0 owns
A; (128, 2) -> <64>, four tiles; (64, 1) -> <64> with one head; L = 1, 32, 33, 64, 65, 80 (a full chunk, then a 16-token
tail: KT 64 then 32 over stale second-tile columns), 97, 130.  One list for all of them (SLOT_QI / SLOT_SI).  The case
tables and every reference are plain CPU data, shared with test_pair_list_ref_cpu.py."""
import functools
import json

import numpy as np
import pytest
import torch

import pair_list_ref as PL
from test_gpu_train_attn_ops import BOUND, SENTINEL, YARD, _rel

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 1e-6
GUARD = 64                  # sentinel floats on either side of a flat output
DEAD_ROW_HOLDS = SENTINEL   # what the dqs / rec rows of a dead slot hold after apply_bwd: what they held before


# ------------------------------------------------------------------------------------------------- index_sum --
def _index_sum_case(P, M, R, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(P, R, generator=g)
    idx = torch.randint(0, M, (P,), generator=g, dtype=torch.int32)
    if M > 2:
        idx[idx == 1] = 0                      # object 1: no slot names it
    if P > 8:
        idx[3], idx[7] = M, -1                 # two indices outside [0, M)
    return src, idx


def _run_index_sum(src, idx, count, M):
    """-> the (M + 2, R) buffer whose rows 1 .. M the launch wrote; rows 0 and M + 1 are guards"""
    from pcr_amd import _lib as L
    P, R = src.shape
    buf = torch.full((M + 2, R), 12345.0, dtype=torch.float32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    L.run.pcr_index_sum_f32(src.cuda(), idx.cuda(), cnt, buf[1:M + 1], P, M, R, L.stream_ptr())
    return buf.cpu()


def _index_sum_check(src, idx, M, counts, tag):
    P = src.shape[0]
    for count in counts:
        want = PL.index_sum_seq_f32(src.numpy(), idx.numpy(), count, M)
        got = _run_index_sum(src, idx, count, M)
        again = _run_index_sum(src, idx, count, M)
        assert np.array_equal(got[1:M + 1].numpy().view(np.int32), want.view(np.int32)), (tag, count)
        assert bool((got[0] == 12345.0).all()) and bool((got[M + 1] == 12345.0).all()), (tag, count)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (tag, count)
        if count == 0:
            assert not got[1:M + 1].view(torch.int32).any()              # +0 everywhere


# kSumCols = 1024 columns per workgroup: R = 1023 / 1024 / 1025; kSumList = 1024 slots per compaction round: P = 1024 / 1025 /
# 2048 (one full round, a round + 1 slot, two full rounds)
@pytest.mark.parametrize("shape", [(37, 5, 130), (64, 8, 64 * 128), (1, 1, 1), (37, 5, 1023), (37, 5, 1024), (37, 5, 1025),
                                   (1024, 3, 70), (1025, 3, 70), (2048, 3, 70)])
def test_index_sum_is_the_sequential_float32_sum(shape):
    P, M, R = shape
    src, idx = _index_sum_case(P, M, R, seed=P)
    _index_sum_check(src, idx, M, (0, P - 3, P, P + 5, None), shape)


@pytest.mark.parametrize("P", [1024, 1025, 2048])
def test_index_sum_when_every_slot_names_one_object(P):
    """the compacted list of ONE workgroup row is full in every round, the other objects' stay empty"""
    M, R = 3, 70
    src, _ = _index_sum_case(P, M, R, seed=P + 1)
    idx = torch.full((P,), 1, dtype=torch.int32)
    _index_sum_check(src, idx, M, (P - 3, None), P)
    got = _run_index_sum(src, idx, None, M)
    assert not got[1].view(torch.int32).any() and not got[3].view(torch.int32).any()      # objects 0 and 2: +0


def test_index_sum_walks_a_list_longer_than_one_round():
    """3000 slots: the workgroups compact the list 1024 slots at a time"""
    P, M, R = 3000, 3, 70
    src, idx = _index_sum_case(P, M, R, seed=11)
    want = PL.index_sum_seq_f32(src.numpy(), idx.numpy(), 2900, M)
    got = _run_index_sum(src, idx, 2900, M)
    assert np.array_equal(got[1:M + 1].numpy().view(np.int32), want.view(np.int32))


def test_pair_gather_sends_dead_slots_nowhere():
    from pcr_amd import train_ops as TO
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 6, generator=g).cuda().requires_grad_(True)
    idx = torch.tensor([2, 0, 2, -1, 4, 3], dtype=torch.int32, device="cuda")
    go = torch.randn(6, 3, 6, generator=g).cuda()
    y = TO.pair_gather(x, idx)
    assert torch.equal(y[:3], x.detach()[[2, 0, 2]]) and torch.equal(y[5], x.detach()[3])
    y.backward(go)
    want = PL.index_sum_seq_f32(go.cpu().numpy().reshape(6, -1), idx.cpu().numpy(), None, 4).reshape(4, 3, 6)
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    assert not x.grad[1].view(torch.int32).any()
    # count = 2: only the first two slots send a gradient back
    x.grad = None
    TO.pair_gather(x, idx, torch.tensor([2], dtype=torch.int32, device="cuda")).backward(go)
    want = PL.index_sum_seq_f32(go.cpu().numpy().reshape(6, -1), idx.cpu().numpy(), 2, 4).reshape(4, 3, 6)
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), want.view(np.int32))
    assert not x.grad[3].view(torch.int32).any()


# ------------------------------------------------------------------------- indexed attention, launch by launch --
# The list of every launch case: M = 4 objects, R = 10 slots (queries of qi[r] against the state of si[r]).  Slot 0 is a
# self-slot; object 2 is the state of FIVE slots (1, 2, 4, 6, 8; slot 4 a self-slot again); object 3 is in no slot; slot 3
# is dead in both lists, slot 5 has qi valid and si = M, slot 7 has qi = -1 and si valid.
SLOT_M = 4
SLOT_QI = [0, 0, 1, -1, 2, 1, 1, -1, 0, 2]
SLOT_SI = [0, 2, 2, -1, 2, 4, 2, 0, 2, 1]
STRESS_OBJECT = 1           # (the state of slot 9)

DH_FORMS = [(64, 2), (128, 2), (64, 1)]
LAUNCH_LS = [1, 32, 33, 64, 65, 80, 97, 130]
# (d, H, L, draw, layout, eps).  draw "stress": q and k times 4 (elu saturates on one side, K' spans e^-12 .. 13) and the k of
# STRESS_OBJECT shifted by -8; that leaves the smallest Q'.ks near 1e8 eps (K' > 1 wherever k > 0), so "near_eps" draws the k
# of that object as N(-20, 1) instead: Q'.ks of the slot that reads it comes within two orders of magnitude of eps
# (test_pair_list_ref_cpu.py prints and checks it).  layout "fused": q | k | v rows of ONE (M, 3d + 4, L) buffer, one batch stride; "split": q, k,
# v, dk, dv in separate tensors with q_bs = (d + 3) L, kv_bs = (d + 5) L, dkv_bs = (d + 7) L, sentinel rows between objects.
LAUNCH_CASES = [(d, H, Ln, "randn", "fused", EPS) for d, H in DH_FORMS for Ln in LAUNCH_LS]
LAUNCH_CASES += [(d, H, 80, "stress", "fused", EPS) for d, H in DH_FORMS]
LAUNCH_CASES += [(d, H, 97, "near_eps", "fused", EPS) for d, H in DH_FORMS]
LAUNCH_CASES += [(64, 2, 33, "randn", "split", EPS), (128, 2, 80, "randn", "split", EPS), (64, 1, 65, "randn", "split", EPS)]
# eps = 0: a padding token's 1 / (Q'.ks + eps) is 1 / 0; L = 33: KT = 64 over 31 padding tokens, L = 80: a 16-token tail
EPS0_CASES = [(d, H, Ln, "randn", "fused", 0.0) for d, H in DH_FORMS for Ln in (33, 80)]
APPLY_CASES = LAUNCH_CASES + EPS0_CASES


def slot_lists_of_the_launch_cases():
    return torch.tensor(SLOT_QI), torch.tensor(SLOT_SI)


@functools.lru_cache(maxsize=None)
def make_pair_input(case):
    """float32 CPU tensors of one launch case: q, k, v (M,d,L), dout (R,d,L)"""
    d, H, Ln, draw, layout, eps = case
    g = torch.Generator().manual_seed((d * 1009 + H * 101 + Ln * 7 + len(draw)) % (2 ** 31))
    q, k, v = (torch.randn(SLOT_M, d, Ln, generator=g) for _ in range(3))
    dout = torch.randn(len(SLOT_QI), d, Ln, generator=g)
    if draw != "randn":
        q, k = 4.0 * q, 4.0 * k
        k[STRESS_OBJECT] = k[STRESS_OBJECT] - 8.0 if draw == "stress" else k[STRESS_OBJECT] / 4.0 - 20.0
    return dict(q=q, k=k, v=v, dout=dout)


def _launch_eval(inp, case, dtype, rec32):
    """every launch's outputs in `dtype` from the float32 inputs; the launches that read records read rec32 = the
    float32 A, ks, drec (None: this evaluation's own, rounded to float32 -- how the float64 reference makes them)"""
    d, H, Ln, draw, layout, eps = case
    qi, si = slot_lists_of_the_launch_cases()
    q, k, v, dout = (inp[n].to(dtype) for n in ("q", "k", "v", "dout"))
    dh = d // H
    A, ks = PL.pairs_state_fwd(k, v, H)
    rec32 = dict(rec32) if rec32 else dict(A=A.float(), ks=ks.float())
    Ar, ksr = rec32["A"].to(dtype), rec32["ks"].to(dtype)
    out = PL.pairs_apply_fwd(q, Ar, ksr, qi, si, H, eps)
    dqs, rec, (t1, t2) = PL.pairs_apply_bwd(q, Ar, ksr, qi, si, H, eps, dout)
    if "drec" not in rec32:
        rec32["drec"] = PL.index_sum_ref(rec, *PL._sum_lists(qi, si, SLOT_M)[1:], None, SLOT_M).float()
    dk, dv, (u1, u2) = PL.pairs_state_bwd(k, v, rec32["drec"].to(dtype), H)
    return dict(A=A, ks=ks, out=out, dqs=dqs, dA=rec[..., :dh * dh], dks=rec[..., dh * dh:], dk=dk, dv=dv,
                terms=dict(dqs=max(float(t1.abs().max()), float(t2.abs().max())),
                           dk=max(float(u1.abs().max()), float(u2.abs().max())))), rec32


def _launch_err(case, name, got, want):
    """max |got - reference| over the tensor's scale: max |reference|, or with ONE token, for the two cancellations, the
    larger cancelling term"""
    if case[2] == 1 and name in ("dqs", "dk"):
        return float((got - want[name]).abs().max()) / want["terms"][name]
    return _rel(got, want[name])


LAUNCH_NAMES = ("A", "ks", "out", "dqs", "dA", "dks", "dk", "dv")


@functools.lru_cache(maxsize=None)
def pair_want(case):
    """the float64 reference of every launch of one case, computed once: the outputs by name, `given` = the float32
    records the launches are fed, `bound` = max(BOUND, YARD y32) by name with y32 the error of the float32 CPU evaluation
    of the same launches on the same operands, `den_min` = the smallest live Q'.ks over eps"""
    d, H, Ln, draw, layout, eps = case
    inp = make_pair_input(case)
    want, given = _launch_eval(inp, case, F64, None)
    f32, _ = _launch_eval(inp, case, torch.float32, given)
    want["given"] = given
    want["y32"] = {n: _launch_err(case, n, f32[n].to(F64), want) for n in LAUNCH_NAMES}
    want["bound"] = {n: max(BOUND, YARD * want["y32"][n]) for n in LAUNCH_NAMES}
    qi, si = slot_lists_of_the_launch_cases()
    want["alive"], _, Qp, _, kss = PL._slot_operands(inp["q"].to(F64), want["A"], want["ks"], qi, si, H)
    want["den_min"] = float(torch.einsum("rhil,rhi->rhl", Qp, kss)[want["alive"]].min()) / max(eps, 1e-30)
    return want


def _specs(d, layout):
    """name -> (buffer, channel rows of that buffer, first row of the block)"""
    if layout == "fused":
        rows = 3 * d + 4
        return dict(q=("qkv", rows, 1), k=("qkv", rows, 2 + d), v=("qkv", rows, 3 + 2 * d),
                    dk=("dqkv", rows, 2 + d), dv=("dqkv", rows, 3 + 2 * d))
    return dict(q=("q", d + 3, 1), k=("k", d + 5, 2), v=("v", d + 5, 3), dk=("dk", d + 7, 3), dv=("dv", d + 7, 4))


def _place(case, names, blocks=None):
    """-> (buffers by key, (M,d,L) device views by name, batch stride in floats by name): buffers full of SENTINEL with
    the named blocks (None: left as sentinel, for a launch to write) embedded"""
    d, H, Ln, draw, layout, eps = case
    spec = _specs(d, layout)
    bufs = {}
    for n in names:
        key, rows, lo = spec[n]
        buf = bufs.setdefault(key, torch.full((SLOT_M, rows, Ln), SENTINEL))
        if blocks is not None:
            buf[:, lo:lo + d] = blocks[n]
    bufs = {key: buf.cuda() for key, buf in bufs.items()}
    views = {n: bufs[spec[n][0]][:, spec[n][2]:spec[n][2] + d] for n in names}
    return bufs, views, {n: spec[n][1] * Ln for n in names}


def _gaps_intact(case, bufs, names):
    """every row of the buffers outside the named blocks -- the rows between the objects -- still holds the sentinel"""
    d = case[0]
    spec = _specs(d, case[4])
    for key, buf in bufs.items():
        keep = torch.ones(buf.shape[1], dtype=torch.bool)
        for n in names:
            if spec[n][0] == key:
                keep[spec[n][2]:spec[n][2] + d] = False
        assert int(keep.sum()) >= 3
        assert bool((buf.cpu()[:, keep] == SENTINEL).all()), (case, key)


def _flat(*shape):
    """-> (buffer, view of `shape` in its middle): GUARD sentinel floats before and after, the view sentinel too"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _flat_intact(*bufs):
    for buf in bufs:
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _untouched(t):
    return bool((t == SENTINEL).all())


def _operands(case, names):
    inp = make_pair_input(case)
    bufs, views, bs = _place(case, names, inp)
    return bufs, {k_: b.clone() for k_, b in bufs.items()}, views, bs


def _only_read(bufs, before):
    for key in bufs:
        assert torch.equal(bufs[key], before[key]), key


def _lists():
    qi, si = slot_lists_of_the_launch_cases()
    return qi.int().cuda(), si.int().cuda()


def _eps_t(eps):
    return torch.full((1,), eps, dtype=torch.float32, device="cuda")


def _run_state_fwd(case):
    from pcr_amd import _lib as L
    d, H, Ln = case[:3]
    dh = d // H
    bufs, before, ops, bs = _operands(case, ("k", "v"))
    assert bs["k"] == bs["v"]
    Ab, A = _flat(SLOT_M, H, dh, dh)
    kb, ks = _flat(SLOT_M, H, dh)
    L.run.pcr_linattn_state_fwd_f32(ops["k"], ops["v"], bs["k"], A, ks, SLOT_M, Ln, d, H, L.stream_ptr())
    torch.cuda.synchronize()
    _only_read(bufs, before)
    _flat_intact(Ab, kb)
    return dict(A=A.clone(), ks=ks.clone())


def _run_apply_fwd(case, given):
    from pcr_amd import _lib as L
    d, H, Ln, draw, layout, eps = case
    Rn = len(SLOT_QI)
    bufs, before, ops, bs = _operands(case, ("q",))
    ob, out = _flat(Rn, d, Ln)
    qi, si = _lists()
    L.run.pcr_linattn_apply_fwd_f32(ops["q"], bs["q"], given["A"].cuda(), given["ks"].cuda(), qi, si, _eps_t(eps), out,
                                    SLOT_M, Rn, Ln, d, H, L.stream_ptr())
    torch.cuda.synchronize()
    _only_read(bufs, before)
    _flat_intact(ob)
    return dict(out=out.clone())


def _run_apply_bwd(case, given):
    from pcr_amd import _lib as L
    d, H, Ln, draw, layout, eps = case
    Rn, dh = len(SLOT_QI), d // H
    bufs, before, ops, bs = _operands(case, ("q",))
    db, dqs = _flat(Rn, d, Ln)
    rb, rec = _flat(Rn, H, dh * (dh + 1))
    qi, si = _lists()
    L.run.pcr_linattn_apply_bwd_f32(ops["q"], bs["q"], given["A"].cuda(), given["ks"].cuda(), qi, si, _eps_t(eps),
                                    make_pair_input(case)["dout"].cuda(), dqs, rec, SLOT_M, Rn, Ln, d, H, L.stream_ptr())
    torch.cuda.synchronize()
    _only_read(bufs, before)
    _flat_intact(db, rb)
    return dict(dqs=dqs.clone(), rec=rec.clone())


def _run_state_bwd(case, given):
    from pcr_amd import _lib as L
    d, H, Ln = case[:3]
    bufs, before, ops, bs = _operands(case, ("k", "v"))
    dbufs, outs, dbs = _place(case, ("dk", "dv"))
    assert dbs["dk"] == dbs["dv"] and (case[4] == "fused" or len({bs["k"], dbs["dk"], (d + 3) * Ln}) == 3)
    L.run.pcr_linattn_state_bwd_f32(ops["k"], ops["v"], bs["k"], given["drec"].cuda(), outs["dk"], outs["dv"], dbs["dk"],
                                    SLOT_M, Ln, d, H, L.stream_ptr())
    torch.cuda.synchronize()
    _only_read(bufs, before)
    _gaps_intact(case, dbufs, ("dk", "dv"))
    return dict(dk=outs["dk"].clone(), dv=outs["dv"].clone())


def _twice(run, *args):
    a, b = run(*args), run(*args)
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    return {n: t.cpu() for n, t in a.items()}


def _launch_check(op, case, got, want, names, rows=None):
    """every named output (its `rows`) within its bound; the worst errors, the bounds and the names that fell back to the
    float32 yardstick go out as one JSON line"""
    worst = {}
    for n in names:
        ref = dict(want, **{n: want[n][rows]}) if rows is not None else want
        worst[n] = _launch_err(case, n, (got[n][rows] if rows is not None else got[n]).to(F64), ref)
    bounds = {n: want["bound"][n] for n in names}
    print(json.dumps(dict(op=op, case=str(case), worst=worst, bound=bounds,
                          yard=[n for n in names if bounds[n] > BOUND])))
    for n in names:
        assert bool(torch.isfinite(got[n][rows] if rows is not None else got[n]).all()), (op, case, n)
        assert worst[n] < bounds[n], (op, case, n, worst[n], bounds[n])


@pytest.mark.parametrize("case", LAUNCH_CASES)
def test_pair_state_fwd_matches_float64(case):
    want = pair_want(case)
    got = _twice(_run_state_fwd, case)
    _launch_check("pair_state_fwd", case, got, want, ("A", "ks"))


@pytest.mark.parametrize("case", APPLY_CASES)
def test_pair_apply_fwd_matches_float64(case):
    want = pair_want(case)
    alive = want["alive"]
    assert (~alive).tolist() == [r in (3, 5, 7) for r in range(len(SLOT_QI))]
    got = _twice(_run_apply_fwd, case, want["given"])
    _launch_check("pair_apply_fwd", case, got, want, ("out",), alive)
    assert not got["out"][~alive].view(torch.int32).any()                 # all three kinds of dead slot: +0, every bit


@pytest.mark.parametrize("case", APPLY_CASES)
def test_pair_apply_bwd_matches_float64(case):
    d, H = case[:2]
    dh = d // H
    want = pair_want(case)
    alive = want["alive"]
    got = _twice(_run_apply_bwd, case, want["given"])
    got.update(dA=got["rec"][..., :dh * dh], dks=got["rec"][..., dh * dh:])
    _launch_check("pair_apply_bwd", case, got, want, ("dqs", "dA", "dks"), alive)
    # a dead slot of any kind: nothing written
    assert bool((got["dqs"][~alive] == DEAD_ROW_HOLDS).all()) and bool((got["rec"][~alive] == DEAD_ROW_HOLDS).all())


@pytest.mark.parametrize("case", LAUNCH_CASES)
def test_pair_state_bwd_matches_float64(case):
    want = pair_want(case)
    got = _twice(_run_state_bwd, case, want["given"])
    _launch_check("pair_state_bwd", case, got, want, ("dk", "dv"))
    # object 3 is in no slot: drec = 0, and so are dk and dv, to the bit
    assert not want["given"]["drec"][3].view(torch.int32).any()
    assert not got["dk"][3].contiguous().view(torch.int32).any() and not got["dv"][3].contiguous().view(torch.int32).any()


def test_pair_launches_with_nothing_to_do_write_nothing():
    """M = 0 (state launches) and R = 0 (apply launches): PCR_OK (L.run raises otherwise), every output still sentinel"""
    from pcr_amd import _lib as L
    case = (64, 2, 33, "randn", "split", EPS)
    d, H, Ln = case[:3]
    dh = d // H
    given = pair_want(case)["given"]
    bufs, before, ops, bs = _operands(case, ("q", "k", "v"))
    dbufs, outs, dbs = _place(case, ("dk", "dv"))
    flats = [_flat(SLOT_M, H, dh, dh), _flat(SLOT_M, H, dh), _flat(2, d, Ln), _flat(2, d, Ln), _flat(2, H, dh * (dh + 1))]
    (_, A), (_, ks), (_, out), (_, dqs), (_, rec) = flats
    qi, si = _lists()
    dout = make_pair_input(case)["dout"].cuda()
    A_in, ks_in, s = given["A"].cuda(), given["ks"].cuda(), L.stream_ptr()
    L.run.pcr_linattn_state_fwd_f32(ops["k"], ops["v"], bs["k"], A, ks, 0, Ln, d, H, s)
    L.run.pcr_linattn_apply_fwd_f32(ops["q"], bs["q"], A_in, ks_in, qi, si, _eps_t(EPS), out, SLOT_M, 0, Ln, d, H, s)
    L.run.pcr_linattn_apply_bwd_f32(ops["q"], bs["q"], A_in, ks_in, qi, si, _eps_t(EPS), dout, dqs, rec, SLOT_M, 0, Ln, d, H, s)
    L.run.pcr_linattn_state_bwd_f32(ops["k"], ops["v"], bs["k"], given["drec"].cuda(), outs["dk"], outs["dv"], dbs["dk"],
                                    0, Ln, d, H, s)
    torch.cuda.synchronize()
    _only_read(bufs, before)
    assert all(_untouched(buf) for buf, _ in flats) and all(_untouched(buf) for buf in dbufs.values())


# --------------------------------------------------------------------------------- indexed attention, Function --
M, CAP, H = 5, 7, 2
# a self-pair (2, 2), object 1 the template of three slots, object 3 in no slot, two dead slots that name object 4 only
PAIRS = [[0, 1], [2, 2], [2, 1], [0, 2], [1, 0], [4, 4], [4, 4]]
COUNT = 5
FN_NAMES = ("out", "dq", "dk", "dv")


def fn_lists(which):
    """-> (M, qi, si): "pairs" = the slot lists of PAIRS / COUNT (dead slots -1 in both lists), "half_dead" = the list of
    the launch cases, half-dead slots as they are"""
    if which == "pairs":
        return (M,) + tuple(PL.slot_lists(PAIRS, COUNT, M))
    return (SLOT_M,) + tuple(slot_lists_of_the_launch_cases())


def fn_want(q, k, v, dout, qi, si, Hn, eps):
    """float32 CPU tensors -> dict(out, dq, dk, dv in float64; scale = max |out| and the maxima of the sums of absolute
    per-slot contributions; bound = max(BOUND, YARD y32) with y32 the float32 CPU evaluation's error on those scales)"""
    ref = PL.linattn_pairs_indexed(q.to(F64), k.to(F64), v.to(F64), qi, si, Hn, eps, dout.to(F64))
    f32 = PL.linattn_pairs_indexed(q, k, v, qi, si, Hn, eps, dout)
    sc = PL.linattn_pairs_scales(q.to(F64), k.to(F64), v.to(F64), qi, si, Hn, eps, dout.to(F64))
    want = dict(zip(FN_NAMES, ref[:4]))
    want["scale"] = dict(out=max(1e-6, float(ref[0].abs().max())), **{n: float(sc[n].max()) for n in ("dq", "dk", "dv")})
    y32 = {n: float((f32[i].to(F64) - ref[i]).abs().max()) / want["scale"][n] for i, n in enumerate(FN_NAMES)}
    want["bound"] = {n: max(BOUND, YARD * y32[n]) for n in FN_NAMES}
    return want


def _poison(*numels):
    """NaN through freed blocks of the sizes the backward is about to torch.empty: a row that apply_bwd leaves unwritten
    holds NaN, not whatever was there, if anything adds it to an object"""
    blocks = [torch.full((n,), float("nan"), device="cuda") for n in numels]      # all held at once, then all freed
    torch.cuda.synchronize()
    del blocks


def _fn_check(tag, qkv, dout, Mn, qi, si, D, Hn, Ln, gathered=True):
    from pcr_amd import train_ops as TO
    alive = PL._alive(qi, si, Mn)
    q, k, v = (qkv[:, n * D:(n + 1) * D].contiguous() for n in range(3))
    want = fn_want(q, k, v, dout, qi, si, Hn, EPS)
    Rn, dh = qi.numel(), D // Hn

    def indexed():
        x = qkv.cuda().requires_grad_(True)
        out = TO.LinAttnPairs.apply(x, qi.int().cuda(), si.int().cuda(), Hn, EPS)
        go = dout.cuda()                     # (before the poison: it is of the size of dqs)
        _poison(Rn * D * Ln, Rn * Hn * dh * (dh + 1))
        out.backward(go)
        return out.detach(), x.grad
    out, dqkv = indexed()
    out2, dqkv2 = indexed()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(dqkv.view(torch.int32), dqkv2.view(torch.int32))
    got = dict(out=out.cpu(), **{n: dqkv[:, i * D:(i + 1) * D].cpu() for i, n in enumerate(("dq", "dk", "dv"))})
    worst = {n: float((got[n].to(F64) - want[n]).abs().max()) / want["scale"][n] for n in FN_NAMES}
    line = dict(op=tag, d=D, H=Hn, L=Ln, R=Rn, indexed_vs_f64=worst, bound=want["bound"],
                yard=[n for n in FN_NAMES if want["bound"][n] > BOUND])

    if gathered:
        # printed only: LinAttn on the gathered operands of the live slots, per-slot gradients added per object in f32
        ql, sl = qi[alive], si[alive]
        ops = [t.cuda().requires_grad_(True) for t in (q[ql], k[sl], v[sl])]
        yo = TO.LinAttn.apply(*ops, Hn, EPS)
        yo.backward(dout[alive].cuda())
        ysum = [torch.from_numpy(PL.index_sum_seq_f32(t.grad.cpu().numpy().reshape(len(ql), -1), ix.numpy(), None, Mn))
                .reshape(Mn, D, Ln) for t, ix in zip(ops, (ql, sl, sl))]
        old = dict(out=float((yo.detach().cpu().to(F64) - want["out"][alive]).abs().max()) / want["scale"]["out"])
        old.update({n: float((ysum[i].to(F64) - want[n]).abs().max()) / want["scale"][n]
                    for i, n in enumerate(("dq", "dk", "dv"))})
        line["gathered_vs_f64"] = old
    print(json.dumps(line))
    for n in FN_NAMES:
        assert worst[n] < want["bound"][n], (tag, n, worst[n], want["bound"][n])
    # dead slots: zeros out; an object no live slot queries with / reads the state of: exactly zero bits
    assert not got["out"][~alive].view(torch.int32).any()
    for m in range(Mn):
        if m not in qi[alive].tolist():
            assert not got["dq"][m].contiguous().view(torch.int32).any(), m
        if m not in si[alive].tolist():
            assert not got["dk"][m].contiguous().view(torch.int32).any(), m
            assert not got["dv"][m].contiguous().view(torch.int32).any(), m
    return got


FN_CASES = [(64, 2, 64), (64, 2, 128), (64, 2, 33), (128, 2, 33), (64, 1, 65)]      # head widths 32 and 64; one head of 64


@pytest.mark.parametrize("which", ["pairs", "half_dead"])
@pytest.mark.parametrize("D,Hn,Ln", FN_CASES)
def test_indexed_attention_matches_float64(D, Hn, Ln, which):
    """LinAttnPairs, forward and backward, on the list of PAIRS and on the list with half-dead slots: a slot with ONE
    index outside [0, M) gives zeros and sends nothing back, to either object"""
    Mn, qi, si = fn_lists(which)
    g = torch.Generator().manual_seed(D + Ln)
    qkv = torch.randn(Mn, 3 * D, Ln, generator=g)
    dout = torch.randn(qi.numel(), D, Ln, generator=g)
    got = _fn_check("LinAttnPairs " + which, qkv, dout, Mn, qi, si, D, Hn, Ln)
    if which == "pairs":
        assert not any(got[n][m].contiguous().view(torch.int32).any() for n in ("dq", "dk", "dv") for m in (3, 4))
    else:
        assert not any(got[n][3].contiguous().view(torch.int32).any() for n in ("dq", "dk", "dv"))


FAN_CAP, FAN_M, FAN_D, FAN_L = 600, 3, 64, 16       # 1200 slots over three objects: past kSumList = 1024 in both sums


def fan_in_case():
    g = torch.Generator().manual_seed(600)
    pairs = torch.randint(0, FAN_M, (FAN_CAP, 2), generator=g)
    qi, si = PL.slot_lists(pairs, None, FAN_M)
    qkv = torch.randn(FAN_M, 3 * FAN_D, FAN_L, generator=g)
    dout = torch.randn(2 * FAN_CAP, FAN_D, FAN_L, generator=g)
    return qkv, dout, qi, si


def test_indexed_attention_sums_past_one_compaction_round():
    """every object is named by ~400 slots of each list, its last ones beyond slot 1024: the record sum and the dqs sum
    both run a second compaction round of pcr_index_sum_f32"""
    qkv, dout, qi, si = fan_in_case()
    assert min(int((qi[1024:] == m).sum()) for m in range(FAN_M)) > 0
    assert min(int((si[1024:] == m).sum()) for m in range(FAN_M)) > 0
    _fn_check("LinAttnPairs fan-in", qkv, dout, FAN_M, qi, si, FAN_D, 2, FAN_L, gathered=False)


def test_indexed_attention_refuses_head_widths_it_does_not_cover():
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    assert TO.linattn_pairs_ok(64, 2) and TO.linattn_pairs_ok(128, 2) and TO.linattn_pairs_ok(64, 1)
    assert not TO.linattn_pairs_ok(64, 4) and not TO.linattn_pairs_ok(256, 2) and not TO.linattn_pairs_ok(60, 2)
    qkv = torch.zeros(2, 3 * 64, 16, device="cuda")
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(L.PcrError):
        TO.LinAttnPairs.apply(qkv, idx, idx, 4, EPS)
