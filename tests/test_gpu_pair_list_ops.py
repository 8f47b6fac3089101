"""GPU: the launches of training on a pair list (include/pcr.h section C3; csrc/train_pair_kernels.hip).

pcr_index_sum_f32 is held bit for bit to a numpy float32 sum in list order.  The indexed linear attention
(train_ops.LinAttnPairs: state per object, apply per slot, records, index sums) is held to the float64 restatement of
tests/pair_list_ref.py with the route the library had before as the yardstick: LinAttn on gathered per-slot tensors, its
per-slot gradients added per object in float32 in list order.  The indexed route may be at most twice as far from float64
as that route, with a floor of 1e-6 of the tensor's scale (the level test_gpu_train_attn_ops.py reports for this head
width)."""
import json

import numpy as np
import pytest
import torch

import pair_list_ref as PL

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 1e-6
FLOOR = 1e-6


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


@pytest.mark.parametrize("shape", [(37, 5, 130), (64, 8, 64 * 128), (1, 1, 1)])
def test_index_sum_is_the_sequential_float32_sum(shape):
    P, M, R = shape
    src, idx = _index_sum_case(P, M, R, seed=P)
    for count in (0, P - 3, P, P + 5, None):
        want = PL.index_sum_seq_f32(src.numpy(), idx.numpy(), count, M)
        got = _run_index_sum(src, idx, count, M)
        again = _run_index_sum(src, idx, count, M)
        assert np.array_equal(got[1:M + 1].numpy().view(np.int32), want.view(np.int32)), (shape, count)
        assert bool((got[0] == 12345.0).all()) and bool((got[M + 1] == 12345.0).all()), (shape, count)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), (shape, count)
        if count == 0:
            assert not got[1:M + 1].view(torch.int32).any()              # +0 everywhere


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


# ---------------------------------------------------------------------------------------- indexed attention --
M, CAP, H = 5, 7, 2
# a self-pair (2, 2), object 1 the template of three slots, object 3 in no slot, two dead slots that name object 4 only
PAIRS = [[0, 1], [2, 2], [2, 1], [0, 2], [1, 0], [4, 4], [4, 4]]
COUNT = 5


def _err(got, want):
    return float((got.detach().cpu().to(F64) - want).abs().max()) / max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("D,Ln", [(64, 64), (64, 128), (64, 33), (128, 33)])       # head widths 32 and 64
def test_indexed_attention_matches_float64_no_worse_than_the_gathered_route(D, Ln):
    from pcr_amd import train_ops as TO
    g = torch.Generator().manual_seed(D + Ln)
    qkv = torch.randn(M, 3 * D, Ln, generator=g)
    dout = torch.randn(2 * CAP, D, Ln, generator=g)
    qi, si = PL.slot_lists(PAIRS, COUNT, M)
    alive = qi >= 0
    q, k, v = (qkv[:, n * D:(n + 1) * D].contiguous() for n in range(3))
    want = PL.linattn_pairs_gathered(q.to(F64), k.to(F64), v.to(F64), qi, si, H, EPS, dout.to(F64))
    assert all(PL._alive(qi, si, M) == alive)

    def indexed():
        x = qkv.cuda().requires_grad_(True)
        out = TO.LinAttnPairs.apply(x, qi.int().cuda(), si.int().cuda(), H, EPS)
        out.backward(dout.cuda())
        return out.detach(), x.grad
    out, dqkv = indexed()
    out2, dqkv2 = indexed()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(dqkv.view(torch.int32), dqkv2.view(torch.int32))

    # the yardstick: LinAttn on the gathered operands of the live slots, per-slot gradients added per object in f32
    ql, sl = qi[alive], si[alive]
    ops = [t.cuda().requires_grad_(True) for t in (q[ql], k[sl], v[sl])]
    yo = TO.LinAttn.apply(*ops, H, EPS)
    yo.backward(dout[alive].cuda())
    ysum = [torch.from_numpy(PL.index_sum_seq_f32(t.grad.cpu().numpy().reshape(len(ql), -1), ix.numpy(), None, M))
            .reshape(M, D, Ln) for t, ix in zip(ops, (ql, sl, sl))]

    errs = dict(out=(_err(out[alive.cuda()], want[0][alive]), _err(yo, want[0][alive])))
    for n, name in enumerate(("dq", "dk", "dv")):
        errs[name] = (_err(dqkv[:, n * D:(n + 1) * D], want[1 + n]), _err(ysum[n], want[1 + n]))
    print(json.dumps(dict(d=D, L=Ln, indexed_vs_f64={k_: e[0] for k_, e in errs.items()},
                          gathered_vs_f64={k_: e[1] for k_, e in errs.items()})))
    for name, (new, old) in errs.items():
        assert new <= max(2.0 * old, FLOOR), (name, new, old)
    # dead slots: zeros out; objects 3 (in no slot) and 4 (named by dead slots only): exactly zero bits everywhere
    assert not out[(~alive).cuda()].view(torch.int32).any()
    assert not dqkv[3].view(torch.int32).any() and not dqkv[4].view(torch.int32).any()


def test_indexed_attention_refuses_head_widths_it_does_not_cover():
    from pcr_amd import _lib as L
    from pcr_amd import train_ops as TO
    assert TO.linattn_pairs_ok(64, 2) and TO.linattn_pairs_ok(128, 2) and TO.linattn_pairs_ok(64, 1)
    assert not TO.linattn_pairs_ok(64, 4) and not TO.linattn_pairs_ok(256, 2) and not TO.linattn_pairs_ok(60, 2)
    qkv = torch.zeros(2, 3 * 64, 16, device="cuda")
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(L.PcrError):
        TO.LinAttnPairs.apply(qkv, idx, idx, 4, EPS)
