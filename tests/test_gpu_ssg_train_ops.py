"""GPU: the first-layer launches of a ball-query group in training mode (pcr_sa_l1c_fwd_f32 / pcr_sa_l1c_bwd_f32:
indexed centres, rows [dxyz, f_i], no centre half) against the float64 statement of tests/ssg_train_ref.py, twice, bit
for bit between the runs.  The launches are linear maps: nothing to condition.  Bound: PROD_BOUND = 1e-5 (`_rel`, each row
of the statistics record under its own norm), as test_gpu_train_sa_ops.py::test_sa_l1_matches_float64 holds the
first-S-points pair; that pair must still give what it gave (its own tests) -- here only that both read one cloud alike
where the groupings coincide."""
import json
import math

import pytest
import torch

import ssg_train_ref as G
from pcr_amd import _lib as L

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))


def _vs(got, want):
    return _rel(got.detach().cpu().to(F64), want.detach())


def _cu(t):
    return None if t is None else t.cuda()


def device_query(S, radius, K):
    """D-FPS + ball query on the device (pinned bit-exact to the C oracle by test_point_ops)"""
    from mmdet3d import ops

    def query(xyz):
        x = xyz.cuda().contiguous()
        centre = ops.furthest_point_sample(x, S)
        new_xyz = torch.gather(x, 1, centre.long().unsqueeze(2).expand(-1, -1, 3)).contiguous()
        return centre.cpu().to(torch.int32), ops.ball_query(0.0, radius, K, x, new_xyz).cpu()
    return query


def _launch(inp, shape):
    from pcr_amd import train_ops as TO
    B, N, S, K, c1 = shape
    xyz, idx, centre, tab = inp["xyz"].cuda(), inp["idx"].cuda(), inp["centre"].cuda(), _cu(inp["tab"])
    y = torch.empty(B, c1, S * K, device="cuda")
    st = torch.zeros(B, 2, L._c32(c1), device="cuda")
    L.run.pcr_sa_l1c_fwd_f32(xyz, idx, centre, tab, inp["wa"].cuda(), _cu(inp["bias"]), y, st, B, N, S, K, c1, L.stream_ptr())
    dtab = torch.empty(B, c1, N, device="cuda") if tab is not None else None
    dwa_p = torch.empty(B, c1, 4, device="cuda")
    L.run.pcr_sa_l1c_bwd_f32(xyz, idx, centre, inp["g"].cuda(), inp["y"].cuda(), inp["ka"].cuda(), inp["kb"].cuda(),
                             inp["kc"].cuda(), dtab, dwa_p, B, N, S, K, c1, L.stream_ptr())
    return [y, st, dtab, TO.reduce_parts(dwa_p, B, c1 * 4, c1, 4, 4)]


@pytest.mark.parametrize("shape,index_set,with_tab,with_bias", G.L1C_CASES)
def test_sa_l1c_matches_float64(shape, index_set, with_tab, with_bias):
    """y, the summed statistics, dtab (a copy counted once per copy), dwa and dbias under PROD_BOUND; two runs give the same
    bits.  Observed worst _rel on the MI355X: y 1.2e-7, sums of y 2.0e-7, of y^2 1.4e-7, dwa 3.2e-7, dbias 5.7e-7, dtab
    1.1e-6 (the "hot" set at (3, 100, 37, 20, 20): one owner adds all 740 rows of a cloud in sequence)."""
    B, N, S, K, c1 = shape
    inp = G.make_l1c_input(shape, index_set, with_tab, with_bias, device_query(S, G.BALL_RADIUS, K))
    idx, centre = inp["idx"], inp["centre"]
    assert idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < N
    assert centre.dtype == torch.int32 and tuple(centre.shape) == (B, S) and int(centre.min()) >= 0 and int(centre.max()) < N
    if index_set == "ball" and K > 1:
        cnt = G.genuine_count(idx)
        assert bool((cnt < K).any()) and bool((cnt == 1).any())
    if index_set == "random" and 2 * S <= N:
        assert int(centre[0].min()) >= S
    runs = [_launch(inp, shape) for _ in range(2)]
    for a, b in zip(*runs):
        assert (a is None and b is None) or torch.equal(a, b)
    y, st, dtab, dwa4 = runs[0]
    y64, want = G.l1c_want(inp)
    worst = dict(y=_vs(y, y64), dwa=_vs(dwa4[:, :3], want["dwa"]), dbias=_vs(dwa4[:, 3], want["dbias"]))
    sums, sums64 = st.sum(0)[:, :c1], torch.stack([y64.sum(dim=(0, 2)), (y64 * y64).sum(dim=(0, 2))])
    worst["stats_1"], worst["stats_2"] = _vs(sums[0], sums64[0]), _vs(sums[1], sums64[1])
    if with_tab:
        worst["dtab"] = _vs(dtab, want["dtab"])
    print(json.dumps(dict(op="sa_l1c", case=str((shape, index_set, with_tab, with_bias)), worst=worst)))
    assert all(math.isfinite(v) for v in worst.values()), worst
    assert max(worst.values()) < G.PROD_BOUND, worst


def test_indexed_and_prefix_launches_agree_where_the_groupings_coincide():
    """centre[b][s] = s and a zero centre half: pcr_sa_l1c_* and pcr_sa_l1_* then state the same map; one row loop and one
    owner scan serve both, so y, the statistics, dP and dwa are the same BITS"""
    B, N, S, K, c1 = shape = G.L1C_SHAPES[1]
    inp = G.make_l1c_input(shape, "random", True, True)
    inp["centre"] = torch.arange(S, dtype=torch.int32).view(1, S).expand(B, S).contiguous()
    got = _launch(inp, shape)
    xyz, idx = inp["xyz"].cuda(), inp["idx"].cuda()
    tab2 = torch.cat([inp["tab"], torch.zeros_like(inp["tab"])], dim=1).cuda()
    y = torch.empty(B, c1, S * K, device="cuda")
    st = torch.zeros(B, 2, L._c32(c1), device="cuda")
    L.run.pcr_sa_l1_fwd_f32(xyz, idx, tab2, inp["wa"].cuda(), inp["bias"].cuda(), y, st, B, N, S, K, c1, L.stream_ptr())
    dtab = torch.empty(B, 2 * c1, N, device="cuda")
    dwa_p = torch.empty(B, c1, 4, device="cuda")
    L.run.pcr_sa_l1_bwd_f32(xyz, idx, inp["g"].cuda(), inp["y"].cuda(), inp["ka"].cuda(), inp["kb"].cuda(), inp["kc"].cuda(),
                            dtab, dwa_p, B, N, S, K, c1, L.stream_ptr())
    from pcr_amd import train_ops as TO
    assert torch.equal(got[0], y) and torch.equal(got[1], st)
    assert torch.equal(got[2], dtab[:, :c1]) and torch.equal(got[3], TO.reduce_parts(dwa_p, B, c1 * 4, c1, 4, 4))
