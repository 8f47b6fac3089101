"""GPU: the wave-autonomous d_model = 128 apply kernel (attn_apply_stream128: SA3's self-attention, weights streamed through
an LDS ring shared by a persistent workgroup's four waves) against the torch-eager oracle, in both arithmetic modes (f32:
the tile kernels), over query sets of 8 / 9 / 32 blocks, head counts 1 / 2 / 4 and batches whose block count leaves
the last workgroup round partly filled; query sets of one block (Lq = 32) stay on the tile kernel and are checked beside.  Reference: models/pointnet2_utils.py:14-47,90-114."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

from pcr_amd import engine, testing as T

pytestmark = pytest.mark.gpu


def _case(nhead, B, L, seed):
    from mmdet3d.models.pointnet2_utils import Self_Attention
    g = torch.Generator().manual_seed(seed)
    m = Self_Attention(128, nhead)
    sd = T.seeded_state_dict(T.manifest_of(m), 5)
    m.load_state_dict(sd)
    return m.cuda().eval(), sd, (torch.randn(B, 128, L, generator=g), torch.randn(B, L, 3, generator=g))


@pytest.mark.parametrize("nhead,B,L", [(2, 3, 32), (2, 5, 256), (1, 3, 288), (4, 7, 32), (2, 2, 1024), (4, 1, 288),
                                       (1, 6, 256)])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_d128_self_attention_matches_oracle(nhead, B, L, prec):
    import model_oracle as MO
    m, sd, args = _case(nhead, B, L, 1000 * nhead + 10 * B + L)
    with torch.no_grad():
        want = MO.self_attention(sd, *args, nhead=nhead)
    with engine.precision(prec), torch.no_grad():
        got = m(*[a.cuda() for a in args]).cpu()
        again = m(*[a.cuda() for a in args]).cpu()
    assert torch.equal(got, again)                                   # fixed orders: run to run identical
    assert float((got - want).abs().max()) < 1e-4, float((got - want).abs().max())
    # a cloud alone gives the bits it gives inside the batch (persistent workgroups; the work split is by block)
    with engine.precision(prec), torch.no_grad():
        one = m(*[a[B - 1:].cuda() for a in args]).cpu()
        first = m(*[a[:1].cuda() for a in args]).cpu()
    assert torch.equal(one[0], got[B - 1])
    assert torch.equal(first[0], got[0])

