"""GPU: the wave-autonomous d_model = 128 kv kernel (attn_kv_stream128: SA3's self-attention key side, the K / V weight image
streamed through an LDS ring shared by a persistent workgroup's four waves, one / two / four waves per cloud by key-set
length) against the torch-eager oracle, in both arithmetic modes (f32: the tile kernels).  Key sets of 8 / 9 / 16 / 32
blocks cover every waves-per-cloud choice; batches leave the last workgroup round partly filled; nhead = 1 stays on the
tile kernel and is checked beside.  Reference: models/pointnet2_utils.py:14-47,90-114."""
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
    sd = T.seeded_state_dict(T.manifest_of(m), 7)
    m.load_state_dict(sd)
    return m.cuda().eval(), sd, (torch.randn(B, 128, L, generator=g), torch.randn(B, L, 3, generator=g))


@pytest.mark.parametrize("nhead,B,L", [(2, 5, 256), (4, 7, 256), (2, 6, 288), (4, 3, 288), (2, 3, 512), (4, 5, 512),
                                       (2, 2, 1024), (4, 3, 1024), (1, 5, 256), (1, 3, 512)])
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_d128_kv_matches_oracle(nhead, B, L, prec):
    import model_oracle as MO
    m, sd, args = _case(nhead, B, L, 7000 + 1000 * nhead + 10 * B + L)
    with torch.no_grad():
        want = MO.self_attention(sd, *args, nhead=nhead)
    with engine.precision(prec), torch.no_grad():
        got = m(*[a.cuda() for a in args]).cpu()
        again = m(*[a.cuda() for a in args]).cpu()
    assert torch.equal(got, again)                                   # fixed orders: run to run identical
    assert float((got - want).abs().max()) < 1e-4, float((got - want).abs().max())
    # a cloud alone gives the bits it gives inside the batch (the waves-per-cloud choice looks at Sk only)
    with engine.precision(prec), torch.no_grad():
        last = m(*[a[B - 1:].cuda() for a in args]).cpu()
        first = m(*[a[:1].cuda() for a in args]).cpu()
    assert torch.equal(last[0], got[B - 1])
    assert torch.equal(first[0], got[0])
