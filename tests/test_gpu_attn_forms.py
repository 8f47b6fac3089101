"""GPU: every launch form of the inference attention block (pcr_attn_kv_f32 / pcr_attn_apply_f32) against the float64
restatement of tests/attn_ref.py, one row per kernel instantiation, in both arithmetic modes.

Bounds.  err = max|got - attn_ref| over the whole output.  Two yardsticks are computed HERE, on the CPU, from the same
inputs (tests/test_attn_ref_cpu.py proves them): y32 = max|model_oracle in float32 - attn_ref| (what float32 arithmetic
costs on this case) and ysplit = max|attn_ref(mm=split_mm) - attn_ref| (what dropping the lo x lo term of every product
costs).  f32 mode and every d > 128 case (attn_bf sends those to the f32 unit): err <= 4 y32 -- the margin
test_gpu_decisions.py uses over a measured float32 deviation; the kernels round in more places than torch (once-rounded
folded weights, another accumulation order, hardware exp / rsqrt).  bf16x3 mode, d <= 128: err <= min(1e-4,
2 ysplit + 4 y32) -- 2 for the spread of a maximum over ~1e4 elements and for kernels that split fewer phases than the
model (the tile kv kernel projects in f32).  No bound is read off a kernel.

Also, per row: a second run is bit-equal; the first and the last cloud alone give the bits they give in the batch; the
kernels the library reports (pcr_attn_launch_form) for the very blocks AttnPlan.kv / .apply launched are the row's entry
of EXPECT below -- the map of rows to kernel instantiations, as data -- and after the kv launch pcr_last_launch_arith()
says the arithmetic that report names.  And the key-side state by itself: M and ksum are
unpacked from the kv launch's image (`unpack_state`) and held to attn_ref.kv_state by the same two yardsticks taken on M
and ksum (`state_bounds`) -- norm1 cancels a uniform scale of M Q', so a wrong normaliser of the mean over the key tokens
is invisible in the block's output and visible only here.

The gated twins (GATE = true) are held bit-equal to these by test_gpu_match_live.py.  The two `fpq`
rows are forms no shipped module builds -- q_pos with cout = 128 or a trailing conv, while the only q_pos block,
Self_Attention, has a residual (cout = c1 = d) and no conv -- so they go through engine.AttnPlan itself: an FP_SA's
weights with q_pos = 1, the query features carrying pos_mlp2 of their own coordinates.

OBSERVED err / bound on an MI355X, `row f32|bf16x3 [M f32, ksum f32 | M bf16x3, ksum bf16x3]` (the brackets:
test_kv_state_against_float64); every row printed by `pytest -s`.  Largest: 0.44 in f32 mode (self-d512-h2-L40), 0.57 in
bf16x3 mode (cross-reversed), 0.43 on the state (cross-d32-h2-96x256, M in f32 mode); "bf16" gave the bits of "bf16x3".
  self-d32-h1-L64 0.27|0.45 [0.26 0.03|0.15 0.14];  self-d32-h4-L64 0.29|0.39 [0.23 0.02|0.20 0.13]
  self-d32-h2-L45 0.18|0.34 [0.35 0.03|0.14 0.01];  self-d32-h2-L1 0.31|0.31 [0.33 0.30|0.11 0.01]
  self-d64-h2-L96 0.23|0.38 [0.20 0.01|0.16 0.15];  self-d64-h2-L160 0.22|0.40 [0.18 0.01|0.20 0.09]
  self-d64-h1-L64 0.25|0.42 [0.36 0.02|0.22 0.23];  self-d64-h4-L64 0.20|0.41 [0.25 0.01|0.20 0.17]
  self-d64-h2-L45 0.23|0.40 [0.23 0.02|0.15 0.01];  self-d96-h2-L40 0.20|0.44 [0.27 0.04|0.16 0.01]
  self-d96-h3-L40 0.27|0.32 [0.28 0.05|0.13 0.01];  self-d128-h2-L256 0.38|0.48 [0.26 0.01|0.17 0.05]
  self-d128-h4-L512 0.37|0.43 [0.41 0.01|0.25 0.02];  self-d128-h1-L256 0.32|0.42 [0.29 0.01|0.20 0.06]
  self-d128-h2-L270 0.32|0.45 [0.25 0.01|0.23 0.05];  self-d128-h2-L32 0.32|0.39 [0.28 0.06|0.14 0.02]
  self-d256-h2-L40 0.33|0.33 [0.20 0.03|0.20 0.03];  self-d256-h4-L40 0.40|0.40 [0.32 0.03|0.32 0.03]
  self-d512-h2-L40 0.43|0.43 [0.37 0.04|0.37 0.04];  self-d512-h4-L40 0.42|0.42 [0.31 0.05|0.31 0.05]
  cross-d64-h2-64x32 0.22|0.38 [0.27 0.06|0.20 0.25];  cross-d64-h2-33x70 0.21|0.45 [0.24 0.03|0.14 0.02]
  cross-d32-h2-96x256 0.19|0.38 [0.42 0.00|0.20 0.04];  cross-d128-h2-64x256 0.34|0.43 [0.35 0.02|0.22 0.04]
  cross-d64-h2-32x1 0.29|0.35 [0.33 0.28|0.15 0.01];  cross-d64-h1-32x160 0.20|0.46 [0.23 0.01|0.22 0.06]
  cross-reversed 0.19|0.57 [0.23 0.02|0.20 0.17];  cross-gallery-L64 0.18|0.38 [0.21 0.02|0.24 0.16]
  cross-gallery-L33 0.17|0.38 [0.20 0.02|0.18 0.15];  fp-3-64-64-32-f64 0.20|0.45 [0.21 0.03|0.16 0.16]
  fp-3-64-64-32-f64-ragged 0.25|0.48 [0.21 0.03|0.20 0.13];  fp-3-64-64-32-f32 0.27|0.43 [0.27 0.02|0.25 0.13]
  fp-32-128-64-64-k128 0.26|0.39 [0.26 0.02|0.19 0.08];  fp-32-128-64-64-k96 0.31|0.46 [0.26 0.01|0.19 0.01]
  fp-32-128-64-64-h1 0.25|0.42 [0.22 0.01|0.20 0.06];  fp-32-128-64-64-f128 0.18|0.41 [0.24 0.01|0.20 0.08]
  fp-64-128-64-128 0.20|0.37 [0.21 0.01|0.19 0.05];  fp-64-64-64-64-f128 0.26|0.38 [0.22 0.02|0.23 0.13]
  fp-64-256-128-128 0.26|0.41 [0.24 0.06|0.13 0.02];  fp-3-128-128-64-f64 0.24|0.38 [0.32 0.07|0.12 0.03]
  fp-32-32-32-160 0.20|0.39 [0.22 0.05|0.14 0.02];  fp-64-128-64-160 0.26|0.38 [0.27 0.05|0.13 0.02]
  fpq-64-64-64-128 0.30|0.41 [0.22 0.02|0.16 0.13];  fpq-64-64-64-64-f128 0.29|0.44 [0.21 0.02|0.17 0.16]
  fp-32-128-64-64-split[splits=2] 0.26|0.38;  fp-32-128-64-64-split[splits=3] 0.24|0.37
  cross-d64-h2-33x200[splits=2] 0.22|0.43;  cross-d64-h2-33x200[splits=3] 0.22|0.43;  self-d64-h2-L96[x16] 0.25|0.44
  self-d128-h2-L256[x16] 0.36|0.42;  fp-32-128-64-64-k128[x16] 0.21|0.47;  cross-d64-h2-32x32[B=2051] -|0.42
  fp-3-64-64-32[B=2051] -|0.46;  self-d32-h2-L32[B=2051] -|0.42
  pooled (max, sum / Lq bound): cross-reversed 0.24, 0.12; cross-gallery-L64 0.37, 0.11
"""
import functools
import types
import zlib
from typing import NamedTuple, Optional, Tuple

import pytest
import torch
import torch.nn.functional as F

import attn_ref as R

F64 = torch.float64
ARITH = {"f32": 0, "bf16x3": 1, "bf16": 2}


class Case(NamedTuple):
    name: str
    kind: str                      # "self" | "cross" | "fp" | "fpq" (FP_SA weights planned with q_pos = 1)
    dims: Tuple[int, int, int, int]  # c1, c2, d, cout
    nhead: int
    B: int
    Lq: int
    Sk: int
    cfinal: int = 0
    Bk: Optional[int] = None       # key-side clouds (default B)
    q_index: Optional[tuple] = None
    kv_index: Optional[tuple] = None
    n_out: Optional[int] = None

    @property
    def indexed(self):
        return self.kv_index is not None or self.q_index is not None


def _self(d, nhead, L, B=3):
    return Case("self-d%d-h%d-L%d" % (d, nhead, L), "self", (d, d, d, d), nhead, B, L, L)


def _cross(d, nhead, Lq, Sk, B=3, tag=None, **kw):
    return Case(tag or "cross-d%d-h%d-%dx%d" % (d, nhead, Lq, Sk), "cross", (d, d, d, d), nhead, B, Lq, Sk, **kw)


def _fp(c1, c2, d, out, Lq, Sk, cfinal=0, nhead=2, tag="", B=3, kind="fp"):
    name = "%s-%d-%d-%d-%d%s" % (kind, c1, c2, d, out, tag)
    return Case(name, kind, (c1, c2, d, out), nhead, B, Lq, Sk, cfinal)


# position MLP, q_pos, k_pos, residual per kind: the three modules' flags and the plan-only q_pos form
FLAGS = dict(R.FLAGS, fpq=("pos_mlp2", 1, 0, 0))


_GQ, _GK = (0, 1, 2, 0, 1, 2, 1), (0, 1, 2, 3, 3, 0, 2)       # gallery: 3 query clouds x 4 key clouds, 7 combinations

CASES = [
    _self(32, 1, 64), _self(32, 4, 64), _self(32, 2, 45), _self(32, 2, 1),
    _self(64, 2, 96), _self(64, 2, 160), _self(64, 1, 64), _self(64, 4, 64), _self(64, 2, 45),
    _self(96, 2, 40), _self(96, 3, 40),
    _self(128, 2, 256), _self(128, 4, 512, B=2), _self(128, 1, 256), _self(128, 2, 270), _self(128, 2, 32),
    _self(256, 2, 40, B=2), _self(256, 4, 40, B=2), _self(512, 2, 40, B=2), _self(512, 4, 40, B=2),
    _cross(64, 2, 64, 32), _cross(64, 2, 33, 70), _cross(32, 2, 96, 256), _cross(128, 2, 64, 256), _cross(64, 2, 32, 1),
    _cross(64, 1, 32, 160),
    _cross(64, 2, 64, 64, tag="cross-reversed", kv_index=(2, 1, 0)),
    _cross(64, 2, 64, 64, tag="cross-gallery-L64", Bk=4, q_index=_GQ, kv_index=_GK, n_out=7),
    _cross(64, 2, 33, 64, tag="cross-gallery-L33", Bk=4, q_index=_GQ, kv_index=_GK, n_out=7),
    _fp(3, 64, 64, 32, 96, 64, cfinal=64, tag="-f64"), _fp(3, 64, 64, 32, 50, 64, cfinal=64, tag="-f64-ragged"),
    _fp(3, 64, 64, 32, 96, 64, cfinal=32, tag="-f32"),
    _fp(32, 128, 64, 64, 64, 128, tag="-k128"), _fp(32, 128, 64, 64, 64, 96, tag="-k96"),
    _fp(32, 128, 64, 64, 64, 128, nhead=1, tag="-h1"),
    _fp(32, 128, 64, 64, 64, 128, cfinal=128, tag="-f128"),
    _fp(64, 128, 64, 128, 64, 160), _fp(64, 64, 64, 64, 64, 64, cfinal=128, tag="-f128"),
    _fp(64, 256, 128, 128, 40, 24), _fp(3, 128, 128, 64, 40, 24, cfinal=64, tag="-f64"),
    _fp(32, 32, 32, 160, 40, 24), _fp(64, 128, 64, 160, 40, 24),
    _fp(64, 64, 64, 128, 64, 64, kind="fpq"), _fp(64, 64, 64, 64, 64, 64, cfinal=128, tag="-f128", kind="fpq"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SPLIT_CASES = [_fp(32, 128, 64, 64, 64, 173, tag="-split"), _cross(64, 2, 33, 200)]
SCALE_CASES = ["self-d64-h2-L96", "self-d128-h2-L256", "fp-32-128-64-64-k128"]
TWIN_CASES = ["self-d64-h2-L160", "fp-3-64-64-32-f64"]              # bf16 == bf16x3, bit for bit
POOL_CASES = ["cross-reversed", "cross-gallery-L64"]
MANY = {"self": _self(32, 2, 32, B=5), "cross": _cross(64, 2, 32, 32, B=5), "fp": _fp(3, 64, 64, 32, 32, 32, cfinal=64, B=5)}

# ---- which kernels a row runs: row -> ((kv, apply) in f32 mode, (kv, apply) in bf16x3 mode), each spelled as a kernel
# trace spells the instantiation (attn_ref.kernel_name).  The x16 rows (SCALE_CASES) and the B = 8 CUs + 3 rows (MANY) run
# their row's kernels: the batch and the values never enter the choice.  tests/test_attn_ref_cpu.py holds every entry to
# what the library reports for the row's block, and every instantiation the dispatch can reach to an entry here (or, for
# the gated twins, in tests/test_gpu_match_live.py).  Compiled but out of reach, so in no row:
#   attn_apply_stream64_kernel<true, 4, 0, 4, 2, false>   q_pos with cout = 128: its weight images need 168 704 bytes of
#       LDS, 4 864 more than a workgroup can have, so `fpq-64-64-64-128` runs the tile kernel
#   attn_apply_kernel<2, 2, true>   a gated block has cout = 64, and no shipped trailing conv is wider than 128
#   attn_kv_kernel_o2<1, 2, 1, 4, true> of the f32 unit   BFP needs the bf16 unit's image
_KT32, _KT96, _KO3 = "attn_kv_kernel<2, 1, 2, 1>", "attn_kv_kernel<1, 2, 0, 4>", "attn_kv_kernel_o3<2, 1, 1, 1>"
_KO2, _KO2B = "attn_kv_kernel_o2<1, 2, 1, 4, false>", "attn_kv_kernel_o2<1, 2, 1, 4, true>"
_KS_F1, _KS_F2 = "attn_kv_stream64_kernel<false, false, 4, false>", "attn_kv_stream64_kernel<true, false, 4, false>"
_KS_1W1, _KS_1W2 = "attn_kv_stream64_kernel<false, true, 4, true>", "attn_kv_stream64_kernel<true, true, 4, true>"
_KS_B1, _KS_B2 = "attn_kv_stream64_kernel<false, true, 4, false>", "attn_kv_stream64_kernel<true, true, 4, false>"
_KS_X1, _KS_X2 = "attn_kv_stream64_kernel<false, true, 8, false>", "attn_kv_stream64_kernel<true, true, 8, false>"
_K32, _K128_2, _K128_4 = "attn_kv_stream32_kernel", "attn_kv_stream128_kernel<2>", "attn_kv_stream128_kernel<4>"
_KW2, _KW3 = "attn_kv_wide_kernel<2>", "attn_kv_wide_kernel<3>"
_AT41, _AT42, _AT21, _AT22 = ("attn_apply_kernel<%s>" % a for a in ("4, 1", "4, 2", "2, 1", "2, 2"))
_AT12, _AT14, _AT18 = ("attn_apply_kernel<%s>" % a for a in ("1, 2", "1, 4", "1, 8"))
_AS32Q, _AS32 = "attn_apply_stream64_kernel<true, 2, 0, 1, 1, false>", "attn_apply_stream64_kernel<false, 2, 0, 1, 1, false>"
_ASQ, _ASX = "attn_apply_stream64_kernel<true, 4, 0, 2, 2, false>", "attn_apply_stream64_kernel<false, 4, 0, 2, 2, false>"
_ASQF, _ASXF = "attn_apply_stream64_kernel<true, 4, 4, 2, 2, false>", "attn_apply_stream64_kernel<false, 4, 4, 2, 2, false>"
_ASH, _ASHF = "attn_apply_stream64_kernel<false, 2, 0, 2, 2, false>", "attn_apply_stream64_kernel<false, 2, 4, 2, 2, false>"
_AS3, _ASW = "attn_apply_stream64_kernel<false, 1, 2, 1, 2, false>", "attn_apply_stream64_kernel<false, 4, 0, 4, 2, false>"
_ASP = "attn_apply_stream64_kernel<false, 4, 0, 2, 2, true>"
_A128 = {h: "attn_apply_stream128_kernel<%d>" % h for h in (1, 2, 4)}
EXPECT = {
    "self-d32-h1-L64": ((_KT32, _AT41), (_K32, _AS32Q)),
    "self-d32-h4-L64": ((_KT32, _AT41), (_K32, _AT41)),
    "self-d32-h2-L45": ((_KT32, _AT41), (_KT32, _AT41)),
    "self-d32-h2-L1": ((_KT32, _AT41), (_KT32, _AT41)),
    "self-d64-h2-L96": ((_KS_F2, _AT21), (_KS_1W2, _ASQ)),
    "self-d64-h2-L160": ((_KS_F2, _AT21), (_KS_B2, _ASQ)),
    "self-d64-h1-L64": ((_KS_F1, _AT21), (_KS_1W1, _ASQ)),
    "self-d64-h4-L64": ((_KS_F2, _AT21), (_KS_1W2, _ASQ)),
    "self-d64-h2-L45": ((_KO3, _AT21), (_KO3, _AT21)),
    "self-d96-h2-L40": ((_KT96, _AT12), (_KT96, _AT12)),
    "self-d96-h3-L40": ((_KT96, _AT12), (_KT96, _AT12)),
    "self-d128-h2-L256": ((_KO2, _AT12), (_K128_2, _A128[2])),
    "self-d128-h4-L512": ((_KO2, _AT12), (_K128_4, _A128[4])),
    "self-d128-h1-L256": ((_KO2, _AT12), (_KO2B, _A128[1])),
    "self-d128-h2-L270": ((_KO2, _AT12), (_KO2B, _AT12)),
    "self-d128-h2-L32": ((_KO2, _AT12), (_KO2, _AT12)),
    "self-d256-h2-L40": ((_KW2, _AT14), (_KW2, _AT14)),
    "self-d256-h4-L40": ((_KW2, _AT14), (_KW2, _AT14)),
    "self-d512-h2-L40": ((_KW3, _AT18), (_KW3, _AT18)),
    "self-d512-h4-L40": ((_KW2, _AT18), (_KW2, _AT18)),
    "cross-d64-h2-64x32": ((_KS_F2, _AT21), (_KS_1W2, _ASX)),
    "cross-d64-h2-33x70": ((_KO3, _AT21), (_KO3, _AT21)),
    "cross-d32-h2-96x256": ((_KT32, _AT41), (_K32, _AS32)),
    "cross-d128-h2-64x256": ((_KO2, _AT12), (_K128_2, _AT12)),
    "cross-d64-h2-32x1": ((_KO3, _AT21), (_KO3, _ASX)),
    "cross-d64-h1-32x160": ((_KS_F1, _AT21), (_KS_B1, _ASX)),
    "cross-reversed": ((_KS_F2, _AT21), (_KS_1W2, _ASX)),
    "cross-gallery-L64": ((_KS_F2, _AT21), (_KS_1W2, _ASX)),
    "cross-gallery-L33": ((_KS_F2, _AT21), (_KS_1W2, _AT21)),
    "fp-3-64-64-32-f64": ((_KS_F2, _AT21), (_KS_1W2, _AS3)),
    "fp-3-64-64-32-f64-ragged": ((_KS_F2, _AT21), (_KS_1W2, _AT21)),
    "fp-3-64-64-32-f32": ((_KS_F2, _AT21), (_KS_1W2, _AT21)),
    "fp-32-128-64-64-k128": ((_KO3, _AT21), (_KS_X2, _ASH)),
    "fp-32-128-64-64-k96": ((_KO3, _AT21), (_KO3, _ASH)),
    "fp-32-128-64-64-h1": ((_KO3, _AT21), (_KS_X1, _ASH)),
    "fp-32-128-64-64-f128": ((_KO3, _AT21), (_KS_X2, _ASHF)),
    "fp-64-128-64-128": ((_KO3, _AT21), (_KS_X2, _ASW)),
    "fp-64-64-64-64-f128": ((_KS_F2, _AT21), (_KS_1W2, _ASXF)),
    "fp-64-256-128-128": ((_KO2, _AT12), (_KO2, _AT12)),
    "fp-3-128-128-64-f64": ((_KO2, _AT12), (_KO2, _AT12)),
    "fp-32-32-32-160": ((_KT32, _AT42), (_KT32, _AT42)),
    "fp-64-128-64-160": ((_KO3, _AT22), (_KO3, _AT22)),
    "fpq-64-64-64-128": ((_KS_F2, _AT21), (_KS_1W2, _AT21)),
    "fpq-64-64-64-64-f128": ((_KS_F2, _AT21), (_KS_1W2, _ASQF)),
    # token split (attn_kv_fold_kernel follows the kv kernel), both counts
    "fp-32-128-64-64-split[splits=2]": ((_KO3, _AT21), (_KO3, _ASH)),
    "fp-32-128-64-64-split[splits=3]": ((_KO3, _AT21), (_KO3, _ASH)),
    "cross-d64-h2-33x200[splits=2]": ((_KO3, _AT21), (_KO3, _AT21)),
    "cross-d64-h2-33x200[splits=3]": ((_KO3, _AT21), (_KO3, _AT21)),
    # pooled output (None: pcr_attn_apply_pool_ok says no and the launch is refused)
    "cross-reversed[pooled]": ((_KS_F2, None), (_KS_1W2, _ASP)),
    "cross-gallery-L64[pooled]": ((_KS_F2, None), (_KS_1W2, _ASP)),
    "cross-d64-h2-32x32[pooled]": ((_KS_F2, None), (_KS_1W2, _ASP)),
    # test_more_work_than_workgroups
    "self-d32-h2-L32": ((_KT32, _AT41), (_K32, _AS32Q)),
    "cross-d64-h2-32x32": ((_KS_F2, _AT21), (_KS_1W2, _ASX)),
    "fp-3-64-64-32": ((_KS_F2, _AT21), (_KS_1W2, _AS3)),
}


# ------------------------------------------------------------------------------------------ CPU side --
def build_module(case):
    """the shipped module of the row with its seeded weights (and the fused trailing conv), on the CPU"""
    from pcr_amd import testing as T
    from mmdet3d.models.attention import corss_attention
    from mmdet3d.models.pointnet2_utils import FP_SA, Self_Attention
    c1, c2, d, cout = case.dims
    if case.kind == "self":
        m = Self_Attention(d, case.nhead)
    elif case.kind == "cross":
        m = corss_attention(d, case.nhead)
    else:                               # "fp", "fpq"
        m = FP_SA(0, c1, c2, d, cout, case.nhead)
    m.load_state_dict(T.seeded_state_dict(T.manifest_of(m), 5))
    conv = None
    if case.cfinal:
        conv = torch.nn.Conv1d(cout, case.cfinal, 1)
        conv.load_state_dict(T.seeded_state_dict(T.manifest_of(conv), 6))
        m.fuse_final_conv(conv)
    return m.eval(), conv


def case_data(case, scale=1.0):
    """state dict, trailing conv and the randn inputs of a row (features x scale)"""
    m, conv = build_module(case)
    c1, c2, d, cout = case.dims
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    tt = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    fq, xq = tt(case.B, c1, case.Lq) * scale, tt(case.B, case.Lq, 3)
    if case.kind == "self":
        fk, xk = fq, xq
    else:
        Bk = case.Bk or case.B
        fk, xk = tt(Bk, c2, case.Sk) * scale, tt(Bk, case.Sk, 3)
    final = None if conv is None else (conv.weight.detach()[:, :, 0].clone(), conv.bias.detach().clone())
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return types.SimpleNamespace(sd=sd, final=final, fq=fq, xq=xq, fk=fk, xk=xk)


def ref_eval(case, dt, mm=R.exact_mm, stages=None, **kw):
    """attn_ref on a row's data (unpooled unless pooled=True is passed)"""
    if case.kind == "self":
        return R.self_attention(dt.sd, dt.fq, dt.xq, case.nhead, mm=mm, stages=stages, **kw)
    if case.kind == "cross":
        return R.cross_attention(dt.sd, dt.fq, dt.xq, dt.fk, dt.xk, case.nhead, mm=mm, stages=stages,
                                 kv_index=case.kv_index, q_index=case.q_index, n_out=case.n_out, **kw)
    if case.kind == "fpq":
        pos_name, q_pos, k_pos, residual = FLAGS["fpq"]
        M, ksum = R.kv_state(dt.sd, pos_name, dt.fk, dt.xk, case.nhead, k_pos, mm=mm, stages=stages)
        return R.apply_block(dt.sd, pos_name, dt.fq, dt.xq, M, ksum, case.Sk, case.nhead, q_pos, residual,
                             final=dt.final, mm=mm, stages=stages, **kw)
    return R.fp_sa(dt.sd, dt.fq, dt.xq, dt.fk, dt.xk, case.nhead, final=dt.final, mm=mm, stages=stages, **kw)


def oracle_eval(case, dt, dtype):
    """oracle/model_oracle.py on the same data in `dtype`; index forms by explicit gathering, the conv by F.conv1d"""
    import model_oracle as MO
    c = lambda t: t.to(dtype)      # noqa: E731
    sd = {k: c(v) for k, v in dt.sd.items()}
    with torch.no_grad():
        if case.kind == "self":
            return MO.self_attention(sd, c(dt.fq), c(dt.xq), case.nhead)
        n = case.n_out if case.n_out is not None else case.B
        qi = torch.arange(n) if case.q_index is None else torch.tensor(case.q_index)[:n]
        ki = torch.arange(n) if case.kv_index is None else torch.tensor(case.kv_index)[:n]
        args = (sd, c(dt.fq)[qi], c(dt.xq)[qi], c(dt.fk)[ki], c(dt.xk)[ki], case.nhead)
        if case.kind == "cross":
            return MO.cross_attention(*args)
        if case.kind == "fpq":
            f1, f2 = args[1].permute(0, 2, 1), args[3].permute(0, 2, 1)
            out = MO.attention_block(sd, f1 + MO._pos_mlp(sd, "pos_mlp2", args[2]), f2,
                                     f2 + MO._pos_mlp(sd, "pos_mlp2", args[4]), f1, case.nhead, False).permute(0, 2, 1)
        else:
            out = MO.fp_sa(*args)
        if dt.final is not None:
            out = F.conv1d(out, c(dt.final[0]).unsqueeze(-1), c(dt.final[1]))
        return out


def _yard(case, scale):
    dt = case_data(case, scale)
    ref = ref_eval(case, dt)
    y32 = float((oracle_eval(case, dt, torch.float32).double() - ref).abs().max())
    ysplit = float((ref_eval(case, dt, mm=R.split_mm) - ref).abs().max())
    return types.SimpleNamespace(case=case, data=dt, ref=ref, y32=y32, ysplit=ysplit)


@functools.lru_cache(maxsize=None)
def _yard_cached(case, scale):
    return _yard(case, scale)


def yardsticks(case, scale=1.0):
    """(computed once per row and shared; nothing mutates it) -> .data, .ref (float64), .y32, .ysplit"""
    return _yard_cached(case, float(scale))


def state32(case, dt):
    """(M, ksum) of the key side in float32 torch, the oracle's order of operations (einsum attention, then merge)"""
    pos_name, _, k_pos, _ = FLAGS[case.kind]
    sd = {k: v.float() for k, v in dt.sd.items()}
    with torch.no_grad():
        f = dt.fk.float().permute(0, 2, 1)
        hid = F.relu(F.linear(dt.xk.float(), sd[pos_name + ".0.weight"], sd[pos_name + ".0.bias"]))
        pos = F.linear(hid, sd[pos_name + ".2.weight"], sd[pos_name + ".2.bias"])
        B, S, _ = f.shape
        d, H = case.dims[2], case.nhead
        K = (F.elu(F.linear(f + pos if k_pos else f, sd["k_proj.weight"])) + 1).view(B, S, H, d // H)
        V = F.linear(f + pos, sd["v_proj.weight"]).view(B, S, H, d // H) / S
        KV = torch.einsum("nshd,nshv->nhdv", K, V)
        M = torch.einsum("ohv,nhdv->nohd", sd["merge.weight"].view(d, H, d // H), KV).reshape(B, d, d)
        return M, K.sum(dim=1).reshape(B, d)


@functools.lru_cache(maxsize=None)
def state_yardsticks(case):
    """the same two yardsticks for the key-side state: .M, .ksum (float64) and (y32, ysplit) of each"""
    dt = yardsticks(case).data
    pos_name, _, k_pos, _ = FLAGS[case.kind]
    M, ksum = R.kv_state(dt.sd, pos_name, dt.fk, dt.xk, case.nhead, k_pos)
    Ms, ks = R.kv_state(dt.sd, pos_name, dt.fk, dt.xk, case.nhead, k_pos, mm=R.split_mm)
    M32, k32 = state32(case, dt)
    gap = lambda a, b: float((a.double() - b).abs().max())      # noqa: E731
    return types.SimpleNamespace(M=M, ksum=ksum, yM32=gap(M32, M), yk32=gap(k32, ksum), yMsplit=gap(Ms, M),
                                 yksplit=gap(ks, ksum))


def bf_unit(case, prec):
    """does the launch run in the split-bf16 unit (attn_bf: a bf16 request and d <= 128)?"""
    return prec != "f32" and case.dims[2] <= 128


def state_bounds(ys, case, prec):
    """-> (bound on max|M - ref|, bound on max|ksum - ref|).  M: as the output's bounds, plus -- in the bf16 unit, where M
    is STORED as a bf16 hi / lo pair (16 significant bits) -- 2^-16 max|M| for the format.  ksum: a sum of Sk positive
    float32 terms in whatever order the kernel takes carries up to Sk 2^-24 ksum (the a-priori bound of recursive
    summation), which torch's pairwise float32 sum, the yardstick's, does not show -- so that term is added."""
    order = case.Sk * 2.0 ** -24 * float(ys.ksum.abs().max())
    if not bf_unit(case, prec):
        return 4.0 * ys.yM32, 4.0 * ys.yk32 + order
    return (2.0 * ys.yMsplit + 4.0 * ys.yM32 + 2.0 ** -16 * float(ys.M.abs().max()),
            2.0 * ys.yksplit + 4.0 * ys.yk32 + order)


def unpack_state(kv, d, bf):
    """plan.kv's per-cloud image (B, d d + d) -> (M (B, d, d), ksum (B, d)) in float64.  M is the A-operand image of the
    apply kernel's message product (csrc/attn_kernels_impl.h, attn_kv_fold_write): f32 -- 8-channel k-blocks, element
    (o, dd) at ((dd/8 d + o) 2 + dd%2) 4 + (dd%8)/2; bf16 unit -- bf16 hi / lo pairs in 16-channel steps, the hi of
    (o, dd) at unit 8 + jj with unit = ((dd/16 (d/32) + o/32) 2) 64 + hh 32 + o%32, hh = (dd%16 / 4) % 2,
    jj = dd%4 + 4 (dd%16 / 8), its lo 64 units further; ksum follows as d plain floats."""
    kv = kv.cpu()
    o, dd = torch.meshgrid(torch.arange(d), torch.arange(d), indexing="ij")
    ksum = kv[:, d * d:d * d + d].double()
    if not bf:
        slot = (((dd >> 3) * d + o) * 2 + (dd & 1)) * 4 + ((dd & 7) >> 1)
        return kv[:, :d * d][:, slot].double(), ksum
    img = kv[:, :d * d].contiguous().view(torch.bfloat16)
    kk = dd & 15
    hh, jj = (kk >> 2) & 1, (kk & 3) + ((kk >> 3) << 2)
    unit = (((dd >> 4) * (d >> 5) + (o >> 5)) * 2) * 64 + hh * 32 + (o & 31)
    return img[:, unit * 8 + jj].double() + img[:, (unit + 64) * 8 + jj].double(), ksum


def bound(y, case, prec):
    if prec == "f32" or case.dims[2] > 128:
        return 4.0 * y.y32
    return min(1e-4, 2.0 * y.ysplit + 4.0 * y.y32)


# ------------------------------------------------------------------------------- blocks and their forms --
_DUMMY = 64         # any address that is not NULL: the queries read pointers against NULL only


def host_plan(case, device="cpu"):
    """engine.AttnPlan of the row, built on the CPU as the modules' plan() calls build it on the device"""
    from pcr_amd import engine
    m, conv = build_module(case)
    pos_name, q_pos, k_pos, residual = FLAGS[case.kind]
    return engine.AttnPlan(m, pos_name, torch.device(device), case.nhead, q_pos=q_pos, k_pos=k_pos, residual=residual,
                           final=conv)


def host_blocks(plan, case, prec, splits=None, pooled=False):
    """-> (kv block, apply block): the parameter blocks AttnPlan.kv / .apply hand the library for the row, without a
    device -- AttnPlan._params on empty tensors with a dummy address in every pointer the call would fill, as
    AttnPlan.live_ok does.  splits: engine.KV_SPLITS (None: the library's suggestion)"""
    from pcr_amd import _lib, engine
    lib = _lib.load()
    e = torch.empty(0)
    nv = case.n_out if case.n_out is not None else case.B
    with engine.precision(prec):
        kv = plan._params(case.Bk or case.B, 1, case.Sk, e, e, e, e, e, e)
        ap = plan._params(nv, case.Lq, case.Sk, e, e if plan.q_pos else None, e, e, e, None if pooled else e)
    for p in (kv, ap):
        p.feat_q = p.feat_k = p.xyz_k = p.kv = _DUMMY
    kv.xyz_q = kv.out = ap.feat_k = ap.xyz_k = _DUMMY
    ap.xyz_q = _DUMMY if plan.q_pos else None
    ns = lib.pcr_attn_kv_splits(kv.B, case.Sk, plan.d) if splits is None else splits
    if ns > 1:
        kv.kv_splits, kv.kv_part = ns, _DUMMY
    if pooled:
        ap.pool_out = _DUMMY
    else:
        ap.out = _DUMMY
    return kv, ap


def reported(p, apply, live=None):
    """the kernel pcr_attn_launch_form names for a block, spelled as a trace spells it (attn_ref.kernel_name), and the
    arithmetic it would note; (None, None): the launch would be refused"""
    import ctypes
    from pcr_amd import _lib
    form = (ctypes.c_int * 16)(*([-1] * 16))
    status = _lib.load().pcr_attn_launch_form(ctypes.byref(p), live, int(apply), form)
    if status != 0:
        assert status == 1 and list(form) == [-1] * 16
        return None, None
    f = R.from_library(list(form), apply)
    return R.kernel_name(f), f[0]


class launched_blocks:
    """with launched_blocks() as seen: every parameter block AttnPlan.kv / .apply build inside is kept, seen["kv"] and
    seen["apply"] in launch order -- a wrapper around AttnPlan._params on the test's side; the engine's call path is as it was"""

    def __enter__(self):
        from pcr_amd import engine
        self.real = {k: getattr(engine.AttnPlan, k) for k in ("_params", "kv", "apply")}
        self.seen, side = {"kv": [], "apply": []}, []

        def params(plan, *a, **kw):
            p = self.real["_params"](plan, *a, **kw)
            if side:
                self.seen[side[-1]].append(p)
            return p

        def sided(name):
            def call(plan, *a, **kw):
                side.append(name)
                try:
                    return self.real[name](plan, *a, **kw)
                finally:
                    side.pop()
            return call
        engine.AttnPlan._params, engine.AttnPlan.kv, engine.AttnPlan.apply = params, sided("kv"), sided("apply")
        return self.seen

    def __exit__(self, *exc):
        from pcr_amd import engine
        for k, v in self.real.items():
            setattr(engine.AttnPlan, k, v)


def table_rows():
    """(table key, case, mode, splits, pooled) of every entry of EXPECT in both modes"""
    cases = dict(BY_NAME, **{c.name: c for c in SPLIT_CASES + list(MANY.values())})
    for key in EXPECT:
        name, _, what = key.partition("[")
        splits = int(what[7:-1]) if what.startswith("splits=") else None
        for prec in ("f32", "bf16x3"):
            yield key, cases[name], prec, splits, what == "pooled]"


def expect(name, prec, what=""):
    """the table's (kv kernel, apply kernel) of a row in a mode; what: "[splits=2]" | "[pooled]" """
    return EXPECT[name + what][0 if prec == "f32" else 1]


# ------------------------------------------------------------------------------------------ GPU side --
@functools.lru_cache(maxsize=None)
def _gpu_module(case):
    return build_module(case)[0].cuda()


def _dev(dt, rep=None):
    """device copies of a row's inputs; rep: cloud b of the launch is a copy of cloud rep[b]"""
    f = lambda t: (t if rep is None else t[rep]).contiguous().cuda()      # noqa: E731
    return f(dt.fq), f(dt.xq), f(dt.fk), f(dt.xk)


def _plan(case, m, dev_args):
    if case.kind == "cross":
        return m.plan(torch.device("cuda"))
    if case.kind == "fpq":
        from pcr_amd import engine
        pos_name, q_pos, k_pos, residual = FLAGS["fpq"]

        def build(dev):
            return engine.AttnPlan(m, pos_name, dev, case.nhead, q_pos=q_pos, k_pos=k_pos, residual=residual, final=m._final)
        return m._plan(torch.device("cuda"), build)
    with torch.no_grad():
        m(*(dev_args[:2] if case.kind == "self" else dev_args))           # (the module builds its plan on first use)
    return m._plan_obj


def run(case, m, dev_args, only=None, pooled=False):
    """the row's output through the shipped module (plan.kv / plan.apply for the indexed and pooled forms); only = b: the
    (virtual) cloud b alone"""
    fq, xq, fk, xk = dev_args
    with torch.no_grad():
        if case.indexed or pooled:
            plan = m.plan(torch.device("cuda"))
            n = case.n_out if case.n_out is not None else case.B
            qi = torch.tensor(case.q_index or tuple(range(n)), dtype=torch.int32).cuda()
            ki = torch.tensor(case.kv_index or tuple(range(n)), dtype=torch.int32).cuda()
            if only is not None:
                qi, ki, n = qi[only:only + 1].contiguous(), ki[only:only + 1].contiguous(), 1
            kv = plan.kv(fk, xk)
            return plan.apply(fq, None, kv, case.Sk, kv_index=ki, q_index=qi, n_out=n, pooled=pooled).cpu()
        s = slice(None) if only is None else slice(only, only + 1)
        if case.kind == "fpq":
            return _plan(case, m, dev_args).run(fq[s].contiguous(), xq[s].contiguous(), fk[s].contiguous(),
                                                xk[s].contiguous()).cpu()
        if case.kind == "self":
            return m(fq[s], xq[s]).cpu()
        return m(fq[s], xq[s], fk[s], xk[s]).cpu()


def kv_arith(case, m, dev_args):
    from pcr_amd import _lib
    plan = _plan(case, m, dev_args)
    plan.kv(dev_args[2], dev_args[3])
    return _lib.load().pcr_last_launch_arith()


def check_forms(seen, kv_seen, arith, want, splits=None):
    """the blocks a run launched (`seen`) and the block of the kv launch after which `arith` was read (`kv_seen`): the
    library reports the table's kernels for them, and the arithmetic it reports for the kv block is the one noted"""
    assert len(seen["kv"]) == 1 and len(seen["apply"]) == 1
    assert (reported(seen["kv"][0], 0)[0], reported(seen["apply"][0], 1)[0]) == want
    kernel, noted = reported(kv_seen["kv"][-1], 0)       # (kv_arith's own launch is the last one)
    assert kernel == want[0] and arith == noted, (kernel, arith, noted)
    if splits is not None:
        assert kv_seen["kv"][-1].kv_splits == splits


def check(case, prec, y, got, tag=""):
    err = float((got.double() - y.ref).abs().max())
    lim = bound(y, case, prec)
    print("ATTN_FORM %s%s %s err %.3e bound %.3e ratio %.3f y32 %.3e ysplit %.3e"
          % (case.name, tag, prec, err, lim, err / lim, y.y32, y.ysplit))
    assert torch.isfinite(got).all()
    assert err <= lim, (case.name, prec, err, lim)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_launch_form_against_float64(name, prec):
    from pcr_amd import engine
    case = BY_NAME[name]
    y = yardsticks(case)
    m = _gpu_module(case)
    args = _dev(y.data)
    nv = case.n_out if case.n_out is not None else case.B
    with engine.precision(prec):
        with launched_blocks() as seen:
            got = run(case, m, args)
        again = run(case, m, args)
        first, last = run(case, m, args, only=0), run(case, m, args, only=nv - 1)
        with launched_blocks() as kv_seen:
            arith = kv_arith(case, m, args)
    check(case, prec, y, got)
    assert torch.equal(got, again)                                      # fixed reduction orders
    assert torch.equal(first[0], got[0]) and torch.equal(last[0], got[nv - 1])
    check_forms(seen, kv_seen, arith, expect(name, prec))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_kv_state_against_float64(name, prec):
    """the key-side state itself, M and ksum, unpacked from the kv launch's image.  norm1 cancels any uniform scale of
    M Q', so a wrong mean over the key tokens (V / (Sk + 1)) never reaches the block's output beyond its eps; here it is
    a relative 1 / (Sk + 1) of M (tests/test_attn_ref_cpu.py, fault e)."""
    from pcr_amd import engine
    case = BY_NAME[name]
    y, ys = yardsticks(case), state_yardsticks(case)
    m = _gpu_module(case)
    args = _dev(y.data)
    with engine.precision(prec):
        plan = _plan(case, m, args)
        M, ksum = unpack_state(plan.kv(args[2], args[3]), case.dims[2], bf_unit(case, prec))
    eM, ek = float((M - ys.M).abs().max()), float((ksum - ys.ksum).abs().max())
    bM, bk = state_bounds(ys, case, prec)
    print("ATTN_STATE %s %s M err %.3e bound %.3e ratio %.3f | ksum err %.3e bound %.3e ratio %.3f"
          % (name, prec, eM, bM, eM / bM, ek, bk, ek / bk))
    assert eM <= bM and ek <= bk, (eM, bM, ek, bk)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TWIN_CASES)
def test_bf16_request_runs_the_split_unit(name):
    """the bf unit is split bf16 whatever was requested: "bf16" gives the bits of "bf16x3" """
    from pcr_amd import engine
    case = BY_NAME[name]
    y = yardsticks(case)
    m = _gpu_module(case)
    args = _dev(y.data)
    with engine.precision("bf16x3"):
        a = run(case, m, args)
    with engine.precision("bf16"):
        b = run(case, m, args)
    check(case, "bf16", y, b)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", POOL_CASES + ["cross-gallery-L33"])
def test_pooled_forms(name):
    """pooled output of the indexed forms (bf16x3, where pool_ok says yes): the maximum within the row's bound, the sum
    within Lq x the bound; the tile form (Lq = 33) and the f32 mode say they cannot pool"""
    from pcr_amd import engine
    case = BY_NAME[name]
    y = yardsticks(case)
    m = _gpu_module(case)
    args = _dev(y.data)
    plan = m.plan(torch.device("cuda"))
    with engine.precision("f32"):
        assert not plan.pool_ok(case.Lq, case.Sk)
    with engine.precision("bf16x3"):
        ok = plan.pool_ok(case.Lq, case.Sk)
        assert ok == (name in POOL_CASES)
        if not ok:
            return
        with launched_blocks() as seen:
            got = run(case, m, args, pooled=True)
        assert (reported(seen["kv"][0], 0)[0], reported(seen["apply"][0], 1)[0]) == expect(name, "bf16x3", "[pooled]")
        again = run(case, m, args, pooled=True)
        nv = case.n_out if case.n_out is not None else case.B
        first, last = run(case, m, args, only=0, pooled=True), run(case, m, args, only=nv - 1, pooled=True)
    lim = bound(y, case, "bf16x3")
    emax = float((got[:, 0].double() - y.ref.amax(dim=2)).abs().max())
    esum = float((got[:, 1].double() - y.ref.sum(dim=2)).abs().max())
    print("ATTN_FORM %s-pooled bf16x3 max err %.3e bound %.3e ratio %.3f | sum err %.3e bound %.3e ratio %.3f"
          % (name, emax, lim, emax / lim, esum, case.Lq * lim, esum / (case.Lq * lim)))
    assert got.shape == (nv, 2, 64)
    assert emax <= lim and esum <= case.Lq * lim, (emax, esum, lim)
    assert torch.equal(got, again)
    assert torch.equal(first[0], got[0]) and torch.equal(last[0], got[nv - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: c.name)
def test_token_split_is_held_to_the_same_bound(case, prec):
    """engine.KV_SPLITS = 2, 3: partial matrices + attn_kv_fold_kernel, the tile kv form (f32 projection) in both modes"""
    from pcr_amd import engine
    y = yardsticks(case)
    m = _gpu_module(case)
    args = _dev(y.data)
    prev = engine.KV_SPLITS
    try:
        with engine.precision(prec):
            for ns in (2, 3):
                engine.KV_SPLITS = ns
                with launched_blocks() as seen:
                    got = run(case, m, args)
                again = run(case, m, args)
                with launched_blocks() as kv_seen:
                    arith = kv_arith(case, m, args)
                check(case, prec, y, got, tag="[splits=%d]" % ns)
                assert torch.equal(got, again)
                check_forms(seen, kv_seen, arith, expect(case.name, prec, "[splits=%d]" % ns), splits=ns)
    finally:
        engine.KV_SPLITS = prev


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", SCALE_CASES)
def test_saturated_features(name, prec):
    """features x 16: elu saturates on both sides; the yardsticks are recomputed for these inputs"""
    from pcr_amd import engine
    case = BY_NAME[name]
    y = yardsticks(case, 16.0)
    m = _gpu_module(case)
    with engine.precision(prec):
        got = run(case, m, _dev(y.data))
    check(case, prec, y, got, tag="[x16]")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(MANY))
def test_more_work_than_workgroups(kind):
    """B = 8 CUs + 3 clouds of 32 tokens: the grid-stride loops of the persistent kernels at forms the benchmark batch
    does not reach (d = 32 self, pooled cross, FP with c1 = 3).  Cloud b is a copy of cloud b % 5: the first five are held
    to float64, every other cloud must give its source's bits."""
    from pcr_amd import engine
    case = MANY[kind]
    y = yardsticks(case)
    m = _gpu_module(case)
    B = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    rep = torch.arange(B) % 5
    args = _dev(y.data, rep)
    big = case._replace(B=B)
    with engine.precision("bf16x3"):
        with launched_blocks() as seen:
            got = run(big, m, args)
        assert (reported(seen["kv"][0], 0)[0], reported(seen["apply"][0], 1)[0]) == expect(case.name, "bf16x3")
        assert kv_arith(big, m, args) == ARITH["bf16x3"]
        with launched_blocks() as seen:
            pooled = run(big, m, args, pooled=True) if kind == "cross" else None
        assert kind != "cross" or reported(seen["apply"][0], 1)[0] == expect(case.name, "bf16x3", "[pooled]")[1]
    check(case, "bf16x3", y, got[:5], tag="[B=%d]" % B)
    assert torch.equal(got, got[:5][rep])
    if pooled is not None:
        lim = bound(y, case, "bf16x3")
        assert float((pooled[:5, 0].double() - y.ref.amax(dim=2)).abs().max()) <= lim
        assert float((pooled[:5, 1].double() - y.ref.sum(dim=2)).abs().max()) <= case.Lq * lim
        assert torch.equal(pooled, pooled[:5][rep])
        assert torch.equal(pooled[:, 0], got.amax(dim=2))
