"""GPU: every launch form of the per-point dense family (csrc/model_kernels.hip: pcr_dense_f32 / _xpm_f32 / _bmm_f32 / _gn_f32 /
_max_f32, pcr_dense_prec_f32 / _gn_prec_f32 / _xpm_prec_f32, pcr_groupnorm_f32) and of the EdgeConv and local-attention
launches (csrc/edge_kernels.hip: pcr_edge_max_f32, pcr_local_attn_f32) against the float64 restatements of
tests/dense_ref.py, one row per reachable kernel instantiation plus rows on the edges that are code paths of their own
(ragged last tile, partial cout window, 16-byte / scalar loads, B = 11 and B = 1).

Bounds.  err = max|got - ref| / max|ref|.  (1) Against the float64 restatement, per arithmetic the launch really runs:
2e-6 (f32), 2e-5 (bf16x3), 2e-2 (bf16) -- the bounds of test_gpu_dense_pm.py and the f32 / bf16x3 bounds of
test_gpu_sa_forms.py, none read off a kernel.  (2) Against the arithmetic of the unit (`dense_ref.dense_emul`: operands
split into bf16 hi / lo, round to nearest even, W_hi x_hi + W_hi x_lo + W_lo x_hi or W_hi x_hi, everything after the split
in float64): 8 y32e, y32e = the same emulated sum evaluated in torch float32 on the CPU against its float64 value.  The
f32 rows are held to 8 y32 (torch float32 of the plain sum) in the same way.  The factor 8 stands for the difference between
the matrix core's accumulation order and torch's blocked sums and is fixed, not fitted.  Both yardsticks are computed per
row on the CPU and printed beside the errors (`pytest -s`).  Check (2) makes the bf16x3 and bf16 rows as sharp as the f32
rows: tests/test_dense_ref_cpu.py plants its faults against ten times THAT bound.

Per dense row: (1), (2); (3) a second run bit-equal; (4) the first and the last cloud alone give the bits they give in the
batch; (5) pcr_last_launch_arith() names the unit `dense_ref.dispatch` names; (6) the output lies inside a larger buffer
filled with a NaN pattern: every output word is written and the words before and after it keep the pattern; (7) bit-equal
between forms where the code documents one k order (never instead of (1), (2)): dense_bf_pc_kernel against dense_bf_kernel
on the cloud cut by eight tokens, dense_rw_kernel against dense_kernel on the cloud cut to 100 tokens, both max forms
against the maximum of the stored layer; (8) engine.dense / rows.dense_gn -- the Python side of the choice -- give the bits
of the direct library call the restated dispatcher names; (9) where L % 4 == 0, the resident-weight and the bf16 kernels
give the same bits with x four bytes off a 16-byte boundary (their scalar load path; the two-role kernel then gives way
to dense_bf_kernel).  Edge rows: bit-equal to the float32 restatement in the
kernel's order ((m + tb) + shift, then the slope), (3), (4), (6), `out2` as a slice of a wider buffer with its own batch
stride.  Local-attention rows: within 2e-6 of the float64 restatement, (3), (4), (6).  Refusals raise and write nothing.
Inputs: dense_ref.dense_inputs / edge_inputs / local_inputs.

No row needed the 8 y32 allowance in place of 2e-6: cin = 1024 in the f32 unit came to 0.68 of 2e-6 at the most
(gn-f32-1024x256-L33-a0-g32, dense_kernel<2,true,true>).

FOUND.  No kernel fault: every row passed at its first run, the worst at 0.68 of bound (1) and 0.43 of bound (2).  What did
not hold was pcr_common.h's promise that every dispatcher notes the arithmetic it launches: of this family only
pcr_dense_xpm_prec_f32 did, so check (5) would have read the previous launch's note after any other dense call.
dense_launch and pcr_dense_max_f32 now note f32, dense_bf_launch the bf16 mode it was asked for, and engine.dense /
rows.dense_gn ask the library (`arith="lib"`) where they passed their own PRECISION string.  No kernel changed.
The dispatcher is the authority, and it moved one of the planned rows: dh = 32 at N = 257 with K = 48 does not run
local_attn_lds_kernel<32> -- the 32 x K index tile takes the head's tables past the 72 KB rule -- but local_attn_kernel<32>;
K = 7 and 20 at N = 257 stay resident.
NOT RUN, reached by no shape without a tuning variable: edge_max_lds_kernel<64> (PCR_EDGE_CS = 64).  PCR_DENSE_NO_RW /
_NO_CHUNK / _NO_PC, PCR_EDGE_NO_LDS and PCR_LOCAL_NO_LDS only send a shape to an instantiation that other shapes reach here.
GroupNorm inputs: channel 0 of x is +-1 by the token and its weights +-4 by the cout, so that no group of a token is nearly
constant -- where 1 / sqrt(var) multiplies the error of any arithmetic, the float64 evaluation of the split operands
included (without it bf16x3 at group size 4 stood at 4e-5 of scale against float64 on the CPU alone).

OBSERVED on an MI355X: 131 dense rows for 58 forms (the 40 dense_* kernel instantiations, dense_bf_kernel counted per KC,
with and without groupnorm_kernel behind them), 13 edge rows for 3 instantiations, 15 local-attention rows for 4; the file
ran in 4.2 s (160 tests).  profiles/r17a_dense_forms_kernels.txt: the kernels one kernel-trace run of this file saw (held to the row
tables by tests/test_dense_ref_cpu.py).  y32 was 3.9e-8 .. 5.5e-7, y32e 7.8e-8 .. 3.1e-7 of scale.  Worst err / bound (1),
then worst err / (8 y32 | 8 y32e), per form:
f32     rw<4,store> .09 .12   rw<8,store> .16 .12   rw<16,store> .24 .13   rw<4,max> .07 .14   rw<8,max> .12 .12   rw<16,max> .17 .12
        tile<1,plain> .45 .43   tile<2,plain> .25 .17   tile<1,gn> .24 .17   tile<2,gn> .14 .14   chunk<plain> .50 .43   chunk<gn> .68 .31
        max<> .21 .20   tile<2,plain> + groupnorm .27 .13
bf16x3  bf<plain,NR1,KC64> .23 .17   <plain,NR1,KC128> .19 .19   <plain,NR1,KC256> .25 .38   <plain,NR2,KC64> .22 .25   <plain,NR2,KC128> .20 .27
        <plain,NR2,KC256> .23 .43   bf<gn,NR1,KC64> .09 .16   <gn,NR1,KC128> .05 .17   <gn,NR1,KC256> .05 .15   <gn,NR2,KC64> .08 .13
        <gn,NR2,KC128> .09 .16   <gn,NR2,KC256> .05 .22   pc<plain,2> .28 .39   <plain,4> .27 .28   <plain,8> .21 .43   pc<gn,2> .06 .21
        <gn,4> .05 .17   <gn,8> .05 .24   pm<1> .23 .27   <2> .28 .28   <3> .23 .12   <4> .29 .27   bf<plain,NR1,KC64> + groupnorm .07 .12
bf16    bf<plain,NR1,KC64> .11 .09   <plain,NR1,KC128> .10 .11   <plain,NR1,KC256> .12 .25   <plain,NR2,KC64> .11 .12   <plain,NR2,KC128> .10 .18
        <plain,NR2,KC256> .11 .22   bf<gn,NR1,KC64> .05 .12   <gn,NR1,KC128> .03 .10   <gn,NR1,KC256> .02 .11   <gn,NR2,KC64> .04 .10
        <gn,NR2,KC128> .05 .10   <gn,NR2,KC256> .03 .13   pc<plain,2> .13 .17   <plain,4> .12 .16   <plain,8> .11 .27   pc<gn,2> .03 .12
        <gn,4> .02 .11   <gn,8> .03 .16   pm<1> .13 .17   <2> .12 .15   <3> .12 .07   <4> .13 .11   bf<plain,NR1,KC64> + groupnorm .06 .12
edge    all 13 rows bit-equal to the float32 restatement (4.3e-8 .. 8.8e-8 of scale from float64)
local   err / 2e-6: lds<32> .10   <32> .20   <16> .15   <0> .15 (y32 1.3e-7 .. 2.2e-7; err at most 2.3 y32)
"""
import types

import pytest
import torch

import dense_ref as R

pytestmark = pytest.mark.gpu

BOUNDS = {"f32": 2e-6, "bf16x3": 2e-5, "bf16": 2e-2}      # test_gpu_dense_pm.py; BOUNDS of test_gpu_sa_forms.py
YARD = 8.0                                                # x y32 / y32e (fixed, see above)
SENTINEL = 0x7FC0BEEF                                     # a quiet NaN no kernel produces
PAD = 256                                                 # words of sentinel kept before and after an output

# (entry, asked precision, B, cin, cout, L, x point-major, act | relu, GroupNorm groups, residual, unit + instantiation)
# entry: dense = engine.dense, gn = rows.dense_gn, bmm = pcr_dense_bmm_f32, max = pcr_dense_max_f32.
# tests/test_dense_ref_cpu.py recomputes the last column from dense_ref.dispatch and holds the table complete.
ROWS = [
    # ---- dense_rw_kernel<KB,MAXE>: cin 16..128, cout >= 128, L >= 128; L 128 (16-byte loads), 131 (scalar), 196 (ragged last tile)
    ('dense', 'f32', 3, 16, 128, 128, 0, 1, 0, 0, 'f32 rw<4,store>'),
    ('dense', 'f32', 3, 24, 160, 131, 0, 2, 0, 0, 'f32 rw<4,store>'),
    ('dense', 'f32', 3, 64, 288, 196, 0, 0, 0, 0, 'f32 rw<8,store>'),
    ('dense', 'f32', 3, 100, 128, 196, 0, 1, 0, 0, 'f32 rw<16,store>'),
    ('dense', 'f32', 3, 128, 160, 128, 0, 2, 0, 0, 'f32 rw<16,store>'),
    ('dense', 'f32', 11, 64, 128, 131, 0, 1, 0, 0, 'f32 rw<8,store>'),
    ('dense', 'f32', 1, 128, 288, 131, 0, 0, 0, 0, 'f32 rw<16,store>'),
    ('dense', 'bf16x3', 3, 24, 160, 131, 0, 2, 0, 0, 'f32 rw<4,store>'),
    ('dense', 'bf16', 3, 100, 128, 196, 0, 1, 0, 0, 'f32 rw<16,store>'),
    ('max', 'f32', 3, 16, 256, 128, 0, 1, 0, 0, 'f32 rw<4,max>'),
    ('max', 'f32', 3, 24, 256, 131, 0, 1, 0, 0, 'f32 rw<4,max>'),
    ('max', 'f32', 3, 64, 512, 196, 0, 1, 0, 0, 'f32 rw<8,max>'),
    ('max', 'f32', 3, 100, 256, 196, 0, 2, 0, 0, 'f32 rw<16,max>'),
    ('max', 'f32', 3, 128, 256, 131, 0, 1, 0, 0, 'f32 rw<16,max>'),
    ('max', 'f32', 11, 64, 256, 131, 0, 1, 0, 0, 'f32 rw<8,max>'),
    # ---- dense_kernel<TB,GN>: TB = 2 (cin <= 283, L > 32), TB = 1 (L <= 32, or cin > 283 with cout % 256 != 0); x_pm; bmm
    ('dense', 'f32', 3, 3, 64, 33, 0, 1, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 3, 20, 48, 50, 0, 2, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 3, 64, 72, 100, 0, 0, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 3, 256, 160, 64, 0, 1, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 11, 20, 48, 50, 0, 1, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 3, 64, 100, 50, 1, 2, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 3, 3, 64, 37, 1, 1, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'bf16x3', 3, 96, 64, 50, 1, 1, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'bf16x3', 3, 256, 160, 64, 1, 0, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'f32', 3, 64, 128, 32, 0, 1, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 3, 3, 64, 17, 0, 2, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 3, 20, 48, 1, 0, 0, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 3, 320, 160, 50, 0, 1, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 3, 1024, 160, 40, 0, 2, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 11, 320, 160, 50, 0, 0, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 3, 512, 256, 32, 0, 1, 0, 0, 'f32 tile<1,plain>'),
    ('dense', 'f32', 1, 3, 64, 33, 0, 1, 0, 0, 'f32 tile<2,plain>'),
    ('dense', 'bf16x3', 3, 320, 160, 50, 0, 1, 0, 0, 'bf16x3 bf<plain,NR2,KC64>'),
    ('bmm', 'f32', 3, 3, 3, 37, 0, 0, 0, 0, 'f32 tile<2,plain>'),
    ('bmm', 'f32', 3, 64, 64, 100, 0, 0, 0, 0, 'f32 tile<2,plain>'),
    ('bmm', 'f32', 3, 3, 3, 20, 0, 0, 0, 0, 'f32 tile<1,plain>'),
    ('bmm', 'f32', 11, 64, 64, 33, 0, 0, 0, 0, 'f32 tile<2,plain>'),
    # (GroupNorm group sizes 4 / 8 / 16 / 32, with and without residual and ReLU; cout 48 / 72: a partly filled 32-block)
    ('gn', 'f32', 3, 20, 64, 50, 0, 0, 16, 0, 'f32 tile<2,gn>'),
    ('gn', 'f32', 3, 20, 64, 50, 0, 1, 8, 1, 'f32 tile<2,gn>'),
    ('gn', 'f32', 3, 20, 64, 50, 0, 1, 4, 0, 'f32 tile<2,gn>'),
    ('gn', 'f32', 3, 20, 64, 50, 0, 0, 2, 1, 'f32 tile<2,gn>'),
    ('gn', 'f32', 3, 20, 48, 20, 0, 1, 6, 1, 'f32 tile<1,gn>'),
    ('gn', 'f32', 3, 320, 96, 50, 0, 0, 3, 1, 'f32 tile<1,gn>'),
    ('gn', 'f32', 3, 64, 72, 100, 0, 1, 9, 0, 'f32 tile<2,gn>'),
    ('gn', 'f32', 3, 128, 48, 40, 0, 0, 12, 1, 'f32 tile<2,gn>'),
    ('gn', 'f32', 11, 20, 64, 50, 0, 1, 8, 1, 'f32 tile<2,gn>'),
    ('gn', 'bf16x3', 3, 64, 72, 100, 0, 1, 9, 0, 'f32 tile<2,gn>'),
    # ---- dense_kernel<2,GN,CH>: cin 512 / 768 / 1024, cout % 256 == 0, L > 32
    ('dense', 'f32', 3, 512, 256, 33, 0, 1, 0, 0, 'f32 chunk<plain>'),
    ('dense', 'f32', 3, 768, 512, 64, 0, 2, 0, 0, 'f32 chunk<plain>'),
    ('dense', 'f32', 3, 1024, 256, 100, 0, 0, 0, 0, 'f32 chunk<plain>'),
    ('dense', 'f32', 11, 512, 256, 33, 0, 1, 0, 0, 'f32 chunk<plain>'),
    ('gn', 'f32', 3, 512, 512, 100, 0, 1, 16, 1, 'f32 chunk<gn>'),
    ('gn', 'f32', 3, 1024, 256, 33, 0, 0, 32, 0, 'f32 chunk<gn>'),
    ('gn', 'f32', 3, 768, 256, 64, 0, 0, 16, 1, 'f32 chunk<gn>'),
    # ---- dense_max_kernel
    ('max', 'f32', 3, 3, 256, 37, 0, 1, 0, 0, 'f32 max<>'),
    ('max', 'f32', 3, 200, 512, 130, 0, 1, 0, 0, 'f32 max<>'),
    ('max', 'f32', 11, 3, 256, 37, 0, 1, 0, 0, 'f32 max<>'),
    ('max', 'bf16x3', 3, 200, 512, 130, 0, 2, 0, 0, 'f32 max<>'),
    # ---- dense_bf_kernel<GN,NS,NR> at KC 64 / 128 / 256, bf16x3: L 64 (vector path), 66 (scalar), 100 (mixed)
    ('dense', 'bf16x3', 3, 64, 32, 64, 0, 1, 0, 0, 'bf16x3 bf<plain,NR1,KC64>'),
    ('dense', 'bf16x3', 3, 192, 160, 66, 0, 2, 0, 0, 'bf16x3 bf<plain,NR2,KC64>'),
    ('dense', 'bf16x3', 3, 128, 96, 100, 0, 0, 0, 0, 'bf16x3 bf<plain,NR1,KC128>'),
    ('dense', 'bf16x3', 3, 384, 288, 64, 0, 1, 0, 0, 'bf16x3 bf<plain,NR2,KC128>'),
    ('dense', 'bf16x3', 3, 256, 128, 128, 0, 2, 0, 0, 'bf16x3 bf<plain,NR1,KC256>'),
    ('dense', 'bf16x3', 3, 256, 160, 100, 0, 1, 0, 0, 'bf16x3 bf<plain,NR2,KC256>'),
    ('dense', 'bf16x3', 3, 512, 288, 66, 0, 0, 0, 0, 'bf16x3 bf<plain,NR2,KC256>'),
    ('dense', 'bf16x3', 3, 1024, 128, 100, 0, 1, 0, 0, 'bf16x3 bf<plain,NR1,KC256>'),
    ('dense', 'bf16x3', 11, 128, 96, 100, 0, 1, 0, 0, 'bf16x3 bf<plain,NR1,KC128>'),
    ('dense', 'bf16x3', 1, 64, 32, 64, 0, 2, 0, 0, 'bf16x3 bf<plain,NR1,KC64>'),
    ('gn', 'bf16x3', 3, 64, 96, 66, 0, 0, 24, 0, 'bf16x3 bf<gn,NR1,KC64>'),
    ('gn', 'bf16x3', 3, 192, 128, 100, 0, 1, 16, 1, 'bf16x3 bf<gn,NR1,KC64>'),
    ('gn', 'bf16x3', 3, 128, 160, 64, 0, 1, 10, 0, 'bf16x3 bf<gn,NR2,KC128>'),
    ('gn', 'bf16x3', 3, 384, 288, 100, 0, 0, 9, 1, 'bf16x3 bf<gn,NR2,KC128>'),
    ('gn', 'bf16x3', 3, 256, 96, 64, 0, 1, 3, 1, 'bf16x3 bf<gn,NR1,KC256>'),
    ('gn', 'bf16x3', 3, 768, 160, 66, 0, 0, 20, 1, 'bf16x3 bf<gn,NR2,KC256>'),
    ('gn', 'bf16x3', 11, 192, 128, 100, 0, 1, 16, 1, 'bf16x3 bf<gn,NR1,KC64>'),
    ('gn', 'bf16x3', 3, 192, 160, 66, 0, 1, 20, 0, 'bf16x3 bf<gn,NR2,KC64>'),
    ('gn', 'bf16x3', 3, 128, 96, 100, 0, 0, 6, 1, 'bf16x3 bf<gn,NR1,KC128>'),
    # ---- dense_bf_pc_kernel<GN,NS,NCH>, bf16x3: cin 256 / 512 / 1024, L % 128 == 0, cout > 128
    ('dense', 'bf16x3', 3, 256, 160, 128, 0, 1, 0, 0, 'bf16x3 pc<plain,2>'),
    ('dense', 'bf16x3', 3, 512, 288, 256, 0, 2, 0, 0, 'bf16x3 pc<plain,4>'),
    ('dense', 'bf16x3', 3, 1024, 512, 128, 0, 0, 0, 0, 'bf16x3 pc<plain,8>'),
    ('dense', 'bf16x3', 11, 256, 160, 128, 0, 1, 0, 0, 'bf16x3 pc<plain,2>'),
    ('gn', 'bf16x3', 3, 256, 288, 256, 0, 1, 9, 1, 'bf16x3 pc<gn,2>'),
    ('gn', 'bf16x3', 3, 512, 160, 128, 0, 1, 10, 1, 'bf16x3 pc<gn,4>'),
    ('gn', 'bf16x3', 3, 1024, 512, 128, 0, 0, 64, 1, 'bf16x3 pc<gn,8>'),
    ('gn', 'bf16x3', 11, 256, 288, 128, 0, 1, 36, 1, 'bf16x3 pc<gn,2>'),
    # ---- dense_pm_stream_kernel<NCB,LO>, bf16x3
    ('dense', 'bf16x3', 3, 64, 7, 32, 1, 1, 0, 0, 'bf16x3 pm<1>'),
    ('dense', 'bf16x3', 3, 256, 32, 33, 1, 0, 0, 0, 'bf16x3 pm<1>'),
    ('dense', 'bf16x3', 3, 64, 64, 50, 1, 2, 0, 0, 'bf16x3 pm<2>'),
    ('dense', 'bf16x3', 3, 256, 100, 33, 1, 1, 0, 0, 'bf16x3 pm<4>'),
    ('dense', 'bf16x3', 3, 64, 128, 50, 1, 0, 0, 0, 'bf16x3 pm<4>'),
    ('dense', 'bf16x3', 11, 256, 64, 50, 1, 1, 0, 0, 'bf16x3 pm<2>'),
    ('dense', 'bf16x3', 3, 64, 72, 50, 1, 1, 0, 0, 'bf16x3 pm<3>'),
    # ---- dense_bf_kernel<GN,NS,NR> at KC 64 / 128 / 256, bf16: L 64 (vector path), 66 (scalar), 100 (mixed)
    ('dense', 'bf16', 3, 64, 32, 64, 0, 1, 0, 0, 'bf16 bf<plain,NR1,KC64>'),
    ('dense', 'bf16', 3, 192, 160, 66, 0, 2, 0, 0, 'bf16 bf<plain,NR2,KC64>'),
    ('dense', 'bf16', 3, 128, 96, 100, 0, 0, 0, 0, 'bf16 bf<plain,NR1,KC128>'),
    ('dense', 'bf16', 3, 384, 288, 64, 0, 1, 0, 0, 'bf16 bf<plain,NR2,KC128>'),
    ('dense', 'bf16', 3, 256, 128, 128, 0, 2, 0, 0, 'bf16 bf<plain,NR1,KC256>'),
    ('dense', 'bf16', 3, 256, 160, 100, 0, 1, 0, 0, 'bf16 bf<plain,NR2,KC256>'),
    ('dense', 'bf16', 3, 512, 288, 66, 0, 0, 0, 0, 'bf16 bf<plain,NR2,KC256>'),
    ('dense', 'bf16', 3, 1024, 128, 100, 0, 1, 0, 0, 'bf16 bf<plain,NR1,KC256>'),
    ('dense', 'bf16', 11, 128, 96, 100, 0, 1, 0, 0, 'bf16 bf<plain,NR1,KC128>'),
    ('dense', 'bf16', 1, 64, 32, 64, 0, 2, 0, 0, 'bf16 bf<plain,NR1,KC64>'),
    ('gn', 'bf16', 3, 64, 96, 66, 0, 0, 24, 0, 'bf16 bf<gn,NR1,KC64>'),
    ('gn', 'bf16', 3, 192, 128, 100, 0, 1, 16, 1, 'bf16 bf<gn,NR1,KC64>'),
    ('gn', 'bf16', 3, 128, 160, 64, 0, 1, 10, 0, 'bf16 bf<gn,NR2,KC128>'),
    ('gn', 'bf16', 3, 384, 288, 100, 0, 0, 9, 1, 'bf16 bf<gn,NR2,KC128>'),
    ('gn', 'bf16', 3, 256, 96, 64, 0, 1, 3, 1, 'bf16 bf<gn,NR1,KC256>'),
    ('gn', 'bf16', 3, 768, 160, 66, 0, 0, 20, 1, 'bf16 bf<gn,NR2,KC256>'),
    ('gn', 'bf16', 11, 192, 128, 100, 0, 1, 16, 1, 'bf16 bf<gn,NR1,KC64>'),
    ('gn', 'bf16', 3, 192, 160, 66, 0, 1, 20, 0, 'bf16 bf<gn,NR2,KC64>'),
    ('gn', 'bf16', 3, 128, 96, 100, 0, 0, 6, 1, 'bf16 bf<gn,NR1,KC128>'),
    # ---- dense_bf_pc_kernel<GN,NS,NCH>, bf16: cin 256 / 512 / 1024, L % 128 == 0, cout > 128
    ('dense', 'bf16', 3, 256, 160, 128, 0, 1, 0, 0, 'bf16 pc<plain,2>'),
    ('dense', 'bf16', 3, 512, 288, 256, 0, 2, 0, 0, 'bf16 pc<plain,4>'),
    ('dense', 'bf16', 3, 1024, 512, 128, 0, 0, 0, 0, 'bf16 pc<plain,8>'),
    ('dense', 'bf16', 11, 256, 160, 128, 0, 1, 0, 0, 'bf16 pc<plain,2>'),
    ('gn', 'bf16', 3, 256, 288, 256, 0, 1, 9, 1, 'bf16 pc<gn,2>'),
    ('gn', 'bf16', 3, 512, 160, 128, 0, 1, 10, 1, 'bf16 pc<gn,4>'),
    ('gn', 'bf16', 3, 1024, 512, 128, 0, 0, 64, 1, 'bf16 pc<gn,8>'),
    ('gn', 'bf16', 11, 256, 288, 128, 0, 1, 36, 1, 'bf16 pc<gn,2>'),
    # ---- dense_pm_stream_kernel<NCB,LO>, bf16
    ('dense', 'bf16', 3, 64, 7, 32, 1, 1, 0, 0, 'bf16 pm<1>'),
    ('dense', 'bf16', 3, 256, 32, 33, 1, 0, 0, 0, 'bf16 pm<1>'),
    ('dense', 'bf16', 3, 64, 64, 50, 1, 2, 0, 0, 'bf16 pm<2>'),
    ('dense', 'bf16', 3, 256, 100, 33, 1, 1, 0, 0, 'bf16 pm<4>'),
    ('dense', 'bf16', 3, 64, 128, 50, 1, 0, 0, 0, 'bf16 pm<4>'),
    ('dense', 'bf16', 11, 256, 64, 50, 1, 1, 0, 0, 'bf16 pm<2>'),
    ('dense', 'bf16', 3, 64, 72, 50, 1, 1, 0, 0, 'bf16 pm<3>'),
    # ---- groupnorm_kernel behind the launch rows.dense_gn falls back to: group sizes 2 and 64, one group
    ('gn', 'f32', 3, 20, 64, 50, 0, 1, 32, 1, 'f32 tile<2,plain> + groupnorm'),
    ('gn', 'bf16x3', 3, 64, 128, 100, 0, 0, 2, 1, 'bf16x3 bf<plain,NR1,KC64> + groupnorm'),
    ('gn', 'f32', 3, 128, 48, 40, 0, 1, 1, 0, 'f32 tile<2,plain> + groupnorm'),
    ('gn', 'bf16', 3, 64, 128, 100, 0, 1, 2, 0, 'bf16 bf<plain,NR1,KC64> + groupnorm'),
    ('gn', 'f32', 11, 20, 64, 50, 0, 0, 32, 1, 'f32 tile<2,plain> + groupnorm'),
]

# (B, N, Co, K, out2 as a slice of a wider buffer, instantiation): pcr_edge_max_f32
EDGE_ROWS = [
    (3, 33, 40, 3, 0, 'edge lds<32>'),
    (3, 128, 64, 20, 1, 'edge lds<32>'),
    (3, 100, 1, 1, 0, 'edge lds<32>'),
    (11, 33, 64, 20, 0, 'edge lds<32>'),
    (3, 129, 1, 1, 0, 'edge lds<16>'),
    (3, 512, 256, 64, 0, 'edge lds<16>'),
    (3, 300, 40, 3, 1, 'edge lds<16>'),
    (11, 129, 40, 3, 0, 'edge lds<16>'),
    (3, 513, 40, 3, 1, 'edge gather'),
    (3, 600, 64, 20, 0, 'edge gather'),
    (3, 513, 1, 20, 0, 'edge gather'),
    (1, 600, 256, 64, 0, 'edge gather'),
    (11, 513, 40, 1, 0, 'edge gather'),
]

# (B, N, C, K, nhead, instantiation): pcr_local_attn_f32
LOCAL_ROWS = [
    (3, 64, 64, 20, 2, 'local lds<32>'),
    (3, 257, 64, 7, 2, 'local lds<32>'),
    (3, 257, 32, 20, 1, 'local lds<32>'),
    (11, 64, 64, 7, 2, 'local lds<32>'),
    (3, 257, 64, 48, 2, 'local<32>'),            # (the K = 48 index tile takes the head's tables past 72 KB)
    (3, 600, 64, 48, 2, 'local<32>'),
    (11, 300, 32, 7, 1, 'local<32>'),
    (3, 100, 32, 7, 2, 'local<16>'),
    (3, 257, 64, 20, 4, 'local<16>'),
    (3, 70, 48, 20, 3, 'local<16>'),
    (11, 100, 32, 20, 2, 'local<16>'),
    (3, 70, 16, 7, 2, 'local<0>'),
    (3, 70, 64, 20, 1, 'local<0>'),
    (3, 45, 16, 48, 4, 'local<0>'),
    (11, 70, 16, 7, 2, 'local<0>'),
]


def row_id(row):
    entry, prec, B, cin, cout, L, x_pm, act, groups, res, _ = row
    return "%s-%s-%dx%d-L%d%s%s%s%s%s" % (entry, prec, cin, cout, L, "-pm" if x_pm else "", "-a%d" % act,
                                         "-g%d" % groups if groups else "", "-res" if res else "", "-B%d" % B if B != 3 else "")


def row_bound(row):
    """the bound of the arithmetic the row really runs in"""
    return BOUNDS[row[10].split(" ")[0]]


def row_inputs(row):
    return R.dense_inputs(*row[:1], *row[2:10])


def row_yardsticks(row, d):
    """(float64 restatement, what check (2) compares with, its float32 yardstick): the emulated arithmetic of the unit for
    a bf16 row, the restatement itself for an f32 row"""
    ref = R.dense_row_eval(row, d)
    if R.unit_of(row[10]) == 0:
        return ref, ref, R.rel_err(R.dense_row_eval(row, d, "y32"), ref)
    emul = R.dense_row_eval(row, d, "emul")
    return ref, emul, R.rel_err(R.dense_row_eval(row, d, "emul32"), emul)


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def _guarded(n):
    """an output of n words inside a buffer that holds the sentinel before, in and after it"""
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf.view(torch.float32)[PAD:PAD + n]


def _confinement(buf, what, fails):
    n = buf.numel() - 2 * PAD
    if bool((buf[:PAD] != SENTINEL).any()) or bool((buf[PAD + n:] != SENTINEL).any()):
        fails.append("%s: words outside the output were written" % what)
    left = int((buf[PAD:PAD + n] == SENTINEL).sum())
    if left:
        fails.append("%s: %d of %d output words were never written" % (what, left, n))


_weights = {}


def _packed(row, d):
    from pcr_amd import engine as E
    key = row[:1] + row[2:10]
    if key not in _weights:
        wp = E.pack_weight_dual(d["w"], torch.device("cuda"))
        assert (getattr(wp, "_pcr_bf", None) is not None) == R.has_bf_image(row[3], row[4])
        _weights[key] = wp
    return _weights[key]


def _dev(d):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _run(row, t, wp, sl=slice(None), Lc=None, entry=None, misalign=False):
    """the library call `dense_ref.dispatch` names for the row (cut to the clouds `sl` and the first Lc tokens; misalign: x
    four bytes past a 16-byte boundary), its output inside a guarded buffer -> (buffer, output, pcr_last_launch_arith(),
    instantiation)"""
    from pcr_amd import _lib as Lb
    lib = Lb.load()
    _, prec, B, cin, cout, L, x_pm, act, groups, res, _ = row
    entry = entry or row[0]
    x = t["x"][sl]
    r = t.get("res")
    r = None if r is None else r[sl]
    if Lc is not None:
        x = x[:, :Lc] if x_pm else x[:, :, :Lc]
        r = None if r is None else r[:, :, :Lc]
    x = x.contiguous()
    r = None if r is None else r.contiguous()
    if misalign:
        off = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(x.shape)
        x = off.copy_(x)
        assert x.is_contiguous() and x.data_ptr() % 16 == 4
    b, l = x.shape[0], (L if Lc is None else Lc)
    name = R.dispatch(entry, b, cin, cout, l, R.PREC[prec] if entry in ("dense", "gn") else 0, x_pm, cout // groups if groups else 0)
    assert name != "refused", row
    unit = R.unit_of(name)
    buf, y = _guarded(cout * b if entry == "max" else b * cout * l)
    st = Lb.stream_ptr()
    bf = getattr(wp, "_pcr_bf", None)
    sc, sh = t.get("scale"), t.get("shift")
    if entry == "bmm":
        img = torch.empty((b, lib.pcr_packed_weight_floats(cin, cin)), dtype=torch.float32, device="cuda")
        Lb.run.pcr_pack_bmm_f32(R.bmm_table(t["t"][sl]).contiguous(), img, b, cin, st)
        Lb.run.pcr_dense_bmm_f32(x, img, y, b, cin, cout, l, st)
    elif entry == "max":
        Lb.run.pcr_dense_max_f32(x, wp, sc, sh, y, b, cin, cout, l, act, st)
    elif entry == "gn":
        if name.endswith("+ groupnorm"):
            mid = torch.empty((b, cout, l), dtype=torch.float32, device="cuda")
            if unit:
                Lb.run.pcr_dense_prec_f32(x, bf, None, None, mid, b, cin, cout, l, 0, unit, st)
            else:
                Lb.run.pcr_dense_f32(x, wp, None, None, mid, b, cin, cout, l, 0, st)
            Lb.run.pcr_groupnorm_f32(mid, t["gamma"], t["beta"], r, y, b, cout, l, groups, act, st)
        elif unit:
            Lb.run.pcr_dense_gn_prec_f32(x, bf, t["gamma"], t["beta"], r, y, b, cin, cout, l, groups, act, unit, st)
        else:
            Lb.run.pcr_dense_gn_f32(x, wp, t["gamma"], t["beta"], r, y, b, cin, cout, l, groups, act, st)
    elif " pm<" in name:
        Lb.run.pcr_dense_xpm_prec_f32(x, bf, sc, sh, y, b, cin, cout, l, act, unit, st)
    elif unit:
        Lb.run.pcr_dense_prec_f32(x, bf, sc, sh, y, b, cin, cout, l, act, unit, st)
    else:
        (Lb.run.pcr_dense_xpm_f32 if x_pm else Lb.run.pcr_dense_f32)(x, wp, sc, sh, y, b, cin, cout, l, act, st)
    arith = lib.pcr_last_launch_arith()
    return buf, y.view((cout, b) if entry == "max" else (b, cout, l)), arith, name


def _through_python(row, t, wp):
    """the same call through engine.dense / rows.dense_gn, which choose the unit themselves"""
    from pcr_amd import _lib as Lb
    from pcr_amd import engine as E
    from pcr_amd import rows
    entry, prec, B, cin, cout, L, x_pm, act, groups, res, _ = row
    with E.precision(prec), torch.no_grad():
        if entry == "dense":
            out = E.dense(t["x"].transpose(1, 2) if x_pm else t["x"], wp, cout, t["scale"], t["shift"], act)
        else:
            gn = types.SimpleNamespace(num_groups=groups, weight=t["gamma"], bias=t["beta"], eps=1e-5)
            out = rows.dense_gn(t["x"], wp, cout, gn, res=t["res"], relu=bool(act))
        return out, Lb.load().pcr_last_launch_arith()


@pytest.mark.parametrize("row", ROWS, ids=[row_id(r) for r in ROWS])
def test_dense_form_against_float64(row):
    entry, prec, B, cin, cout, L, x_pm, act, groups, res, expect = row
    d = row_inputs(row)
    ref, sharp, yard = row_yardsticks(row, d)
    t = _dev(d)
    wp = None if entry == "bmm" else _packed(row, d)
    fails = []
    buf, got, arith, name = _run(row, t, wp)
    torch.cuda.synchronize()
    _confinement(buf, "output", fails)
    _, again, _, _ = _run(row, t, wp)
    bound = row_bound(row)
    err, err2 = R.rel_err(got.cpu(), ref), R.rel_err(got.cpu(), sharp)
    print("DENSEFORM %s | %s | err %.3g = %.3f of the bound %.0e | against the unit's arithmetic %.3g = %.3f of %g x %.3g" % (
        row_id(row), expect, err, err / bound, bound, err2, err2 / (YARD * yard), YARD, yard))
    if name != expect:
        fails.append("the restated dispatcher says %s" % name)
    if arith != R.unit_of(expect):
        fails.append("ran in arithmetic %d, the dispatcher's rule says %s" % (arith, expect))
    if not torch.isfinite(got).all():
        fails.append("not finite")
    if not err <= bound:
        fails.append("err %.3g of scale > bound %.3g" % (err, bound))
    if not err2 <= YARD * yard:
        fails.append("err %.3g against the unit's arithmetic > %g x %.3g (torch float32 of the same sum)" % (err2, YARD, yard))
    if not torch.equal(got, again):
        fails.append("two launches differ")
    for b in (0, B - 1):
        _, alone, _, _ = _run(row, t, wp, sl=slice(b, b + 1))
        if not torch.equal(alone[:, 0] if entry == "max" else alone[0], got[:, b] if entry == "max" else got[b]):
            fails.append("cloud %d alone differs from the cloud in its batch" % b)
    # (7) forms that document one k order
    if " pc<" in expect or (" rw<" in expect and entry != "max"):
        Lc = L - 8 if " pc<" in expect else 100
        cbuf, cut, carith, cname = _run(row, t, wp, Lc=Lc)
        _confinement(cbuf, "cut cloud", fails)
        assert (" bf<" if " pc<" in expect else " tile<") in cname and carith == arith, cname
        if not torch.equal(cut, got[:, :, :Lc]):
            fails.append("%s and %s differ on the first %d tokens" % (expect, cname, Lc))
    # (9) x off its 16-byte boundary: the resident-weight and the bf16 tile kernels take their scalar load path, the two-role
    # kernel is not chosen and dense_bf_kernel runs -- every one documented to the same k order, so the same bits
    if L % 4 == 0 and "+" not in expect and any(f in expect for f in (" rw<", " bf<", " pc<")):
        mbuf, mis, marith, _ = _run(row, t, wp, misalign=True)
        _confinement(mbuf, "unaligned x", fails)
        if marith != arith or not torch.equal(mis, got):
            fails.append("x four bytes off a 16-byte boundary gives other bits (arithmetic %d)" % marith)
    if entry == "max":
        _, stored, _, sname = _run(row, t, wp, entry="f32")
        if not torch.equal(stored.max(dim=2)[0].t(), got):
            fails.append("differs from the maximum of the stored layer (%s)" % sname)
    # (8) the Python side of the choice
    if entry in ("dense", "gn"):
        out, arith_p = _through_python(row, t, wp)
        if arith_p != R.unit_of(expect) or not torch.equal(out, got):
            fails.append("engine / rows ran arithmetic %d and %s the bits of %s" % (
                arith_p, "gave" if torch.equal(out, got) else "did not give", expect))
    assert not fails, "; ".join(fails)


def edge_id(row):
    return "N%d-Co%d-K%d%s%s" % (row[1], row[2], row[3], "-out2" if row[4] else "", "-B%d" % row[0] if row[0] != 3 else "")


@pytest.mark.parametrize("row", EDGE_ROWS, ids=[edge_id(r) for r in EDGE_ROWS])
def test_edge_max_form_is_the_float32_restatement_bit_for_bit(row):
    from pcr_amd import _lib as Lb
    B, N, Co, K, with_out2, expect = row
    assert R.edge_dispatch(N, Co, K, B) == expect
    ta, tb, idx, shift = R.edge_inputs(B, N, Co, K)
    want = R.edge_max_ref(ta, tb, idx, shift, 0.2, torch.float32)
    ref = R.edge_max_ref(ta, tb, idx, shift)
    t = [v.cuda() for v in (ta, tb, idx, shift)]
    Ct, off = Co + 24, 8          # out2: channels off .. off + Co of a (B,Ct,N) buffer

    def run(sl=slice(None)):
        a, b_, i = (v[sl].contiguous() for v in t[:3])
        nb = a.shape[0]
        buf, out = _guarded(nb * Co * N)
        wbuf, w = _guarded(nb * Ct * N)
        out2 = w.data_ptr() + 4 * off * N if with_out2 else None
        Lb.run.pcr_edge_max_f32(a, b_, i, t[3], 0.2, out, 0, out2, Ct * N, nb, N, Co, K, Lb.stream_ptr())
        return buf, out.view(nb, Co, N), wbuf, wbuf[PAD:PAD + nb * Ct * N].view(nb, Ct, N)

    fails = []
    buf, got, wbuf, wide = run()
    _confinement(buf, "out", fails)
    _, again, _, _ = run()
    print("EDGEFORM %s | %s | err against float64 %.3g" % (edge_id(row), expect, R.rel_err(got.cpu(), ref)))
    if not torch.equal(got.cpu(), want):
        fails.append("differs from the float32 restatement: %.3g of scale" % R.rel_err(got.cpu(), want))
    if not torch.equal(got, again):
        fails.append("two launches differ")
    for b in (0, B - 1):
        if not torch.equal(run(slice(b, b + 1))[1][0], got[b]):
            fails.append("cloud %d alone differs from the cloud in its batch" % b)
    inside = wide[:, off:off + Co].contiguous().view(torch.float32)
    rest = torch.cat([wide[:, :off].reshape(-1), wide[:, off + Co:].reshape(-1), wbuf[:PAD], wbuf[-PAD:]])
    if bool((rest != SENTINEL).any()):
        fails.append("out2: words outside the slice were written")
    if with_out2 and not torch.equal(inside, got):
        fails.append("out2 differs from out")
    if not with_out2 and bool((wide != SENTINEL).any()):
        fails.append("out2 = NULL was written")
    assert not fails, "; ".join(fails)


def local_id(row):
    return "N%d-C%d-K%d-h%d%s" % (row[1], row[2], row[3], row[4], "-B%d" % row[0] if row[0] != 3 else "")


@pytest.mark.parametrize("row", LOCAL_ROWS, ids=[local_id(r) for r in LOCAL_ROWS])
def test_local_attn_form_against_float64(row):
    from pcr_amd import _lib as Lb
    B, N, C, K, nhead, expect = row
    assert R.local_dispatch(N, C, K, nhead, B) == expect
    qkv, idx = R.local_inputs(B, N, C, K)
    ref = R.local_attn_ref(qkv, idx, nhead, 1e-6)
    y32 = R.rel_err(R.local_attn_ref(qkv, idx, nhead, 1e-6, torch.float32), ref)
    q_d, i_d = qkv.cuda(), idx.cuda()

    def run(sl=slice(None)):
        q, i = q_d[sl].contiguous(), i_d[sl].contiguous()
        buf, msg = _guarded(q.shape[0] * C * N)
        Lb.run.pcr_local_attn_f32(q, i, msg, q.shape[0], N, C, K, nhead, 1e-6, Lb.stream_ptr())
        return buf, msg.view(q.shape[0], C, N)

    fails = []
    buf, got = run()
    _confinement(buf, "msg", fails)
    err = R.rel_err(got.cpu(), ref)
    print("LOCALFORM %s | %s | err %.3g = %.3f of the bound %.0e, %.2f y32 (y32 %.3g)" % (
        local_id(row), expect, err, err / BOUNDS["f32"], BOUNDS["f32"], err / y32, y32))
    if not err <= BOUNDS["f32"]:
        fails.append("err %.3g of scale > bound %.3g (float32 torch: %.3g)" % (err, BOUNDS["f32"], y32))
    if not torch.equal(got, run()[1]):
        fails.append("two launches differ")
    for b in (0, B - 1):
        if not torch.equal(run(slice(b, b + 1))[1][0], got[b]):
            fails.append("cloud %d alone differs from the cloud in its batch" % b)
    assert not fails, "; ".join(fails)


def test_shapes_the_dispatchers_must_refuse_raise_and_write_nothing():
    from pcr_amd import _lib as Lb
    from pcr_amd import engine as E
    st = Lb.stream_ptr()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    # f32: cin 1536 with cout 100 -- no chunked form (cout % 256), and 1536 x 33 floats are beyond the LDS limit
    B, cin, cout, L = 2, 1536, 100, 40
    assert R.dispatch("dense", B, cin, cout, L) == "refused" and R.dispatch("dense", B, cin, 256, L) == "f32 chunk<plain>"
    x = torch.randn(B, cin, L, generator=g).cuda()
    wp = E.pack_weight(torch.randn(cout, cin, generator=g), dev)
    buf, y = _guarded(B * cout * L)
    with pytest.raises(Lb.PcrError):
        Lb.run.pcr_dense_f32(x, wp, None, None, y, B, cin, cout, L, 0, st)
    with pytest.raises(Lb.PcrError):
        E.dense(x, wp, cout)
    # the point-major bf16 form: the weight image of cin 2048 x cout 128 is beyond LDS
    cin, cout = 2048, 128
    assert R.dispatch("xpm_prec", B, cin, cout, L, 1) == "refused" and not R.xpm_prec_ok(cin, cout, L)
    xp = torch.randn(B, L, cin, generator=g).cuda()
    wbf = E.pack_weight_bf(torch.randn(cout, cin, generator=g), dev)
    buf2, y2 = _guarded(B * cout * L)
    for prec in (1, 2):
        with pytest.raises(Lb.PcrError):
            Lb.run.pcr_dense_xpm_prec_f32(xp, wbf, None, None, y2, B, cin, cout, L, 0, prec, st)
    # more clouds than a grid dimension holds
    B = 65536
    assert R.dispatch("dense", B, 3, 32, 1) == "refused" and R.dispatch("max", B, 3, 256, 1) == "refused"
    xb = torch.zeros(B, 3, 1, device="cuda")
    w3 = E.pack_weight(torch.randn(32, 3, generator=g), dev)
    buf3, y3 = _guarded(B * 32)
    with pytest.raises(Lb.PcrError):
        Lb.run.pcr_dense_f32(xb, w3, None, None, y3, B, 3, 32, 1, 0, st)
    torch.cuda.synchronize()
    for b in (buf, buf2, buf3):
        assert bool((b == SENTINEL).all())
