"""GPU: every launch form of the inference set-abstraction layer (pcr_sa_mlp_f32 through engine.SaPlan.run) against the
float64 restatement of tests/sa_ref.py, one row per reachable kernel instantiation, in the three arithmetic modes.

Bounds.  err = max|got - sa_ref| over the output / max|sa_ref|; per arithmetic 2e-6 (f32), 2e-5 (bf16x3), 3e-2 (bf16):
the project's own, from test_gpu_precision.py::test_sa_layer_in_every_precision_against_torch and BOUND of
test_gpu_sa_krow_items.py -- none read off a kernel, none widened here (no row came closer than 0.53 of its bound).  A row
is held to the bound of the arithmetic it really runs in (`row_bound`).  y32 = max|sa_ref32 - sa_ref| / scale, torch's
unfused float32 ops on the same inputs, is computed per row on the CPU and printed beside err (`pytest -s`: err / bound,
err / y32); it was 1.0e-7 .. 5.7e-7.  The bf16 bound separates structural faults only weakly -- leaving a group's last row
out moves the result by 0.038 of its scale at the weakest row, the bound is 0.03 -- but the bf16 unit is the bf16x3
unit's template with another operand image, and the bf16x3 rows (bound 2e-5, every planted fault of
tests/test_sa_ref_cpu.py at least ten times that) carry that weight.

Per row: (1) err within the bound; (2) a second run bit-equal; (3) point-major output bit-equal to channel-major; (4) the
first and the last cloud alone give the bits they give in the batch; (5) pcr_last_launch_arith() names the unit the
restated dispatcher (sa_ref.dispatch) names; (6) on rows with hit counts, the K-row evaluation of the same call (cnt
withheld) is within ITS bound too, and bit-equal to the ragged one wherever both ran in one arithmetic -- 152 of the 212
such rows, all 152 bit-equal: every sa_rag_kernel form against its sa_fused_kernel twin in all three units, the stream
forms against each other, the cout-split kernel against itself.  The other 60 are rows of the bf16 units whose K-row twin
runs in f32 by rule (K = 20 and 1 are no multiple of 16; 64/128/256 and 32/64/64 have no layer 1 on the matrix core);
(7) a launch fed the ball query's row table gives the bits of the launch fed the index tensor.
Inputs: `row_inputs` -- a group's genuine entries are distinct points and its first and last genuine rows each own a
channel's maximum, so a dropped or leaked boundary row is seen.

Shapes: B = 3 (one row per family B = 11), S = 2 cpw + 1 for the K-row tile kernel (a partial last workgroup; cpw + 3
where that passes 131), two tiles / items and one centre for the others, N = max(64, K + 8, S), D = 8 in mode 0 (prefix
centres), D = 5 in mode 1 (given centres; cin % 8 != 0).  One D = 0 row per form in every unit that holds it -- no
layer-1 table is a code path of its own in each kernel (`hasp` / `pref` in sa_rag_kernel, `tab.on` in the stream forms,
the reset of `acc1` in the cout-split kernel); a K-row tile form counts without its TB and epilogue flag -- and one
B = 11 row per kernel family and unit: both held by tests/test_sa_ref_cpu.py.

FOUND.  64 / 64 / c3 with 129 <= c3 <= 256 and K % 16 == 0 in a bf16 mode: the K-row fan-out (then sa2_launch_tb) sent the class (2 ways, 1 way) to
sa_fused_kernel<TB,1,2,1> whatever the number of cout-block rounds, and with NR = 1, W3 = 1 wave w computes cout block w
only.  Channels 128 and up of layer 3 were never computed and their maxima read from LDS nobody wrote: before the fix the
eight rows 64_64_160 / 64_64_256 at K = 16 / 48 (bf16x3 and bf16) failed with err 1.4 .. 3.1 of the scale (70 000 ..
153 000 bounds in bf16x3), two launches differing.  The bf16 units now refuse the class when nr != 1 and the layer runs
in the f32 unit's <TB,2,0,0,1>: the same rows pass at 0.19 / 0.20 of the bound, pcr_last_launch_arith() = f32.  No shipped
model has that layer.  Every other row passed unchanged.

The dispatcher is the authority, and it moved three of the issue's rows.  32 / 32 / 64 never reaches a bf16 unit: its
classes are (4 ways, 2 ways), which sa_tile_shape_ok (ragged) and the K-row class rule refuse BEFORE the stream forms are
looked at -- ragged it runs the f32 unit's sa_rag_kernel<4,1,0,0,1,0>, K-row sa_fused_kernel<TB,1,0,0> (so this one
ball-query shape evaluates ragged and K-row in one arithmetic only because both fall back).  64 / 64 / 128 at K = 96 does
not fit the index form's LDS and runs sa_rag_kernel<4,1,2,1,1,0>.  The 8-wave TABLE form is chosen only where twelve
waves' areas do not fit, and no shape that reads the table is that large.
NOT RUN, reached by no shape without a tuning variable: sa_stream_kernel<1,2,*>, sa_stream_rag_kernel<1,2,*,*,*> (above);
sa_stream_rag_kernel<*,*,*,true,8> (PCR_SA_NO_W12 only); (TB, form) pairs the LDS / register rule never picks (e.g.
<5..6,2,1,1>, <1..2,1,4,4>), which test_sa_ref_cpu.py shows by enumerating K = 1 .. 192.

Instantiation -> rows: the last column of ROWS (held to sa_ref.dispatch by tests/test_sa_ref_cpu.py, and to the kernel
names of a kernel-trace run of this file, profiles/r16a_sa_forms_kernels.txt).  OBSERVED worst err / bound per
instantiation on an MI355X (436 rows, 185 instantiations; the file ran in 4.4 s).  Largest: 0.30 in the f32 unit
(m1-D0-128_256_256-K1), 0.53 in bf16x3 (m0-D8-96_96_96-K32-B11), 0.20 in bf16 (m0-D0-32_32_32-K32).
sa_fused_kernel, f32 unit, `full` (K % 16 != 0) then `maxe`, TB ascending over the TBs the cost model reaches:
  <TB,1,4,4,1,4> 32/32/32     TB 3-6: .08 .07 .10 .07 | .12 .09 .10 .07     <TB,1,4,4> 64/32/32  .10 .08 .10 .08 | .12 .08 .13 .11
  <TB,1,2,2> 64/64/64       TB 2,4,5,6: .21 .20 .08 .12 | .11 .12 .16 .16
  <TB,1,1,1> 128/128/128 (+72/100/120)  TB 1-6: .18 .14 .19 .15 .22 .16 | .15 .19 .17 .15 .20 .17
  <TB,2,1,1,1> 128/128/256 (+128/128/192)  TB 1-5: .16 .20 .13 .15 .11 | .18 .19 .15 .13 .15
  <TB,2,1,1> 128/256/256     TB 1-4: .30 .20 .21 .18 | .17 .14 .21 .14
  <TB,1,0,0> 32/64/128 (+24/40/72, 32/32/64)  TB 2-6: .13 .13 .12 .13 .10 | TB 2-6: .11 .23 .12 .10 .11
  <TB,2,0,0,1> 64/64/256 (+64/64/160)  TB 2-6: .14 .09 .14 .12 .11 | TB 2,4,5,6: .19 .11 .12 .20
  <TB,2,0,0> 64/256/64       TB 2-4: .19 .16 .19 | .20 .26 .27        <TB,4,1,1,4> 128/256/512, 64/64/512  TB 1-2: .23 .27 | .23 .22
sa_fused_kernel, bf16x3 | bf16 unit (maxe only):
  <TB,1,4,4> 32/32/32 TB 3-6: .52 .37 .29 .40 | .13 .10 .14 .10      <TB,1,2,2> 64/64/64 TB 4-6: .40 .37 .26 | .13 .16 .13
  <TB,1,2,1> 64/64/96 TB 2,4,5,6: .31 .27 .20 .22 | .10 .09 .12 .10
  <TB,1,1,1> 96/96/96 TB 1-6: .53 .41 .32 .44 .46 .36 | .14 .10 .09 .11 .10 .14
  <TB,2,1,1,1> 128/128/192, 96/128/256 TB 1-5: .28 .23 .32 .28 .28 | .10 .08 .11 .13 .10
  <TB,2,1,1> 128/256/256 TB 1-4: .33 .28 .32 .35 | .12 .10 .09 .08
sa_rag_kernel, f32 | bf16x3 | bf16 (`-` = not instantiated there):
  <2,2,1,1,1,1> .18 | .43 | .14    <2,2,1,1,1,0> .18 | .34 | .14    <2,2,1,1,2,0> .23 | .32 | .14    <2,2,0,0,1,0> .14 | - | -
  <2,2,0,0,2,0> .26 | - | -        <4,1,1,1,1,0> .24 | .38 | .16    <4,1,2,1,1,2> .16 | .39 | .13    <4,1,2,1,1,0> .15 | .47 | .16
  <4,1,2,2,1,0> .18 | .42 | .18    <4,1,4,4,1,0> .11 | .35 | .10    <4,1,0,0,1,0> .15 | - | -
sa_stream_rag_kernel, bf16x3 | bf16, index form <..,false,8> then table form <..,true,12>:
  <1,1> .49 .41 | .11 .13      <2,2> .44 .48 | .16 .18      <2,4> .26 .34 | .10 .12
sa_stream_kernel <1,1> .36 | .20   <2,2> .33 | .14   <2,4> .32 | .09   <4,4> .48 | .12      sa_wsplit_rag_kernel<4,8> .43 | .12
sa_mlp_kernel (fast=False on three shapes; 20/40/72, whose c1 % 8 != 0 sa_make_plan refuses) .13
"""
import zlib

import pytest
import torch

import sa_ref as R

# err = max|got - sa_ref| / max|sa_ref|.  The project's own bounds for this layer, per arithmetic:
# test_gpu_precision.py::test_sa_layer_in_every_precision_against_torch (all three), BOUND of test_gpu_sa_krow_items.py
BOUNDS = {"f32": 2e-6, "bf16x3": 2e-5, "bf16": 3e-2}

# (asked precision, mode, D, widths, K, S, group kind | None = no hit counts, B, row table fed, fast, unit + instantiation)
# tests/test_sa_ref_cpu.py recomputes the last column from sa_ref.dispatch and holds the table complete.
ROWS = [
    # ---- K-row tile kernel sa_fused_kernel, f32 mode: one K per (TB, MAXE) the cost model can choose, per width form
    ('f32', 0, 8, (32, 32, 32), 43, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,4,4,1,4,full>'),
    ('f32', 1, 0, (32, 32, 32), 43, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,4,4,1,4,full>'),
    ('f32', 1, 5, (32, 32, 32), 1, 131, None, 3, 0, 1, 'f32 krow_tile<4,1,4,4,1,4,full>'),
    ('f32', 0, 8, (32, 32, 32), 129, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,4,4,1,4,full>'),
    ('f32', 1, 5, (32, 32, 32), 161, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,4,4,1,4,full>'),
    ('f32', 0, 8, (32, 32, 32), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,4,4,1,4,maxe>'),
    ('f32', 1, 5, (32, 32, 32), 16, 17, None, 3, 0, 1, 'f32 krow_tile<4,1,4,4,1,4,maxe>'),
    ('f32', 0, 8, (32, 32, 32), 144, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,4,4,1,4,maxe>'),
    ('f32', 1, 5, (32, 32, 32), 176, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,4,4,1,4,maxe>'),
    ('f32', 0, 8, (64, 32, 32), 43, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,4,4,full>'),
    ('f32', 1, 0, (64, 32, 32), 43, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,4,4,full>'),
    ('f32', 1, 5, (64, 32, 32), 1, 131, None, 3, 0, 1, 'f32 krow_tile<4,1,4,4,full>'),
    ('f32', 0, 8, (64, 32, 32), 129, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,4,4,full>'),
    ('f32', 1, 5, (64, 32, 32), 161, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,4,4,full>'),
    ('f32', 0, 8, (64, 32, 32), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,4,4,maxe>'),
    ('f32', 1, 5, (64, 32, 32), 16, 17, None, 3, 0, 1, 'f32 krow_tile<4,1,4,4,maxe>'),
    ('f32', 0, 8, (64, 32, 32), 144, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,4,4,maxe>'),
    ('f32', 1, 5, (64, 32, 32), 176, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,4,4,maxe>'),
    ('f32', 0, 8, (64, 64, 64), 1, 129, None, 3, 0, 1, 'f32 krow_tile<2,1,2,2,full>'),
    ('f32', 1, 0, (64, 64, 64), 1, 129, None, 3, 0, 1, 'f32 krow_tile<2,1,2,2,full>'),
    ('f32', 1, 5, (64, 64, 64), 11, 23, None, 3, 0, 1, 'f32 krow_tile<4,1,2,2,full>'),
    ('f32', 0, 8, (64, 64, 64), 65, 5, None, 3, 0, 1, 'f32 krow_tile<5,1,2,2,full>'),
    ('f32', 1, 5, (64, 64, 64), 43, 9, None, 3, 0, 1, 'f32 krow_tile<6,1,2,2,full>'),
    ('f32', 0, 8, (64, 64, 64), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,1,2,2,maxe>'),
    ('f32', 1, 5, (64, 64, 64), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,1,2,2,maxe>'),
    ('f32', 0, 8, (64, 64, 64), 80, 5, None, 3, 0, 1, 'f32 krow_tile<5,1,2,2,maxe>'),
    ('f32', 1, 5, (64, 64, 64), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,1,2,2,maxe>'),
    ('f32', 0, 8, (128, 128, 128), 1, 65, None, 3, 0, 1, 'f32 krow_tile<1,1,1,1,full>'),
    ('f32', 1, 0, (128, 128, 128), 1, 65, None, 3, 0, 1, 'f32 krow_tile<1,1,1,1,full>'),
    ('f32', 1, 5, (128, 128, 128), 7, 19, None, 3, 0, 1, 'f32 krow_tile<2,1,1,1,full>'),
    ('f32', 0, 8, (128, 128, 128), 22, 9, None, 3, 0, 1, 'f32 krow_tile<3,1,1,1,full>'),
    ('f32', 1, 5, (128, 128, 128), 97, 3, None, 3, 0, 1, 'f32 krow_tile<4,1,1,1,full>'),
    ('f32', 0, 8, (128, 128, 128), 129, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,1,1,full>'),
    ('f32', 1, 5, (128, 128, 128), 161, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,1,1,full>'),
    ('f32', 0, 8, (128, 128, 128), 16, 5, None, 3, 0, 1, 'f32 krow_tile<1,1,1,1,maxe>'),
    ('f32', 1, 5, (128, 128, 128), 64, 3, None, 3, 0, 1, 'f32 krow_tile<2,1,1,1,maxe>'),
    ('f32', 0, 8, (128, 128, 128), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,1,1,maxe>'),
    ('f32', 1, 5, (128, 128, 128), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,1,1,1,maxe>'),
    ('f32', 0, 8, (128, 128, 128), 144, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,1,1,maxe>'),
    ('f32', 1, 5, (128, 128, 128), 176, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,1,1,maxe>'),
    ('f32', 0, 8, (128, 128, 256), 1, 65, None, 3, 0, 1, 'f32 krow_tile<1,2,1,1,1,full>'),
    ('f32', 1, 0, (128, 128, 256), 1, 65, None, 3, 0, 1, 'f32 krow_tile<1,2,1,1,1,full>'),
    ('f32', 1, 5, (128, 128, 256), 11, 11, None, 3, 0, 1, 'f32 krow_tile<2,2,1,1,1,full>'),
    ('f32', 0, 8, (128, 128, 256), 65, 3, None, 3, 0, 1, 'f32 krow_tile<3,2,1,1,1,full>'),
    ('f32', 1, 5, (128, 128, 256), 33, 7, None, 3, 0, 1, 'f32 krow_tile<4,2,1,1,1,full>'),
    ('f32', 0, 8, (128, 128, 256), 16, 5, None, 3, 0, 1, 'f32 krow_tile<1,2,1,1,1,maxe>'),
    ('f32', 1, 5, (128, 128, 256), 64, 3, None, 3, 0, 1, 'f32 krow_tile<2,2,1,1,1,maxe>'),
    ('f32', 0, 8, (128, 128, 256), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,2,1,1,1,maxe>'),
    ('f32', 1, 5, (128, 128, 256), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,2,1,1,1,maxe>'),
    ('f32', 0, 8, (128, 128, 256), 144, 3, None, 3, 0, 1, 'f32 krow_tile<5,2,1,1,1,maxe>'),
    ('f32', 1, 5, (128, 256, 256), 1, 65, None, 3, 0, 1, 'f32 krow_tile<1,2,1,1,full>'),
    ('f32', 1, 0, (128, 256, 256), 1, 65, None, 3, 0, 1, 'f32 krow_tile<1,2,1,1,full>'),
    ('f32', 0, 8, (128, 256, 256), 11, 11, None, 3, 0, 1, 'f32 krow_tile<2,2,1,1,full>'),
    ('f32', 1, 5, (128, 256, 256), 65, 3, None, 3, 0, 1, 'f32 krow_tile<3,2,1,1,full>'),
    ('f32', 0, 8, (128, 256, 256), 33, 7, None, 3, 0, 1, 'f32 krow_tile<4,2,1,1,full>'),
    ('f32', 1, 5, (128, 256, 256), 16, 5, None, 3, 0, 1, 'f32 krow_tile<1,2,1,1,maxe>'),
    ('f32', 0, 8, (128, 256, 256), 48, 3, None, 3, 0, 1, 'f32 krow_tile<2,2,1,1,maxe>'),
    ('f32', 1, 5, (128, 256, 256), 80, 3, None, 3, 0, 1, 'f32 krow_tile<3,2,1,1,maxe>'),
    ('f32', 0, 8, (128, 256, 256), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,2,1,1,maxe>'),
    ('f32', 1, 5, (32, 64, 128), 1, 129, None, 3, 0, 1, 'f32 krow_tile<2,1,0,0,full>'),
    ('f32', 1, 0, (32, 64, 128), 1, 129, None, 3, 0, 1, 'f32 krow_tile<2,1,0,0,full>'),
    ('f32', 0, 8, (32, 64, 128), 65, 3, None, 3, 0, 1, 'f32 krow_tile<3,1,0,0,full>'),
    ('f32', 1, 5, (32, 64, 128), 22, 11, None, 3, 0, 1, 'f32 krow_tile<4,1,0,0,full>'),
    ('f32', 0, 8, (32, 64, 128), 129, 3, None, 3, 0, 1, 'f32 krow_tile<5,1,0,0,full>'),
    ('f32', 1, 5, (32, 64, 128), 161, 3, None, 3, 0, 1, 'f32 krow_tile<6,1,0,0,full>'),
    ('f32', 0, 8, (32, 64, 128), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,1,0,0,maxe>'),
    ('f32', 1, 5, (32, 64, 128), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,1,0,0,maxe>'),
    ('f32', 0, 8, (32, 64, 128), 80, 5, None, 3, 0, 1, 'f32 krow_tile<5,1,0,0,maxe>'),
    ('f32', 1, 5, (32, 64, 128), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,1,0,0,maxe>'),
    ('f32', 0, 8, (64, 64, 256), 1, 107, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,full>'),
    ('f32', 1, 0, (64, 64, 256), 1, 107, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,full>'),
    ('f32', 1, 5, (64, 64, 256), 65, 3, None, 3, 0, 1, 'f32 krow_tile<3,2,0,0,1,full>'),
    ('f32', 0, 8, (64, 64, 256), 33, 7, None, 3, 0, 1, 'f32 krow_tile<4,2,0,0,1,full>'),
    ('f32', 1, 5, (64, 64, 256), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,maxe>'),
    ('f32', 0, 8, (64, 64, 256), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,2,0,0,1,maxe>'),
    ('f32', 1, 5, (64, 64, 256), 80, 5, None, 3, 0, 1, 'f32 krow_tile<5,2,0,0,1,maxe>'),
    ('f32', 0, 8, (64, 64, 256), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,2,0,0,1,maxe>'),
    ('f32', 1, 5, (64, 256, 64), 1, 107, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,full>'),
    ('f32', 1, 0, (64, 256, 64), 1, 107, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,full>'),
    ('f32', 0, 8, (64, 256, 64), 65, 3, None, 3, 0, 1, 'f32 krow_tile<3,2,0,0,full>'),
    ('f32', 1, 5, (64, 256, 64), 33, 7, None, 3, 0, 1, 'f32 krow_tile<4,2,0,0,full>'),
    ('f32', 0, 8, (64, 256, 64), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,maxe>'),
    ('f32', 1, 5, (64, 256, 64), 80, 3, None, 3, 0, 1, 'f32 krow_tile<3,2,0,0,maxe>'),
    ('f32', 0, 8, (64, 256, 64), 112, 3, None, 3, 0, 1, 'f32 krow_tile<4,2,0,0,maxe>'),
    ('f32', 1, 5, (128, 256, 512), 1, 53, None, 3, 0, 1, 'f32 krow_tile<1,4,1,1,4,full>'),
    ('f32', 1, 0, (128, 256, 512), 1, 53, None, 3, 0, 1, 'f32 krow_tile<1,4,1,1,4,full>'),
    ('f32', 0, 8, (128, 256, 512), 17, 7, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,full>'),
    ('f32', 1, 5, (128, 256, 512), 16, 5, None, 3, 0, 1, 'f32 krow_tile<1,4,1,1,4,maxe>'),
    ('f32', 0, 8, (128, 256, 512), 48, 3, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,maxe>'),
    # (padded cout blocks; 64/64/512: layer 2 has two cout blocks under W2 = 1, its clamped blocks must stay harmless)
    ('f32', 1, 5, (72, 100, 120), 12, 11, None, 3, 0, 1, 'f32 krow_tile<2,1,1,1,full>'),
    ('f32', 0, 8, (72, 100, 120), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,1,1,maxe>'),
    ('f32', 1, 5, (24, 40, 72), 20, 7, None, 3, 0, 1, 'f32 krow_tile<2,1,0,0,full>'),
    ('f32', 0, 8, (24, 40, 72), 32, 5, None, 3, 0, 1, 'f32 krow_tile<2,1,0,0,maxe>'),
    ('f32', 1, 5, (64, 64, 512), 10, 13, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,full>'),
    ('f32', 0, 8, (64, 64, 512), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,maxe>'),
    ('f32', 1, 5, (64, 64, 512), 64, 3, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,maxe>'),
    ('f32', 0, 8, (64, 64, 64), 48, 9, None, 11, 0, 1, 'f32 krow_tile<6,1,2,2,maxe>'),
    # (narrower last layers leave LDS for pairs the ten forms above cannot reach)
    ('f32', 0, 8, (64, 64, 160), 129, 3, None, 3, 0, 1, 'f32 krow_tile<5,2,0,0,1,full>'),
    ('f32', 1, 5, (64, 64, 160), 33, 11, None, 3, 0, 1, 'f32 krow_tile<6,2,0,0,1,full>'),
    ('f32', 0, 8, (128, 128, 192), 129, 3, None, 3, 0, 1, 'f32 krow_tile<5,2,1,1,1,full>'),
    # ---- K-row tile kernel, bf16x3: shapes neither the stream nor the cout-split kernel takes, one K per reachable TB
    ('bf16x3', 0, 8, (32, 32, 32), 80, 3, None, 3, 0, 1, 'bf16x3 krow_tile<3,1,4,4,maxe>'),
    ('bf16x3', 1, 0, (32, 32, 32), 80, 3, None, 3, 0, 1, 'bf16x3 krow_tile<3,1,4,4,maxe>'),
    ('bf16x3', 0, 8, (32, 32, 32), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,1,4,4,maxe>'),
    ('bf16x3', 0, 8, (32, 32, 32), 144, 3, None, 3, 0, 1, 'bf16x3 krow_tile<5,1,4,4,maxe>'),
    ('bf16x3', 0, 8, (32, 32, 32), 176, 3, None, 3, 0, 1, 'bf16x3 krow_tile<6,1,4,4,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 64), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,1,2,2,maxe>'),
    ('bf16x3', 1, 0, (64, 64, 64), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,1,2,2,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 64), 80, 5, None, 3, 0, 1, 'bf16x3 krow_tile<5,1,2,2,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 64), 176, 3, None, 3, 0, 1, 'bf16x3 krow_tile<6,1,2,2,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 96), 16, 9, None, 3, 0, 1, 'bf16x3 krow_tile<2,1,2,1,maxe>'),
    ('bf16x3', 1, 0, (64, 64, 96), 16, 9, None, 3, 0, 1, 'bf16x3 krow_tile<2,1,2,1,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 96), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,1,2,1,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 96), 80, 5, None, 3, 0, 1, 'bf16x3 krow_tile<5,1,2,1,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 96), 48, 9, None, 3, 0, 1, 'bf16x3 krow_tile<6,1,2,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,1,1,1,maxe>'),
    ('bf16x3', 1, 0, (96, 96, 96), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 64, 3, None, 3, 0, 1, 'bf16x3 krow_tile<2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 48, 5, None, 3, 0, 1, 'bf16x3 krow_tile<3,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 144, 3, None, 3, 0, 1, 'bf16x3 krow_tile<5,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 176, 3, None, 3, 0, 1, 'bf16x3 krow_tile<6,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 128, 192), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16x3', 1, 0, (128, 128, 192), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 128, 192), 64, 3, None, 3, 0, 1, 'bf16x3 krow_tile<2,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 128, 192), 48, 5, None, 3, 0, 1, 'bf16x3 krow_tile<3,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 128, 192), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 128, 192), 144, 3, None, 3, 0, 1, 'bf16x3 krow_tile<5,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 128, 256), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16x3', 1, 0, (96, 128, 256), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 128, 256), 64, 3, None, 3, 0, 1, 'bf16x3 krow_tile<2,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 128, 256), 48, 5, None, 3, 0, 1, 'bf16x3 krow_tile<3,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 128, 256), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 128, 256), 144, 3, None, 3, 0, 1, 'bf16x3 krow_tile<5,2,1,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 256, 256), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,2,1,1,maxe>'),
    ('bf16x3', 1, 0, (128, 256, 256), 16, 5, None, 3, 0, 1, 'bf16x3 krow_tile<1,2,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 256, 256), 48, 3, None, 3, 0, 1, 'bf16x3 krow_tile<2,2,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 256, 256), 80, 3, None, 3, 0, 1, 'bf16x3 krow_tile<3,2,1,1,maxe>'),
    ('bf16x3', 0, 8, (128, 256, 256), 112, 3, None, 3, 0, 1, 'bf16x3 krow_tile<4,2,1,1,maxe>'),
    ('bf16x3', 0, 8, (96, 96, 96), 32, 3, None, 11, 0, 1, 'bf16x3 krow_tile<1,1,1,1,maxe>'),
    # (64 / 64 / c3 > 128: two cout-block rounds of layer 3 under (2 ways, 1 way), which the bf16 units refuse)
    ('bf16x3', 0, 8, (64, 64, 160), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 160), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,2,0,0,1,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 256), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 256), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,2,0,0,1,maxe>'),
    # (refused by the bf16 units: no layer 1 on the matrix core, (1 way, 2 ways), K % 16 != 0, 512-wide layers)
    ('bf16x3', 0, 8, (32, 64, 64), 80, 5, None, 3, 0, 1, 'f32 krow_tile<5,1,2,2,maxe>'),
    ('bf16x3', 0, 8, (64, 256, 64), 32, 5, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,maxe>'),
    ('bf16x3', 1, 5, (64, 64, 64), 20, 7, None, 3, 0, 1, 'f32 krow_tile<2,1,2,2,full>'),
    ('bf16x3', 1, 5, (128, 128, 128), 44, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,1,1,full>'),
    ('bf16x3', 0, 8, (128, 256, 512), 16, 5, None, 3, 0, 1, 'f32 krow_tile<1,4,1,1,4,maxe>'),
    ('bf16x3', 1, 0, (64, 64, 512), 32, 5, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,maxe>'),
    # ---- the same in bf16
    ('bf16', 0, 8, (32, 32, 32), 80, 3, None, 3, 0, 1, 'bf16 krow_tile<3,1,4,4,maxe>'),
    ('bf16', 1, 0, (32, 32, 32), 80, 3, None, 3, 0, 1, 'bf16 krow_tile<3,1,4,4,maxe>'),
    ('bf16', 0, 8, (32, 32, 32), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,1,4,4,maxe>'),
    ('bf16', 0, 8, (32, 32, 32), 144, 3, None, 3, 0, 1, 'bf16 krow_tile<5,1,4,4,maxe>'),
    ('bf16', 0, 8, (32, 32, 32), 176, 3, None, 3, 0, 1, 'bf16 krow_tile<6,1,4,4,maxe>'),
    ('bf16', 0, 8, (64, 64, 64), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,1,2,2,maxe>'),
    ('bf16', 1, 0, (64, 64, 64), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,1,2,2,maxe>'),
    ('bf16', 0, 8, (64, 64, 64), 80, 5, None, 3, 0, 1, 'bf16 krow_tile<5,1,2,2,maxe>'),
    ('bf16', 0, 8, (64, 64, 64), 176, 3, None, 3, 0, 1, 'bf16 krow_tile<6,1,2,2,maxe>'),
    ('bf16', 0, 8, (64, 64, 96), 16, 9, None, 3, 0, 1, 'bf16 krow_tile<2,1,2,1,maxe>'),
    ('bf16', 1, 0, (64, 64, 96), 16, 9, None, 3, 0, 1, 'bf16 krow_tile<2,1,2,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 96), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,1,2,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 96), 80, 5, None, 3, 0, 1, 'bf16 krow_tile<5,1,2,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 96), 48, 9, None, 3, 0, 1, 'bf16 krow_tile<6,1,2,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,1,1,1,maxe>'),
    ('bf16', 1, 0, (96, 96, 96), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 64, 3, None, 3, 0, 1, 'bf16 krow_tile<2,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 48, 5, None, 3, 0, 1, 'bf16 krow_tile<3,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 144, 3, None, 3, 0, 1, 'bf16 krow_tile<5,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 176, 3, None, 3, 0, 1, 'bf16 krow_tile<6,1,1,1,maxe>'),
    ('bf16', 0, 8, (128, 128, 192), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16', 1, 0, (128, 128, 192), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (128, 128, 192), 64, 3, None, 3, 0, 1, 'bf16 krow_tile<2,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (128, 128, 192), 48, 5, None, 3, 0, 1, 'bf16 krow_tile<3,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (128, 128, 192), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (128, 128, 192), 144, 3, None, 3, 0, 1, 'bf16 krow_tile<5,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 128, 256), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16', 1, 0, (96, 128, 256), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 128, 256), 64, 3, None, 3, 0, 1, 'bf16 krow_tile<2,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 128, 256), 48, 5, None, 3, 0, 1, 'bf16 krow_tile<3,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 128, 256), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (96, 128, 256), 144, 3, None, 3, 0, 1, 'bf16 krow_tile<5,2,1,1,1,maxe>'),
    ('bf16', 0, 8, (128, 256, 256), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,2,1,1,maxe>'),
    ('bf16', 1, 0, (128, 256, 256), 16, 5, None, 3, 0, 1, 'bf16 krow_tile<1,2,1,1,maxe>'),
    ('bf16', 0, 8, (128, 256, 256), 48, 3, None, 3, 0, 1, 'bf16 krow_tile<2,2,1,1,maxe>'),
    ('bf16', 0, 8, (128, 256, 256), 80, 3, None, 3, 0, 1, 'bf16 krow_tile<3,2,1,1,maxe>'),
    ('bf16', 0, 8, (128, 256, 256), 112, 3, None, 3, 0, 1, 'bf16 krow_tile<4,2,1,1,maxe>'),
    ('bf16', 0, 8, (96, 96, 96), 32, 3, None, 11, 0, 1, 'bf16 krow_tile<1,1,1,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 160), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 160), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,2,0,0,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 256), 16, 9, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,1,maxe>'),
    ('bf16', 0, 8, (64, 64, 256), 48, 9, None, 3, 0, 1, 'f32 krow_tile<6,2,0,0,1,maxe>'),
    ('bf16', 0, 8, (32, 64, 64), 80, 5, None, 3, 0, 1, 'f32 krow_tile<5,1,2,2,maxe>'),
    ('bf16', 0, 8, (64, 256, 64), 32, 5, None, 3, 0, 1, 'f32 krow_tile<2,2,0,0,maxe>'),
    ('bf16', 1, 5, (64, 64, 64), 20, 7, None, 3, 0, 1, 'f32 krow_tile<2,1,2,2,full>'),
    ('bf16', 1, 5, (128, 128, 128), 44, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,1,1,full>'),
    ('bf16', 0, 8, (128, 256, 512), 16, 5, None, 3, 0, 1, 'f32 krow_tile<1,4,1,1,4,maxe>'),
    ('bf16', 1, 0, (64, 64, 512), 32, 5, None, 3, 0, 1, 'f32 krow_tile<2,4,1,1,4,maxe>'),
    # ---- ragged tile kernel sa_rag_kernel, f32 mode: the eleven forms x group kinds x K in {1, 20, tile rows}
    ('f32', 1, 5, (128, 128, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,1>'),
    ('f32', 1, 5, (128, 128, 256), 64, 3, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,1>'),
    ('f32', 1, 5, (128, 128, 256), 64, 3, 'full', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,1>'),
    ('f32', 1, 5, (128, 128, 256), 20, 7, 'ones', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,1>'),
    ('f32', 1, 5, (128, 128, 256), 1, 65, 'full', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,1>'),
    ('f32', 1, 5, (64, 128, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,0>'),
    ('f32', 1, 5, (64, 128, 256), 64, 3, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,0>'),
    ('f32', 1, 5, (64, 128, 256), 64, 3, 'full', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,0>'),
    ('f32', 1, 5, (64, 128, 256), 20, 7, 'ones', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,0>'),
    ('f32', 1, 5, (64, 128, 256), 1, 65, 'full', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,0>'),
    ('f32', 1, 5, (128, 256, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,2,0>'),
    ('f32', 1, 5, (128, 256, 256), 64, 3, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,2,0>'),
    ('f32', 1, 5, (128, 256, 256), 64, 3, 'full', 3, 0, 1, 'f32 rag_tile<2,2,1,1,2,0>'),
    ('f32', 1, 5, (128, 256, 256), 20, 7, 'ones', 3, 0, 1, 'f32 rag_tile<2,2,1,1,2,0>'),
    ('f32', 1, 5, (128, 256, 256), 1, 65, 'full', 3, 0, 1, 'f32 rag_tile<2,2,1,1,2,0>'),
    ('f32', 1, 5, (32, 64, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,0,0,1,0>'),
    ('f32', 1, 5, (32, 64, 256), 64, 3, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,0,0,1,0>'),
    ('f32', 1, 5, (32, 64, 256), 64, 3, 'full', 3, 0, 1, 'f32 rag_tile<2,2,0,0,1,0>'),
    ('f32', 1, 5, (32, 64, 256), 20, 7, 'ones', 3, 0, 1, 'f32 rag_tile<2,2,0,0,1,0>'),
    ('f32', 1, 5, (32, 64, 256), 1, 65, 'full', 3, 0, 1, 'f32 rag_tile<2,2,0,0,1,0>'),
    ('f32', 1, 5, (64, 256, 64), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,0,0,2,0>'),
    ('f32', 1, 5, (64, 256, 64), 64, 3, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,0,0,2,0>'),
    ('f32', 1, 5, (64, 256, 64), 64, 3, 'full', 3, 0, 1, 'f32 rag_tile<2,2,0,0,2,0>'),
    ('f32', 1, 5, (64, 256, 64), 20, 7, 'ones', 3, 0, 1, 'f32 rag_tile<2,2,0,0,2,0>'),
    ('f32', 1, 5, (64, 256, 64), 1, 65, 'full', 3, 0, 1, 'f32 rag_tile<2,2,0,0,2,0>'),
    ('f32', 1, 5, (128, 128, 128), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    ('f32', 1, 5, (128, 128, 128), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    ('f32', 1, 5, (128, 128, 128), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    ('f32', 1, 5, (128, 128, 128), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    ('f32', 1, 5, (128, 128, 128), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    ('f32', 1, 0, (64, 64, 128), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,2>'),
    ('f32', 1, 0, (64, 64, 128), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,2>'),
    ('f32', 1, 0, (64, 64, 128), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,2>'),
    ('f32', 1, 0, (64, 64, 128), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,2>'),
    ('f32', 1, 0, (64, 64, 128), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,2>'),
    ('f32', 1, 5, (64, 64, 128), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (64, 64, 128), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (64, 64, 128), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (64, 64, 128), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (64, 64, 128), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (32, 64, 128), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (32, 64, 128), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (32, 64, 128), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (32, 64, 128), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (32, 64, 128), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 5, (64, 64, 64), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,2,1,0>'),
    ('f32', 1, 5, (64, 64, 64), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,2,1,0>'),
    ('f32', 1, 5, (64, 64, 64), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,2,1,0>'),
    ('f32', 1, 5, (64, 64, 64), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,2,2,1,0>'),
    ('f32', 1, 5, (64, 64, 64), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,2,2,1,0>'),
    ('f32', 1, 5, (32, 32, 32), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,4,4,1,0>'),
    ('f32', 1, 5, (32, 32, 32), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,4,4,1,0>'),
    ('f32', 1, 5, (32, 32, 32), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,4,4,1,0>'),
    ('f32', 1, 5, (32, 32, 32), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,4,4,1,0>'),
    ('f32', 1, 5, (32, 32, 32), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,4,4,1,0>'),
    ('f32', 1, 5, (32, 128, 64), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('f32', 1, 5, (32, 128, 64), 128, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('f32', 1, 5, (32, 128, 64), 128, 3, 'full', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('f32', 1, 5, (32, 128, 64), 20, 13, 'ones', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('f32', 1, 5, (32, 128, 64), 1, 129, 'full', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('f32', 1, 0, (32, 32, 32), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,4,4,1,0>'),
    ('f32', 1, 5, (128, 128, 128), 20, 13, 'rand', 11, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    # (K above the tile's rows with hit counts: falls through to the K-row kernel)
    ('f32', 1, 5, (128, 128, 256), 80, 3, 'rand', 3, 0, 1, 'f32 krow_tile<3,2,1,1,1,maxe>'),
    ('f32', 1, 5, (64, 64, 64), 144, 3, 'rand', 3, 0, 1, 'f32 krow_tile<5,1,2,2,maxe>'),
    # ---- ragged tile kernel, bf16x3: the eight explicit forms at shapes the stream form does not take
    ('bf16x3', 1, 5, (128, 128, 192), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 5, (128, 128, 192), 64, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 5, (128, 128, 192), 1, 65, 'ones', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 5, (64, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,0>'),
    ('bf16x3', 1, 5, (64, 128, 256), 64, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,0>'),
    ('bf16x3', 1, 5, (64, 128, 256), 1, 65, 'ones', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,0>'),
    ('bf16x3', 1, 5, (96, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 5, (96, 128, 256), 64, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 5, (96, 128, 256), 1, 65, 'ones', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 5, (128, 256, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,2,0>'),
    ('bf16x3', 1, 5, (128, 256, 256), 64, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,2,0>'),
    ('bf16x3', 1, 5, (128, 256, 256), 1, 65, 'ones', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,2,0>'),
    ('bf16x3', 1, 5, (96, 96, 96), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,1,1,1,0>'),
    ('bf16x3', 1, 5, (96, 96, 96), 128, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<4,1,1,1,1,0>'),
    ('bf16x3', 1, 5, (96, 96, 96), 1, 129, 'ones', 3, 0, 1, 'bf16x3 rag_tile<4,1,1,1,1,0>'),
    ('bf16x3', 1, 0, (64, 64, 128), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,2>'),
    ('bf16x3', 1, 0, (64, 64, 128), 128, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,2>'),
    ('bf16x3', 1, 0, (64, 64, 128), 1, 129, 'ones', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,2>'),
    ('bf16x3', 1, 5, (64, 64, 96), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,0>'),
    ('bf16x3', 1, 5, (64, 64, 96), 128, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,0>'),
    ('bf16x3', 1, 5, (64, 64, 96), 1, 129, 'ones', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,0>'),
    ('bf16x3', 1, 5, (64, 64, 64), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 5, (64, 64, 64), 128, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 5, (64, 64, 64), 1, 129, 'ones', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 5, (32, 32, 32), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,4,4,1,0>'),
    ('bf16x3', 1, 5, (32, 32, 32), 128, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<4,1,4,4,1,0>'),
    ('bf16x3', 1, 5, (32, 32, 32), 1, 129, 'ones', 3, 0, 1, 'bf16x3 rag_tile<4,1,4,4,1,0>'),
    ('bf16x3', 1, 5, (32, 64, 64), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 5, (32, 64, 64), 128, 3, 'full', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 5, (32, 64, 64), 1, 129, 'ones', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 5, (96, 96, 96), 20, 13, 'rand', 11, 0, 1, 'bf16x3 rag_tile<4,1,1,1,1,0>'),
    ('bf16x3', 1, 5, (128, 128, 192), 80, 3, 'rand', 3, 0, 1, 'bf16x3 krow_tile<3,2,1,1,1,maxe>'),
    # (the cout-split kernel, ragged and K-row: tests/test_gpu_sa_wsplit.py holds it to torch, this file to float64)
    ('bf16x3', 1, 5, (128, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 wsplit<4,8>'),
    ('bf16x3', 1, 5, (128, 128, 256), 64, 3, None, 3, 0, 1, 'bf16x3 wsplit<4,8>'),
    # ---- the same in bf16
    ('bf16', 1, 5, (128, 128, 192), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 5, (128, 128, 192), 64, 3, 'full', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 5, (128, 128, 192), 1, 65, 'ones', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 5, (64, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,0>'),
    ('bf16', 1, 5, (64, 128, 256), 64, 3, 'full', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,0>'),
    ('bf16', 1, 5, (64, 128, 256), 1, 65, 'ones', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,0>'),
    ('bf16', 1, 5, (96, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 5, (96, 128, 256), 64, 3, 'full', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 5, (96, 128, 256), 1, 65, 'ones', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 5, (128, 256, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,2,0>'),
    ('bf16', 1, 5, (128, 256, 256), 64, 3, 'full', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,2,0>'),
    ('bf16', 1, 5, (128, 256, 256), 1, 65, 'ones', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,2,0>'),
    ('bf16', 1, 5, (96, 96, 96), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,1,1,1,0>'),
    ('bf16', 1, 5, (96, 96, 96), 128, 3, 'full', 3, 0, 1, 'bf16 rag_tile<4,1,1,1,1,0>'),
    ('bf16', 1, 5, (96, 96, 96), 1, 129, 'ones', 3, 0, 1, 'bf16 rag_tile<4,1,1,1,1,0>'),
    ('bf16', 1, 0, (64, 64, 128), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,2>'),
    ('bf16', 1, 0, (64, 64, 128), 128, 3, 'full', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,2>'),
    ('bf16', 1, 0, (64, 64, 128), 1, 129, 'ones', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,2>'),
    ('bf16', 1, 5, (64, 64, 96), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,0>'),
    ('bf16', 1, 5, (64, 64, 96), 128, 3, 'full', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,0>'),
    ('bf16', 1, 5, (64, 64, 96), 1, 129, 'ones', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,0>'),
    ('bf16', 1, 5, (64, 64, 64), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 5, (64, 64, 64), 128, 3, 'full', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 5, (64, 64, 64), 1, 129, 'ones', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 5, (32, 32, 32), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,4,4,1,0>'),
    ('bf16', 1, 5, (32, 32, 32), 128, 3, 'full', 3, 0, 1, 'bf16 rag_tile<4,1,4,4,1,0>'),
    ('bf16', 1, 5, (32, 32, 32), 1, 129, 'ones', 3, 0, 1, 'bf16 rag_tile<4,1,4,4,1,0>'),
    ('bf16', 1, 5, (32, 64, 64), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 5, (32, 64, 64), 128, 3, 'full', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 5, (32, 64, 64), 1, 129, 'ones', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 5, (96, 96, 96), 20, 13, 'rand', 11, 0, 1, 'bf16 rag_tile<4,1,1,1,1,0>'),
    ('bf16', 1, 5, (128, 128, 192), 80, 3, 'rand', 3, 0, 1, 'bf16 krow_tile<3,2,1,1,1,maxe>'),
    ('bf16', 1, 5, (128, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 wsplit<4,8>'),
    ('bf16', 1, 5, (128, 128, 256), 64, 3, None, 3, 0, 1, 'bf16 wsplit<4,8>'),
    # ---- ragged stream kernel sa_stream_rag_kernel, bf16x3: index tensor and the ball query's row table; 32/32/64 is
    # refused by the tile-shape rule before the stream form is looked at and runs the f32 unit's ragged tile kernel;
    # 64/64/128 at K = 96 does not fit the index form's LDS and runs the ragged tile kernel.  Then the K-row stream
    # kernel, one row per form (tests/test_gpu_sa_krow_items.py is its thorough file)
    ('bf16x3', 1, 5, (32, 32, 32), 16, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<1,1>:idx8'),
    ('bf16x3', 1, 5, (32, 32, 32), 16, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<1,1>:tab12'),
    ('bf16x3', 1, 5, (32, 32, 32), 48, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<1,1>:idx8'),
    ('bf16x3', 1, 5, (32, 32, 32), 48, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<1,1>:tab12'),
    ('bf16x3', 1, 5, (32, 32, 32), 96, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<1,1>:idx8'),
    ('bf16x3', 1, 5, (32, 32, 32), 96, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<1,1>:tab12'),
    ('bf16x3', 1, 5, (32, 32, 64), 16, 17, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16x3', 1, 5, (32, 32, 64), 48, 5, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16x3', 1, 5, (32, 32, 64), 96, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16x3', 1, 5, (64, 64, 64), 16, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,2>:idx8'),
    ('bf16x3', 1, 5, (64, 64, 64), 16, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,2>:tab12'),
    ('bf16x3', 1, 5, (64, 64, 64), 48, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,2>:idx8'),
    ('bf16x3', 1, 5, (64, 64, 64), 48, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,2>:tab12'),
    ('bf16x3', 1, 5, (64, 64, 64), 96, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,2>:idx8'),
    ('bf16x3', 1, 5, (64, 64, 64), 96, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,2>:tab12'),
    ('bf16x3', 1, 5, (64, 64, 128), 16, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,4>:idx8'),
    ('bf16x3', 1, 5, (64, 64, 128), 16, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,4>:tab12'),
    ('bf16x3', 1, 5, (64, 64, 128), 48, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,4>:idx8'),
    ('bf16x3', 1, 5, (64, 64, 128), 48, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,4>:tab12'),
    ('bf16x3', 1, 5, (64, 64, 128), 96, 3, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,0>'),
    ('bf16x3', 1, 0, (32, 32, 32), 32, 33, 'ones', 3, 0, 1, 'bf16x3 stream_rag<1,1>:idx8'),
    ('bf16x3', 1, 5, (64, 64, 64), 32, 33, 'full', 11, 1, 1, 'bf16x3 stream_rag<2,2>:tab12'),
    ('bf16x3', 0, 8, (32, 32, 32), 48, 5, None, 3, 0, 1, 'bf16x3 stream<1,1>'),
    ('bf16x3', 0, 8, (32, 32, 64), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,0,0,maxe>'),
    ('bf16x3', 0, 8, (64, 64, 64), 48, 5, None, 3, 0, 1, 'bf16x3 stream<2,2>'),
    ('bf16x3', 0, 8, (64, 64, 128), 48, 5, None, 3, 0, 1, 'bf16x3 stream<2,4>'),
    ('bf16x3', 0, 8, (128, 128, 128), 48, 5, None, 3, 0, 1, 'bf16x3 stream<4,4>'),
    ('bf16x3', 0, 8, (64, 64, 64), 32, 7, None, 11, 0, 1, 'bf16x3 stream<2,2>'),
    # ---- the same in bf16
    ('bf16', 1, 5, (32, 32, 32), 16, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<1,1>:idx8'),
    ('bf16', 1, 5, (32, 32, 32), 16, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<1,1>:tab12'),
    ('bf16', 1, 5, (32, 32, 32), 48, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<1,1>:idx8'),
    ('bf16', 1, 5, (32, 32, 32), 48, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<1,1>:tab12'),
    ('bf16', 1, 5, (32, 32, 32), 96, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<1,1>:idx8'),
    ('bf16', 1, 5, (32, 32, 32), 96, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<1,1>:tab12'),
    ('bf16', 1, 5, (32, 32, 64), 16, 17, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16', 1, 5, (32, 32, 64), 48, 5, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16', 1, 5, (32, 32, 64), 96, 3, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16', 1, 5, (64, 64, 64), 16, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,2>:idx8'),
    ('bf16', 1, 5, (64, 64, 64), 16, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,2>:tab12'),
    ('bf16', 1, 5, (64, 64, 64), 48, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,2>:idx8'),
    ('bf16', 1, 5, (64, 64, 64), 48, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,2>:tab12'),
    ('bf16', 1, 5, (64, 64, 64), 96, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,2>:idx8'),
    ('bf16', 1, 5, (64, 64, 64), 96, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,2>:tab12'),
    ('bf16', 1, 5, (64, 64, 128), 16, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,4>:idx8'),
    ('bf16', 1, 5, (64, 64, 128), 16, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,4>:tab12'),
    ('bf16', 1, 5, (64, 64, 128), 48, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,4>:idx8'),
    ('bf16', 1, 5, (64, 64, 128), 48, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,4>:tab12'),
    ('bf16', 1, 5, (64, 64, 128), 96, 3, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,0>'),
    ('bf16', 1, 0, (32, 32, 32), 32, 33, 'ones', 3, 0, 1, 'bf16 stream_rag<1,1>:idx8'),
    ('bf16', 1, 5, (64, 64, 64), 32, 33, 'full', 11, 1, 1, 'bf16 stream_rag<2,2>:tab12'),
    ('bf16', 0, 8, (32, 32, 32), 48, 5, None, 3, 0, 1, 'bf16 stream<1,1>'),
    ('bf16', 0, 8, (32, 32, 64), 48, 5, None, 3, 0, 1, 'f32 krow_tile<3,1,0,0,maxe>'),
    ('bf16', 0, 8, (64, 64, 64), 48, 5, None, 3, 0, 1, 'bf16 stream<2,2>'),
    ('bf16', 0, 8, (64, 64, 128), 48, 5, None, 3, 0, 1, 'bf16 stream<2,4>'),
    ('bf16', 0, 8, (128, 128, 128), 48, 5, None, 3, 0, 1, 'bf16 stream<4,4>'),
    ('bf16', 0, 8, (64, 64, 64), 32, 7, None, 11, 0, 1, 'bf16 stream<2,2>'),
    # ---- without features (D = 0: no layer-1 table, a code path of its own in every kernel), one row for each ragged
    # tile form, stream form (index and table, K-row) and the cout-split kernel in each unit that has it -- the K-row
    # tile forms have theirs above; and the cout-split kernel on more clouds than XCD slots
    ('f32', 1, 0, (128, 128, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,1>'),
    ('f32', 1, 0, (64, 128, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,1,0>'),
    ('f32', 1, 0, (128, 256, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,1,1,2,0>'),
    ('f32', 1, 0, (32, 64, 256), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,0,0,1,0>'),
    ('f32', 1, 0, (64, 256, 64), 20, 7, 'rand', 3, 0, 1, 'f32 rag_tile<2,2,0,0,2,0>'),
    ('f32', 1, 0, (128, 128, 128), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,1,1,1,0>'),
    ('f32', 1, 0, (32, 64, 128), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,1,1,0>'),
    ('f32', 1, 0, (64, 64, 64), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,2,2,1,0>'),
    ('f32', 1, 0, (32, 128, 64), 20, 13, 'rand', 3, 0, 1, 'f32 rag_tile<4,1,0,0,1,0>'),
    ('bf16x3', 1, 0, (128, 128, 192), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,1>'),
    ('bf16x3', 1, 0, (64, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,1,0>'),
    ('bf16x3', 1, 0, (128, 256, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 rag_tile<2,2,1,1,2,0>'),
    ('bf16x3', 1, 0, (96, 96, 96), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,1,1,1,0>'),
    ('bf16x3', 1, 0, (32, 64, 96), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,1,1,0>'),
    ('bf16x3', 1, 0, (64, 64, 64), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,2,2,1,0>'),
    ('bf16x3', 1, 0, (32, 32, 32), 20, 13, 'rand', 3, 0, 1, 'bf16x3 rag_tile<4,1,4,4,1,0>'),
    ('bf16x3', 1, 0, (64, 64, 64), 16, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,2>:idx8'),
    ('bf16x3', 1, 0, (64, 64, 128), 16, 33, 'rand', 3, 0, 1, 'bf16x3 stream_rag<2,4>:idx8'),
    ('bf16x3', 1, 0, (32, 32, 32), 16, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<1,1>:tab12'),
    ('bf16x3', 1, 0, (64, 64, 64), 16, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,2>:tab12'),
    ('bf16x3', 1, 0, (64, 64, 128), 16, 33, 'rand', 3, 1, 1, 'bf16x3 stream_rag<2,4>:tab12'),
    ('bf16x3', 1, 0, (128, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16x3 wsplit<4,8>'),
    ('bf16x3', 1, 5, (128, 128, 256), 20, 7, 'rand', 11, 0, 1, 'bf16x3 wsplit<4,8>'),
    ('bf16x3', 0, 0, (32, 32, 32), 32, 7, None, 3, 0, 1, 'bf16x3 stream<1,1>'),
    ('bf16x3', 0, 0, (64, 64, 64), 32, 7, None, 3, 0, 1, 'bf16x3 stream<2,2>'),
    ('bf16x3', 0, 0, (64, 64, 128), 32, 7, None, 3, 0, 1, 'bf16x3 stream<2,4>'),
    ('bf16x3', 0, 0, (128, 128, 128), 32, 7, None, 3, 0, 1, 'bf16x3 stream<4,4>'),
    ('bf16', 1, 0, (128, 128, 192), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,1>'),
    ('bf16', 1, 0, (64, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,1,0>'),
    ('bf16', 1, 0, (128, 256, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 rag_tile<2,2,1,1,2,0>'),
    ('bf16', 1, 0, (96, 96, 96), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,1,1,1,0>'),
    ('bf16', 1, 0, (32, 64, 96), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,1,1,0>'),
    ('bf16', 1, 0, (64, 64, 64), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,2,2,1,0>'),
    ('bf16', 1, 0, (32, 32, 32), 20, 13, 'rand', 3, 0, 1, 'bf16 rag_tile<4,1,4,4,1,0>'),
    ('bf16', 1, 0, (64, 64, 64), 16, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,2>:idx8'),
    ('bf16', 1, 0, (64, 64, 128), 16, 33, 'rand', 3, 0, 1, 'bf16 stream_rag<2,4>:idx8'),
    ('bf16', 1, 0, (32, 32, 32), 16, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<1,1>:tab12'),
    ('bf16', 1, 0, (64, 64, 64), 16, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,2>:tab12'),
    ('bf16', 1, 0, (64, 64, 128), 16, 33, 'rand', 3, 1, 1, 'bf16 stream_rag<2,4>:tab12'),
    ('bf16', 1, 0, (128, 128, 256), 20, 7, 'rand', 3, 0, 1, 'bf16 wsplit<4,8>'),
    ('bf16', 1, 5, (128, 128, 256), 20, 7, 'rand', 11, 0, 1, 'bf16 wsplit<4,8>'),
    ('bf16', 0, 0, (32, 32, 32), 32, 7, None, 3, 0, 1, 'bf16 stream<1,1>'),
    ('bf16', 0, 0, (64, 64, 64), 32, 7, None, 3, 0, 1, 'bf16 stream<2,2>'),
    ('bf16', 0, 0, (64, 64, 128), 32, 7, None, 3, 0, 1, 'bf16 stream<2,4>'),
    ('bf16', 0, 0, (128, 128, 128), 32, 7, None, 3, 0, 1, 'bf16 stream<4,4>'),
    # ---- generic kernel sa_mlp_kernel: fast=False, and c1 % 8 != 0 which sa_make_plan refuses
    ('f32', 0, 8, (64, 64, 64), 20, 5, None, 3, 0, 0, 'f32 generic<>'),
    ('bf16x3', 1, 5, (32, 64, 128), 16, 5, None, 3, 0, 0, 'f32 generic<>'),
    ('f32', 1, 0, (24, 40, 72), 7, 5, None, 11, 0, 0, 'f32 generic<>'),
    ('f32', 0, 8, (20, 40, 72), 16, 5, None, 3, 0, 1, 'f32 generic<>'),
    ('bf16x3', 1, 5, (20, 40, 72), 20, 5, 'rand', 3, 0, 1, 'f32 generic<>'),
]


def row_id(row):
    prec, mode, D, w, K, S, kind, B, table, fast, _ = row
    return "%s-m%d-D%d-%d_%d_%d-K%d%s%s%s%s" % (prec, mode, D, w[0], w[1], w[2], K, "-" + kind if kind else "",
                                                "-tab" if table else "", "-B%d" % B if B != 3 else "", "" if fast else "-slow")


def row_bound(row):
    """the bound of the arithmetic the row really runs in.  A launch the bf16 units refuse runs layers 2 / 3 in the f32
    unit, but engine.SaPlan.run has by then built the feature tables of layer 1 (D > 0) in the arithmetic that was asked
    for: only a row without tables, a row asked in f32 and the generic kernel (which reads no tables) are f32 throughout"""
    prec, D, expect = row[0], row[2], row[10]
    if expect.startswith("f32 ") and (prec == "f32" or D == 0 or "generic" in expect):
        return BOUNDS["f32"]
    return BOUNDS[prec]


def row_inputs(row, convs, bns):
    """xyz, feat, idx, cnt, centre_idx (CPU) and the float64 result.  Mode 0 rows take the prefix convention, mode 1 rows
    given centres.  Every group's first and last genuine rows own a channel's maximum (sa_ref.maxima_at_the_ends)."""
    prec, mode, D, w, K, S, kind, B, table, fast, _ = row
    g = torch.Generator().manual_seed(zlib.crc32(row_id(row).encode()))
    N = max(64, K + 8, S if mode == 0 else 0)
    xyz = torch.randn(B, N, 3, generator=g)
    feat = torch.randn(B, D, N, generator=g) if D else None
    idx, cnt = R.groups(B, N, S, K, kind or "full", g)
    cidx = torch.randint(0, N, (B, S), generator=g, dtype=torch.int32) if mode == 1 else None
    rows = R.sa_rows(convs, bns, mode, xyz, feat, idx, cidx)
    idx = R.maxima_at_the_ends(idx, cnt, rows)
    return xyz, feat, idx, cnt, cidx, rows.max(dim=2)[0].transpose(1, 2)


_plans = {}


def _plan(mode, D, widths, fast):
    from pcr_amd import engine
    key = (mode, D, widths, fast)
    if key not in _plans:      # (host-side weight packing is most of a plan's cost)
        convs, bns = R.layer(mode, D, widths)
        _plans[key] = (convs, bns, engine.SaPlan(convs, bns, torch.device("cuda"), mode, fast=bool(fast)))
    return _plans[key]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[row_id(r) for r in ROWS])
def test_form_against_float64(row):
    from pcr_amd import _lib as L
    from pcr_amd import engine
    prec, mode, D, w, K, S, kind, B, table, fast, expect = row
    lib = L.load()
    convs, bns, plan = _plan(mode, D, w, fast)
    xyz, feat, idx, cnt, cidx, want = row_inputs(row, convs, bns)
    scale = float(want.abs().max())
    y32 = float((R.sa_ref32(convs, bns, mode, xyz, feat, idx, cidx).double() - want).abs().max()) / scale
    tab = R.row_table(xyz, idx, cnt, cidx).view(B, -1) if table else None
    dev = lambda t: None if t is None else t.cuda()     # noqa: E731
    xyz_d, feat_d, idx_d, cnt_d, cidx_d, tab_d = dev(xyz), dev(feat), dev(idx), dev(cnt), dev(cidx), dev(tab)

    def run(sl=slice(None), pm=False, ragged=kind is not None, with_tab=bool(table)):
        c = lambda t: None if t is None else t[sl].contiguous()     # noqa: E731
        kw = dict(centre_idx=c(cidx_d), out_point_major=pm)
        if ragged:
            kw["cnt"] = c(cnt_d)
        if ragged and with_tab:
            out = plan.run(c(xyz_d), c(feat_d), None, rows=c(tab_d).reshape(-1), K=K, **kw)
        else:
            out = plan.run(c(xyz_d), c(feat_d), c(idx_d), **kw)
        return out, lib.pcr_last_launch_arith()

    with engine.precision(prec), torch.no_grad():
        if table:
            assert plan.wants_row_table(xyz.shape[1], K, 0.0, B, S)
        got, arith = run()
        again, _ = run()
        pm, _ = run(pm=True)
        alone = {b: run(sl=slice(b, b + 1))[0] for b in (0, B - 1)}
        from_idx = run(with_tab=False)[0] if table else None
        krow, arith_k = run(ragged=False) if kind is not None else (None, None)
    fails = []
    assert got.shape == (B, w[2], S)
    if not torch.isfinite(got).all():
        fails.append("not finite")
    bound = row_bound(row)
    err = float((got.cpu().double() - want).abs().max()) / scale
    print("SAFORM %s | %s | err %.3g = %.3f of the bound %.0e, %.2f y32 (y32 %.3g)" % (
        row_id(row), expect, err, err / bound, bound, err / y32, y32))
    if arith != R.PREC[expect.split(" ")[0]]:
        fails.append("ran in arithmetic %d, the dispatcher's rule says %s" % (arith, expect))
    if not err <= bound:
        fails.append("err %.3g of scale > bound %.3g (float32 torch: %.3g)" % (err, bound, y32))
    if not torch.equal(got, again):
        fails.append("two launches differ")
    if not (pm.transpose(1, 2).is_contiguous() and torch.equal(got, pm)):
        fails.append("channel-major and point-major output differ")
    for b, o in alone.items():
        if not torch.equal(o[0], got[b]):
            fails.append("cloud %d alone differs from the cloud in its batch" % b)
    if from_idx is not None and not torch.equal(from_idx, got):
        fails.append("row table and index tensor give different bits")
    if krow is not None:
        # the K-row evaluation of the same call: the maximum over all K entries is the maximum over the first cnt
        kexp = R.dispatch(mode, D, w[0], w[1], w[2], K, R.PREC[prec], False, bool(fast))
        kbound = row_bound(row[:10] + (R.form_name(kexp),))
        kerr = float((krow.cpu().double() - want).abs().max()) / scale
        print("SAFORM %s | K-row twin %s | err %.3g = %.3f of the bound %.0e | bit-equal %s, arithmetic %d / %d" % (
            row_id(row), R.form_name(kexp), kerr, kerr / kbound, kbound, torch.equal(krow, got), arith, arith_k))
        if arith_k != kexp[0]:
            fails.append("the K-row twin ran in arithmetic %d, the rule says %s" % (arith_k, R.form_name(kexp)))
        if not kerr <= kbound:
            fails.append("K-row twin: err %.3g of scale > bound %.3g" % (kerr, kbound))
        if arith_k == arith and not torch.equal(krow, got):
            fails.append("ragged and K-row evaluation differ in the same arithmetic (max |d| %.3g of scale)" % (
                float((krow - got).abs().max()) / scale))
    assert not fails, "; ".join(fails)
