"""Host side of the training-mode kernels (include/pcr.h section C; csrc/train_kernels.hip, train_sa_kernels.hip):
ctypes parameter blocks, launches, and the torch.autograd.Functions that put them under `loss.backward()`.

What runs where: every dense layer of the training graph -- the grouped set-abstraction MLPs with BatchNorm in
batch-statistics mode (reference pointnet2_utils.py:333-360), the per-point tables of their first layer, the attention
projections / feed-forward layers and the match head -- is a HIP launch forward and a HIP launch backward on the
matrix core; autograd only strings the Functions together.  Nothing here has a CPU path.  The packed weight images the
launches read, and their cache, are pcr_amd/train_pack.py's.
"""
import ctypes
import os

import torch
from torch.autograd import Function

from . import _lib as L
from ._lib import _c32, _f32, _p
from .abi import _AttnHeadP, _AttnTailP, _BnBwd, _BnFwd, _LinAttnP, _ReduceJob, _TBwd, _TFwd
from .engine import _prof
from .train_pack import (_PAD_CACHE, _PREPACKS, _Prepack, _dev, _lookup, pack_bf_T, pack_both, pack_both_bf,  # noqa: F401
                         pack_dev, pad32, prepack)

FUSE_POOL = True       # SaEdgeTrain: take the max over K inside the last layer's launch where the library offers it


# ------------------------------------------------------------------------------------------- launches --
def tdense_fwd(x, wp, cout, x2=None, isc=None, ish=None, in_relu=False, bias=None, res=None, out_relu=False,
               want_stats=False, pool=None):
    """-> (y, stats partials or None[, (ymax, argmax) or None when `pool` = (K, gamma) is given: the fused max over the K
    rows of every centre, where the launch can provide it (pcr_tdense_fwd_pooled)])"""
    x = _dev(x)
    B, cin1, Ln = x.shape
    cin2 = 0
    if x2 is not None:
        x2 = _dev(x2)
        cin2 = x2.shape[1]
    y = _f32(B, cout, Ln, device=x.device)
    p = _TFwd()
    p.B, p.cin1, p.cin2, p.cout, p.L = B, cin1, cin2, cout, Ln
    p.x, p.x2, p.isc, p.ish, p.in_relu = _p(x), _p(x2), _p(isc), _p(ish), int(in_relu)
    p.wp, p.bias, p.res, p.out_relu = _p(wp), _p(pad32(bias, cout)), _p(res), int(out_relu)
    p.y = _p(y)
    # rows of the statistics partials = workgroups of THIS launch (the library picks the kernel from the block)
    pooled = None
    if pool is not None:
        K, gamma = pool
        S = Ln // K
        ymax = _f32(B, cout, S, device=x.device)
        arg = torch.empty((B, cout, S), dtype=torch.int32, device=x.device)
        p.pool_K, p.pool_gamma, p.pool_ymax, p.pool_arg = K, _p(gamma.detach()), _p(ymax), _p(arg)
        if L.load().pcr_tdense_fwd_pooled(ctypes.byref(p)):
            pooled = (ymax, arg)
        else:
            p.pool_K = 0
    stats = _f32(L.load().pcr_tdense_fwd_groups(ctypes.byref(p)), 2, _c32(cout), device=x.device) if want_stats else None
    p.stats = _p(stats)
    cin = cin1 + cin2
    with _prof("tdense_fwd[cin=%d,cout=%d,L=%d]" % (cin, cout, Ln), 2.0 * B * Ln * cin * cout,
               4.0 * B * Ln * (cin + cout * (2 if res is not None else 1)), arith="lib"):
        L.run.pcr_tdense_fwd_f32(ctypes.byref(p), L.stream_ptr())
    if pool is not None:
        return y, stats, pooled
    return y, stats


def reduce_parts(part, nparts, stride, rows, cols, ld):
    out = _f32(rows, cols, device=part.device)
    L.run.pcr_reduce_parts_f32(part, nparts, stride, rows, cols, ld, out, L.stream_ptr())
    return out


# ---- partial-sum reductions -------------------------------------------------------------------------------------------
# A backward launch leaves per-workgroup partial records (weight / bias / norm gradients side by side); ONE launch
# (pcr_reduce_multi_f32) sums every region of the record into its own compact tensor -- no padded views, so autograd's
# AccumulateGrad takes the gradients as they are instead of cloning them.  (Tried in round 5 and removed: deferring all
# reductions of a backward pass to one launch at its end through an autograd-engine callback.  It measured no faster --
# the cost is the bytes of the partial records, not the ~35 launches -- and it is only safe for a parameter used ONCE in
# the graph: a second use makes the engine add the still-unreduced buffer.)
def reduce_regions(part, nparts, stride, regions):
    """regions [(offset in floats, rows, cols, ld)] of every partial record -> compact (rows, cols) tensors, summed over the
    nparts records (increasing record order, fixed: bit-reproducible)"""
    dev = part.device
    outs = [_f32(rows, cols, device=dev) for _, rows, cols, _ in regions]
    jobs = [_ReduceJob(part.data_ptr() + 4 * off, o.data_ptr(), stride, nparts, rows, cols, ld)
            for (off, rows, cols, ld), o in zip(regions, outs)]
    arr = (_ReduceJob * len(jobs))(*jobs)
    L.run.pcr_reduce_multi_f32(arr, len(jobs), L.stream_ptr())
    return outs


# Arithmetic of the training launches' matrix phases:
#   "f32"         f32-input MFMA, exact fmaf chains everywhere;
#   "bf16x3"      (default) split bf16 on the bf16 matrix core (three MFMAs per product, f32 accumulation) for the
#                 GRADIENT products only -- dx and dW of the 128 x 128 grouped-MLP layers (pcr_tdense_bwd.precision) and of
#                 the fused attention chains (pcr_attn_tail / pcr_attn_head .precision); every forward value, and with it
#                 every ReLU mask and max-pool winner, is the f32 graph's;
#   "bf16x3_all"  opt-in: the fused chains' forward (and its recomputation) as split bf16 too.  ~0.3 ms per pt128_train
#                 step faster, and ~1 ReLU in 10^5 whose argument lies within 1e-5 of zero opens where the f32 graph keeps
#                 it shut: that token's gradient row moves by per cent, a weight gradient by ~1e-4 of its scale.
# PCR_TRAIN_PRECISION in the environment or set_train_precision() select it.
_TRAIN_PRECISIONS = ("f32", "bf16x3", "bf16x3_all")
TRAIN_PRECISION = os.environ.get("PCR_TRAIN_PRECISION", "bf16x3")
if TRAIN_PRECISION not in _TRAIN_PRECISIONS:
    raise L.PcrError("PCR_TRAIN_PRECISION must be one of %s" % (_TRAIN_PRECISIONS,))


def set_train_precision(name):
    """-> previous setting"""
    global TRAIN_PRECISION
    if name not in _TRAIN_PRECISIONS:
        raise L.PcrError("training precision must be one of %s" % (_TRAIN_PRECISIONS,))
    prev, TRAIN_PRECISION = TRAIN_PRECISION, name
    return prev


def _bwd_bf():
    return TRAIN_PRECISION != "f32"


def tdense_bwd(g, x, cout, dy_mode=0, y=None, k=None, argmax=None, pooled=None, K=0, S=0, x2=None, isc=None, ish=None,
               iinv=None, in_relu=False, wpT=None, want_dstats=False, want_dw=True, wpT_bf=None):
    """-> dict(dx, dx2, dstats, dW (cout, cin1+cin2), db (cout)); see pcr_tdense_bwd in include/pcr.h"""
    x = _dev(x)
    B, cin1, Ln = x.shape
    cin2 = 0
    if x2 is not None:
        x2 = _dev(x2)
        cin2 = x2.shape[1]
    cin = cin1 + cin2
    dev = x.device
    out = {}
    p = _TBwd()
    p.B, p.cin1, p.cin2, p.cout, p.L = B, cin1, cin2, cout, Ln
    p.g, p.y, p.dy_mode = _p(g), _p(y), dy_mode
    if k is not None:
        p.ka, p.kb, p.kc = _p(k["ka"]), _p(k["kb"]), _p(k["kc"])
    p.argmax, p.pooled, p.K, p.S = _p(argmax), _p(pooled), K, S
    p.x, p.x2, p.isc, p.ish, p.iinv, p.in_relu = _p(x), _p(x2), _p(isc), _p(ish), _p(iinv), int(in_relu)
    # workgroups of THIS launch = rows of its partial buffers: asked with the wanted outputs marked non-NULL (the
    # library picks the kernel -- and with it the grid -- from the parameter block), then the real buffers go in
    p.wpT = _p(wpT)
    if wpT_bf is not None and _bwd_bf():
        p.wpT_bf, p.precision = _p(wpT_bf), 1
    if wpT is not None:
        p.dx, p.dx2 = 1, (1 if cin2 else None)
        p.dstats = 1 if want_dstats else None
    if want_dw:
        p.dwp = p.dbp = 1
        p.part_stride = _c32(cout) * _c32(cin) + _c32(cout)
    nwg = L.load().pcr_tdense_bwd_groups(ctypes.byref(p))
    p.dx = p.dx2 = p.dstats = p.dwp = p.dbp = None
    if wpT is not None:
        out["dx"] = _f32(B, cin1, Ln, device=dev)
        out["dx2"] = _f32(B, cin2, Ln, device=dev) if cin2 else None
        p.wpT, p.dx, p.dx2 = _p(wpT), _p(out["dx"]), _p(out["dx2"])
        if want_dstats:
            out["dstats"] = _f32(nwg, 2, _c32(cin1), device=dev)
            p.dstats = _p(out["dstats"])
    coutP, cinP = _c32(cout), _c32(cin)
    if want_dw:
        # per workgroup: the dW image (coutP x cinP) followed by db (coutP); ONE reduction over both
        per = coutP * cinP + coutP
        parts = _f32(nwg, per, device=dev)
        p.dwp, p.dbp, p.part_stride = _p(parts), parts.data_ptr() + 4 * coutP * cinP, per
    # algorithmic work: dW = dy f(x)^T and dx = W^T dy (2 B L cout cin flops each); bytes: read g (or the small pooled
    # tensors in mode 3), y (BatchNorm / ReLU modes), x; write dx
    flops = 2.0 * B * Ln * cout * cin * ((1 if want_dw else 0) + (1 if wpT is not None else 0))
    nbytes = 4.0 * B * Ln * ((cout if dy_mode != 3 else 0) + (cout if dy_mode != 0 else 0) + cin +
                             (cin if wpT is not None else 0))
    with _prof("tdense_bwd[mode=%d,cin=%d,cout=%d,L=%d]" % (dy_mode, cin, cout, Ln), flops, nbytes, arith="lib"):
        L.run.pcr_tdense_bwd_f32(ctypes.byref(p), L.stream_ptr())
    if want_dw:
        dW, db = reduce_regions(parts, nwg, per, [(0, cout, cin, cinP), (coutP * cinP, 1, cout, cout)])
        out["dW"], out["db"] = dW, db.view(cout)
    return out


def bn_fwd_finalize(part, nparts, C, R, gamma, beta, eps, momentum, running_mean=None, running_var=None, shift0=None,
                    shift0_stride=1):
    dev = part.device
    o = {k: _f32(C, device=dev) for k in ("scale", "shift", "inv_scale", "mean", "invstd")}
    p = _BnFwd()
    p.part, p.nparts, p.C, p.R = _p(part), nparts, C, float(R)
    p.gamma, p.beta, p.eps, p.momentum = _p(gamma.detach()), _p(beta.detach()), eps, momentum
    p.running_mean, p.running_var = _p(running_mean), _p(running_var)
    p.shift0, p.shift0_stride = _p(shift0), shift0_stride
    for k, v in o.items():
        setattr(p, k, _p(v))
    L.run.pcr_bn_fwd_finalize_f32(ctypes.byref(p), L.stream_ptr())
    return o


def bn_bwd_finalize(part, nparts, C, R, gamma, mean, invstd, centre=None):
    dev = part.device
    o = {k: _f32(C, device=dev) for k in ("ka", "kb", "kc", "dgamma", "dbeta")}
    p = _BnBwd()
    p.part, p.nparts, p.C, p.R = _p(part), nparts, C, float(R)
    p.gamma, p.mean, p.invstd = _p(gamma.detach()), _p(mean), _p(invstd)
    p.centre = _p(centre)
    for k, v in o.items():
        setattr(p, k, _p(v))
    L.run.pcr_bn_bwd_finalize_f32(ctypes.byref(p), L.stream_ptr())
    return o


def _bn_nparts(B, C):
    """rows of the partial sums pcr_bn_sums_f32 leaves over (B, C, L); a backward uses the value of its forward"""
    return max(1, min(B, 2048 // max(C, 1)))


def _require_batch(R, shape):
    """torch's training-mode BatchNorm refuses a single value per channel (there is no variance to normalise by); so
    does this path, before any launch, rather than return beta and update the running statistics"""
    if R <= 1:
        raise L.PcrError("Expected more than 1 value per channel when training, got input size %s" % (tuple(shape),))


def _bn_refuse(*bns):
    for bn in bns:
        if bn.momentum is None:
            # nn.BatchNorm2d(momentum=None) is the cumulative average 1 / num_batches_tracked (a device counter: a
            # host read per layer and step); no reference config uses it -- refused rather than approximated
            raise L.PcrError("BatchNorm with momentum=None (cumulative average) is not supported by the HIP training path")


def _bn_batch_step(part, nparts, C, R, gamma, beta, bn, shift0=None, shift0_stride=1):
    """The batch-statistics step of module `bn` (an nn.BatchNorm*d in training mode), the one copy of it: the refusal
    (a Function with launches in front of this step calls _bn_refuse itself, ahead of them), pcr_bn_fwd_finalize over
    the partial sums of R values per channel, the running statistics updated in place as the module does"""
    _bn_refuse(bn)
    track = bn.track_running_stats
    o = bn_fwd_finalize(part, nparts, C, R, gamma, beta, bn.eps, bn.momentum, bn.running_mean if track else None,
                        bn.running_var if track else None, shift0=shift0, shift0_stride=shift0_stride)
    if track:
        # (written through raw pointers by the finalize launch: keep Tensor._version honest for the caches)
        torch.autograd.graph.increment_version([bn.running_mean, bn.running_var])
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked += 1
    return o


# ----------------------------------------------------------------------------------- autograd Functions --
class TDense(Function):
    """y = [relu](W [x ; x2] + bias [+ res]) on (B,C,L) tensors; W (cout, cin1+cin2) row-major (nn.Linear / 1x1 conv)"""

    @staticmethod
    def forward(ctx, x, x2, W, bias, res, out_relu):
        cout = W.shape[0]
        need_dx = x.requires_grad or (x2 is not None and x2.requires_grad)
        wp, wpT = pack_both(W) if need_dx else (pack_dev(W), None)
        y, _ = tdense_fwd(x, wp, cout, x2=x2, bias=bias, res=res, out_relu=out_relu)
        ctx.save_for_backward(x, x2, W, y if out_relu else None, wpT)
        ctx.meta = (out_relu, bias is not None, res is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, x2, W, y, wpT = ctx.saved_tensors
        out_relu, has_bias, has_res = ctx.meta
        g = g.contiguous()
        need_dx = ctx.needs_input_grad[0] or (x2 is not None and ctx.needs_input_grad[1])
        if need_dx and wpT is None:
            wpT = pack_dev(W, transpose=True)
        r = tdense_bwd(g, x, W.shape[0], dy_mode=2 if out_relu else 0, y=y, x2=x2,
                       wpT=wpT if need_dx else None,
                       want_dw=ctx.needs_input_grad[2] or (has_bias and ctx.needs_input_grad[3]))
        g_res = None
        if has_res and ctx.needs_input_grad[4]:
            # relu(W x + res): the residual sees the gradient through the same mask (only the wide-layer tiling below
            # builds this combination; one elementwise select)
            g_res = torch.where(y > 0, g, torch.zeros((), dtype=g.dtype, device=g.device)) if out_relu else g
        return (r.get("dx"), r.get("dx2"), r.get("dW"), r.get("db") if has_bias else None, g_res, None)


# pcr_tdense_{fwd,bwd}_f32 take up to 384 output rows and 288 input rows per launch, and the backward less than that
# rectangle: it keeps dy and the forward input of a 64-token tile in LDS together (`bwd_fits`, the rule of include/pcr.h),
# which excludes the corner from (384, 224) / (320, 288) on.  Wider layers -- the 256-channel attention blocks and 512-row
# feed-forward / table layers of the mul = 2 Point-Transformer -- and the layers of that corner run as a grid of launches:
# output rows in chunks, input rows in chunks chained through the launch's residual input; autograd sees ordinary
# Functions, so the backward tiles the same way.
_MAX_COUT, _MAX_CIN, _CHUNK = 384, 288, 256
_BWD_LDS, _TILE_PITCH = 160 * 1024, 65


def bwd_fits(cout, cin, cin1):
    """whether pcr_tdense_bwd_f32 takes a (cout, cin = cin1 + cin2) layer in ONE launch: its LDS rule
    ((max(ceil32(cout), ceil32(cin)) + ceil32(cin)) 65 + 3 cout + 3 cin1) 4 <= 160 KiB inside cout <= 384, cin <= 288"""
    coutP, cinP = _c32(cout), _c32(cin)
    return cout <= _MAX_COUT and cin <= _MAX_CIN and \
        ((max(coutP, cinP) + cinP) * _TILE_PITCH + 3 * cout + 3 * cin1) * 4 <= _BWD_LDS


def _trains(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def dense(x, W, bias=None, x2=None, res=None, relu=False):
    cout, cin = W.shape
    # (the shapes the backward takes too -- every layer of the models -- pay a few integer operations here; a forward
    # that no backward will follow needs the forward's limits only)
    if cout <= _MAX_COUT and cin <= _MAX_CIN and not (relu and res is not None) and \
            (bwd_fits(cout, cin, x.shape[1]) or not _trains(x, x2, W, bias, res)):
        return TDense.apply(x, x2, W, bias, res, relu)
    segs = [x] if x2 is None else [x, x2]             # input = the channel concatenation of the segments
    pieces, c0 = [], 0                                # (tensor, first column of W)
    for t in segs:
        for a in range(0, t.shape[1], _CHUNK):
            b = min(t.shape[1], a + _CHUNK)
            pieces.append((t if (a == 0 and b == t.shape[1]) else t[:, a:b].contiguous(), c0 + a, c0 + b))
        c0 += t.shape[1]
    assert c0 == cin, "dense: input width %d != weight width %d" % (c0, cin)
    outs = []
    for o0 in range(0, cout, _CHUNK):
        o1 = min(cout, o0 + _CHUNK)
        acc = None if res is None else (res if (o0 == 0 and o1 == cout) else res[:, o0:o1].contiguous())
        for i, (t, a, b) in enumerate(pieces):
            last = i == len(pieces) - 1
            acc = TDense.apply(t, None, W[o0:o1, a:b], bias[o0:o1] if (bias is not None and i == 0) else None, acc,
                               relu and last)
        outs.append(acc)
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


def _sa_mlp_fwd(ctx, xyz, idx, centre, tab, wa, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, bns):
    """The one forward of the grouped MLP in training mode (SaEdgeTrain and SaGroupTrain): layer 1 from the per-point
    table, three (conv, BatchNorm over the B S K rows, ReLU) layers, max over K.  centre None: the first S points are the
    centres and tab is [P ; Q] (pcr_sa_l1_fwd_f32); centre (B,S) int32: indexed centres, tab = P (pcr_sa_l1c_fwd_f32).
    A bias may be None (a conv built without one)."""
    xyz, idx = _dev(xyz), idx.contiguous()
    L.require_i32(idx)
    B, N, _ = xyz.shape
    _, S, K = idx.shape
    Ln = S * K
    R = B * Ln
    c1, c2, c3 = wa.shape[0], w2.shape[0], w3.shape[0]
    dev = xyz.device
    tab = None if tab is None else _dev(tab)
    _bn_refuse(*bns)                                  # (all three, before the first layer's statistics are tracked)
    y1 = _f32(B, c1, Ln, device=dev)
    st1 = _f32(B, 2, _c32(c1), device=dev)
    b1d = None if b1 is None else b1.detach()
    if centre is None:
        with _prof("sa_l1_fwd[c1=%d,N=%d,S=%d,K=%d]" % (c1, N, S, K), 8.0 * B * Ln * c1, 4.0 * B * (Ln * (c1 + 1) + 2 * c1 * N)):
            L.run.pcr_sa_l1_fwd_f32(xyz, idx, tab, _dev(wa.detach()), b1d, y1, st1, B, N, S, K, c1, L.stream_ptr())
    else:
        centre = centre.contiguous()
        L.require_i32(centre)
        if tuple(centre.shape) != (B, S):
            raise L.PcrError("centre indices must be (B, S) = (%d, %d), got %s" % (B, S, tuple(centre.shape)))
        with _prof("sa_l1c_fwd[c1=%d,N=%d,S=%d,K=%d]" % (c1, N, S, K), 8.0 * B * Ln * c1, 4.0 * B * (Ln * (c1 + 1) + c1 * N)):
            L.run.pcr_sa_l1c_fwd_f32(xyz, idx, centre, tab, _dev(wa.detach()), b1d, y1, st1, B, N, S, K, c1,
                                     L.stream_ptr())
    n1 = _bn_batch_step(st1, B, c1, R, g1, be1, bns[0])
    y2, st2 = tdense_fwd(y1, pack_dev(w2), c2, isc=n1["scale"], ish=n1["shift"], in_relu=True, bias=b2, want_stats=True)
    n2 = _bn_batch_step(st2, st2.shape[0], c2, R, g2, be2, bns[1])
    # the last layer's launch also finds every centre's winning row where it can (max of the raw output for
    # gamma >= 0, min otherwise: relu(scale y + shift) is monotone in y); the pooled activation is then one affine +
    # ReLU over the (B,c3,S) winners instead of a second pass over the (B,c3,S K) tensor
    y3, st3, *won = tdense_fwd(y2, pack_dev(w3), c3, isc=n2["scale"], ish=n2["shift"], in_relu=True, bias=b3,
                               want_stats=True, pool=(K, g3) if FUSE_POOL else None)
    won = won[0] if won else None                     # (tdense_fwd returns the third value only where it was asked)
    n3 = _bn_batch_step(st3, st3.shape[0], c3, R, g3, be3, bns[2])
    pooled = _f32(B, c3, S, device=dev)
    if won is not None:
        ymax, argmax = won
        L.run.pcr_bn_affine_f32(ymax, None, n3["scale"], n3["shift"], None, None, None, None, 1, 0.0, pooled, B,
                                c3, S, L.stream_ptr())
    else:
        argmax = torch.empty((B, c3, S), dtype=torch.int32, device=dev)
        ymax = _f32(B, c3, S, device=dev)
        with _prof("sa_pool_fwd[c=%d,S=%d,K=%d]" % (c3, S, K), 2.0 * B * Ln * c3, 4.0 * B * c3 * (Ln + 2 * S)):
            L.run.pcr_sa_pool_fwd_f32(y3, n3["scale"], n3["shift"], pooled, argmax, ymax, B, c3, S, K,
                                      L.stream_ptr())
    ctx.save_for_backward(xyz, idx, y1, y2, y3, pooled, argmax, w2, w3, g1, g2, g3, ymax, centre)
    ctx.norms = (n1, n2, n3)
    ctx.has_tab = tab is not None
    ctx.has_bias = (b1 is not None, b2 is not None, b3 is not None)
    ctx.dims = (B, N, S, K, c1, c2, c3)
    ctx.mark_non_differentiable(argmax)
    return pooled


def _sa_mlp_bwd(ctx, gp):
    """-> (dtab, dwa, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3, dg3, dbe3); a bias that was None gets None"""
    xyz, idx, y1, y2, y3, pooled, argmax, w2, w3, g1, g2, g3, ymax, centre = ctx.saved_tensors
    n1, n2, n3 = ctx.norms
    B, N, S, K, c1, c2, c3 = ctx.dims
    Ln, R, dev = S * K, B * S * K, xyz.device
    gp = gp.contiguous()
    part3 = _f32(B, 2, _c32(c3), device=dev)
    gz = _f32(B, c3, S, device=dev)          # the pooled gradient where the ReLU is open, zero elsewhere
    L.run.pcr_sa_pool_bwd_stats_f32(gp, pooled, ymax, part3, gz, B, c3, S, L.stream_ptr())
    k3 = bn_bwd_finalize(part3, B, c3, R, g3, n3["mean"], n3["invstd"])
    # (128 x 128 layers: dx and dW on the bf16 matrix core when TRAIN_PRECISION says so)
    bf3 = pack_bf_T(w3) if (_bwd_bf() and c3 == 128 and c2 == 128) else None
    bf2 = pack_bf_T(w2) if (_bwd_bf() and c2 == 128 and c1 == 128) else None
    r3 = tdense_bwd(gz, y2, c3, dy_mode=3, y=y3, k=k3, argmax=argmax, pooled=None, K=K, S=S,
                    isc=n2["scale"], ish=n2["shift"], iinv=n2["inv_scale"], in_relu=True,
                    wpT=pack_dev(w3, transpose=True), want_dstats=True, wpT_bf=bf3)
    k2 = bn_bwd_finalize(r3["dstats"], r3["dstats"].shape[0], c2, R, g2, n2["mean"], n2["invstd"])
    r2 = tdense_bwd(r3["dx"], y1, c2, dy_mode=1, y=y2, k=k2, isc=n1["scale"], ish=n1["shift"], iinv=n1["inv_scale"],
                    in_relu=True, wpT=pack_dev(w2, transpose=True), want_dstats=True, wpT_bf=bf2)
    k1 = bn_bwd_finalize(r2["dstats"], r2["dstats"].shape[0], c1, R, g1, n1["mean"], n1["invstd"])
    dwa_p = _f32(B, c1, 4, device=dev)
    if centre is None:
        dtab = _f32(B, 2 * c1, N, device=dev) if ctx.has_tab else None
        with _prof("sa_l1_bwd[c1=%d,N=%d,S=%d,K=%d]" % (c1, N, S, K), 10.0 * B * Ln * c1, 4.0 * B * (Ln * (2 * c1 + 1) + 2 * c1 * N)):
            L.run.pcr_sa_l1_bwd_f32(xyz, idx, r2["dx"], y1, k1["ka"], k1["kb"], k1["kc"], dtab, dwa_p, B, N, S, K, c1,
                                    L.stream_ptr())
    else:
        dtab = _f32(B, c1, N, device=dev) if ctx.has_tab else None
        with _prof("sa_l1c_bwd[c1=%d,N=%d,S=%d,K=%d]" % (c1, N, S, K), 10.0 * B * Ln * c1, 4.0 * B * (Ln * (2 * c1 + 1) + c1 * N)):
            L.run.pcr_sa_l1c_bwd_f32(xyz, idx, centre, r2["dx"], y1, k1["ka"], k1["kb"], k1["kc"], dtab, dwa_p, B, N, S,
                                     K, c1, L.stream_ptr())
    dwa4 = reduce_parts(dwa_p, B, c1 * 4, c1, 4, 4)
    hb = ctx.has_bias
    return (dtab, dwa4[:, :3].contiguous(), dwa4[:, 3].contiguous() if hb[0] else None, k1["dgamma"], k1["dbeta"],
            r2["dW"], r2["db"] if hb[1] else None, k2["dgamma"], k2["dbeta"],
            r3["dW"], r3["db"] if hb[2] else None, k3["dgamma"], k3["dbeta"])


class SaEdgeTrain(Function):
    """Grouped edge MLP of one set-abstraction layer in TRAINING mode: layer 1 from per-point tables, three
    (conv, BatchNorm over the batch, ReLU) layers, max over K.  Inputs: xyz (B,N,3), idx (B,S,K) int32, tab (B,2c1,N)
    or None, then per layer (W, b, gamma, beta); `bns` = the three nn.BatchNorm2d modules (running statistics are
    updated in place, as nn.BatchNorm2d does in training mode).  -> pooled (B,c3,S)."""

    @staticmethod
    def forward(ctx, xyz, idx, tab, wa, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, bns):
        return _sa_mlp_fwd(ctx, xyz, idx, None, tab, wa, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, bns)

    @staticmethod
    def backward(ctx, gp):
        return (None, None) + _sa_mlp_bwd(ctx, gp) + (None,)


class SaGroupTrain(Function):
    """Grouped MLP of one ball-query scale of a PointSAModule in TRAINING mode (QueryAndGroup with use_xyz + three
    ConvModules + max over K).  Rows are [xyz_i - xyz_centre, f_i]; centre (B,S) int32 holds the sampled centres' point
    indices; rows k >= cnt of a centre are the ball query's copies of its row 0 and count in the batch statistics and
    in every gradient, as they do in nn.BatchNorm2d over (B,C,S,K).  tab (B,c1,N) = Wf f or None; a conv bias may be
    None.  -> pooled (B,c3,S).  Same body as SaEdgeTrain; the first-layer launches are pcr_sa_l1c_*."""

    @staticmethod
    def forward(ctx, xyz, idx, centre, tab, wa, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, bns):
        if centre is None:
            raise L.PcrError("SaGroupTrain needs the centres' point indices")
        return _sa_mlp_fwd(ctx, xyz, idx, centre, tab, wa, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, bns)

    @staticmethod
    def backward(ctx, gp):
        return (None, None, None) + _sa_mlp_bwd(ctx, gp) + (None,)


def sa_edge_train(sa, xyz, feats, idx):
    """PointNetSetAbstractionEdgeSA's grouped MLP + max in training mode: xyz (B,N,3), feats (B,D,N) or None,
    idx (B,S,K) -> (B,c3,S).  The first conv's weight [Wa | Wc | Wf] is split here; autograd carries the table
    weights' gradient back into it."""
    convs, bns = list(sa.mlp_convs), list(sa.mlp_bns)
    c1 = convs[0].weight.shape[0]
    w1 = convs[0].weight.view(c1, -1)
    wa = w1[:, :3]
    tab = None
    if feats is not None:
        D = feats.shape[1]
        wc, wf = w1[:, 3:3 + D], w1[:, 3 + D:3 + 2 * D]
        tab = dense(feats, torch.cat([wf, wc - wf], dim=0))          # (B, 2 c1, N): [P ; Q]
    args = [xyz, idx, tab, wa, convs[0].bias, bns[0].weight, bns[0].bias]
    for l in (1, 2):
        args += [convs[l].weight.view(convs[l].weight.shape[0], -1), convs[l].bias, bns[l].weight, bns[l].bias]
    return SaEdgeTrain.apply(*args, bns)


def sa_group_train(mlp, xyz, feats, idx, centre):
    """One ball-query scale of a PointSAModule in training mode: mlp = its nn.Sequential of three ConvModules (conv, bn,
    ReLU), xyz (B,N,3) (no gradient), feats (B,D,N) or None, idx (B,S,K) int32 from ball_query, centre (B,S) int32 the
    sampled centres -> (B,c3,S).  The first conv's weight [Wa | Wf] is split here and P = Wf f is one dense layer over
    the N points; the gradient reaches feats and Wf through dtab."""
    layers = list(mlp.children())
    convs, bns = [l.conv for l in layers], [l.bn for l in layers]
    c1 = convs[0].weight.shape[0]
    w1 = convs[0].weight.view(c1, -1)
    D = 0 if feats is None else feats.shape[1]
    if w1.shape[1] != 3 + D:
        raise L.PcrError("the first conv takes %d channels; the rows [dxyz, f] have 3 + %d" % (w1.shape[1], D))
    tab = dense(feats.contiguous(), w1[:, 3:].contiguous()) if D else None     # (B, c1, N): P
    args = [xyz.detach(), idx, centre, tab, w1[:, :3], convs[0].bias, bns[0].weight, bns[0].bias]
    for l in (1, 2):
        args += [convs[l].weight.view(convs[l].weight.shape[0], -1), convs[l].bias, bns[l].weight, bns[l].bias]
    return SaGroupTrain.apply(*args, bns)


# ---------------------------------------------------------------- attention / norm / pooling Functions --
def _block(t, d):
    """(pointer, batch stride) of a (B,d,L) channel-major block that may be a channel slice of a wider tensor"""
    assert t.dim() == 3 and t.shape[1] == d and t.stride(2) == 1 and t.stride(1) == t.shape[2], \
        "attention operands must be channel slices of contiguous (B,C,L) tensors"
    return t.data_ptr(), t.stride(0)


def _linattn_fwd(q, k, v, H, eps, kv_roll=0):
    L.require_cuda(q, k, v)
    B, d, Lq = q.shape
    Sk = k.shape[2]
    dev = q.device
    out = _f32(B, d, Lq, device=dev)
    A = _f32(B, H, d // H, d // H, device=dev)
    ks = _f32(B, H, d // H, device=dev)
    p = _LinAttnP()
    p.B, p.Lq, p.Sk, p.d, p.H, p.eps, p.kv_roll = B, Lq, Sk, d, H, eps, kv_roll
    (p.q, p.q_bs), (p.k, p.k_bs), (p.v, p.v_bs) = _block(q, d), _block(k, d), _block(v, d)
    p.out, p.A, p.ks = _p(out), _p(A), _p(ks)
    L.run.pcr_linattn_fwd_f32(ctypes.byref(p), L.stream_ptr())
    return out, A, ks


def _linattn_bwd(q, k, v, A, ks, g, dq, dk, dv, H, eps, kv_roll=0):
    B, d, Lq = q.shape
    p = _LinAttnP()
    p.B, p.Lq, p.Sk, p.d, p.H, p.eps, p.kv_roll = B, Lq, k.shape[2], d, H, eps, kv_roll
    (p.q, p.q_bs), (p.k, p.k_bs), (p.v, p.v_bs) = _block(q, d), _block(k, d), _block(v, d)
    p.A, p.ks, p.dout = _p(A), _p(ks), _p(g)
    (p.dq, p.dq_bs), (p.dk, p.dk_bs), (p.dv, p.dv_bs) = _block(dq, d), _block(dk, d), _block(dv, d)
    L.run.pcr_linattn_bwd_f32(ctypes.byref(p), L.stream_ptr())


class LinAttn(Function):
    """LinearAttention (pointnet2_utils.py:26-47) on channel-major tensors: q (B,d,Lq), k, v (B,d,Sk) -> (B,d,Lq)"""

    @staticmethod
    def forward(ctx, q, k, v, H, eps):
        out, A, ks = _linattn_fwd(q, k, v, H, eps)
        ctx.save_for_backward(q, k, v, A, ks)
        ctx.meta = (H, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, A, ks = ctx.saved_tensors
        H, eps = ctx.meta
        dq, dk, dv = torch.empty_like(q, memory_format=torch.contiguous_format), \
            torch.empty_like(k, memory_format=torch.contiguous_format), torch.empty_like(v, memory_format=torch.contiguous_format)
        _linattn_bwd(q, k, v, A, ks, g.contiguous(), dq, dk, dv, H, eps)
        return dq, dk, dv, None, None


class LinAttnQKV(Function):
    """the same on ONE fused projection qkv (B,3d,L) = [q ; k ; v] (self-attention): the kernels address the three
    channel blocks by a batch stride, and the gradient comes back as one (B,3d,L) buffer -- no slice / pad / add nodes
    in the autograd graph"""

    @staticmethod
    def forward(ctx, qkv, H, eps, kv_roll=0):
        """kv_roll: query cloud b attends to the keys / values of cloud (b + kv_roll) % B of the same buffer (the matching
        stages: every cloud against its pair partner, ReIDNet.py:231-247) -- no rolled copy of the batch"""
        qkv = _dev(qkv)
        d = qkv.shape[1] // 3
        out, A, ks = _linattn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], H, eps, kv_roll)
        ctx.save_for_backward(qkv, A, ks)
        ctx.meta = (H, eps, kv_roll)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, A, ks = ctx.saved_tensors
        H, eps, kv_roll = ctx.meta
        d = qkv.shape[1] // 3
        buf = torch.empty_like(qkv)
        _linattn_bwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], A, ks, g.contiguous(),
                     buf[:, :d], buf[:, d:2 * d], buf[:, 2 * d:], H, eps, kv_roll)
        return buf, None, None, None


class LocalAttn(Function):
    """core of local_self_attention in training mode (attention.py:262-296): qkv (B,3C,N) = the fused q | k | v
    projection per POINT, idx (B,N,K) int32 feature-space neighbours (no gradient) -> msg (B,C,N); the backward's
    per-edge gradients are folded onto the points by the grouping backward (owner-computes, no float atomics)"""

    @staticmethod
    def forward(ctx, qkv, idx, H, eps):
        qkv, idx = _dev(qkv), idx.contiguous()
        L.require_i32(idx)
        B, C3, N = qkv.shape
        C, K = C3 // 3, idx.shape[2]
        msg = _f32(B, C, N, device=qkv.device)
        L.run.pcr_local_attn_train_fwd_f32(qkv, idx, msg, B, N, C, K, H, eps, L.stream_ptr())
        ctx.save_for_backward(qkv, idx)
        ctx.meta = (H, eps)
        return msg

    @staticmethod
    def backward(ctx, g):
        qkv, idx = ctx.saved_tensors
        H, eps = ctx.meta
        B, C3, N = qkv.shape
        C, K = C3 // 3, idx.shape[2]
        g = g.contiguous()
        dqkv = torch.zeros((B, 3 * C, N), dtype=torch.float32, device=qkv.device)      # (k | v rows: accumulated into)
        edge = _f32(B, 2 * C, N, K, device=qkv.device)
        L.run.pcr_local_attn_train_bwd_f32(qkv, idx, g, dqkv, 3 * C * N, edge, B, N, C, K, H, eps, L.stream_ptr())
        dkv = torch.zeros((B, 2 * C, N), dtype=torch.float32, device=qkv.device)
        L.run.pcr_group_bwd_f32(edge, idx, dkv, B, 2 * C, N, N, K, L.stream_ptr())
        dqkv[:, C:] = dkv
        return dqkv, None, None, None


class TNorm(Function):
    """[relu](LayerNorm (G = 1) / GroupNorm over the channels of every token of (B,C,L) [+ res])"""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, G, eps, relu):
        x = _dev(x)
        B, C, Ln = x.shape
        y = torch.empty_like(x)
        mean, rstd = _f32(B, G, Ln, device=x.device), _f32(B, G, Ln, device=x.device)
        L.run.pcr_tnorm_fwd_f32(x, gamma.detach(), beta.detach(), None if res is None else _dev(res), y, mean, rstd, B,
                                C, Ln, G, eps, int(relu), L.stream_ptr())
        ctx.save_for_backward(x, gamma, mean, rstd, y if relu else None)
        ctx.meta = (G, res is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, rstd, y = ctx.saved_tensors
        G, has_res = ctx.meta
        B, C, Ln = x.shape
        g = g.contiguous()
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (has_res and y is not None) else None
        nparts = (B * Ln + 63) // 64              # one partial row per 64-token wave
        part = _f32(nparts, 2, C, device=x.device)
        L.run.pcr_tnorm_bwd_f32(g, x, gamma.detach(), mean, rstd, y, dx, dres, part, B, C, Ln, G, L.stream_ptr())
        dgam, dbet = reduce_regions(part, nparts, 2 * C, [(0, 1, C, C), (C, 1, C, C)])
        return dx, dgam.view(C), dbet.view(C), (dres if dres is not None else g) if has_res else None, None, None, None


def tnorm(x, norm, res=None, relu=False):
    L.require_default_eps(norm)
    G = getattr(norm, "num_groups", 1)
    return TNorm.apply(x, norm.weight, norm.bias, res, G, norm.eps, relu)


# ------------------------------------------------------------------------------- fused per-token chains --
# PCR_TRAIN_FUSED=0 keeps the unfused graph (one launch per layer: the form of rounds 2-4, and the yardstick of
# tests/test_gpu_train_chain.py)
FUSED_CHAINS = os.environ.get("PCR_TRAIN_FUSED", "1") != "0"


def _chain_bf():
    """-> (backward matrix phases on the bf16 core, forward chain too)"""
    return TRAIN_PRECISION != "f32", TRAIN_PRECISION == "bf16x3_all"


def _chain_images(w, bf):
    """(image of W for the forward chain, image of W^T for the backward) in the formats the arithmetic `bf` = (bwd, fwd)
    reads: bf16 hi / lo images where that side runs on the bf16 matrix core, pcr_pack_weight images where it does not"""
    f32 = pack_both(w) if not (bf[0] and bf[1]) else None
    b16 = pack_both_bf(w) if (bf[0] or bf[1]) else None
    return (b16[0] if bf[1] else f32[0]), (b16[1] if (bf[0] or bf[1]) else f32[1])


def _chain_precision(p, bf):
    p.precision, p.fwd_precision = int(bf[0] or bf[1]), int(bf[1])


# The backward of a chain leaves one partial record per workgroup; the two functions below say where its fields lie, as
# [(offset in floats, rows, cols, ld)] in the order the Function returns the gradients.  They restate TailShape::O_* /
# HeadShape::O_* of csrc/train_chain_kernels.hip, whose last field closes the record: check_part_regions holds them to it.
def tail_regions(d, c1, hid, out):
    """dWm (d, d) | dW0 (hid, c1 + d), rows padded to ceil32 | dW2 (out, hid) | dg1, db1 (d) | dg2, db2 (out)"""
    cup = _c32(c1 + d)
    o0, o2 = d * d, d * d + hid * cup
    og = o2 + out * hid
    return [(0, d, d, d), (o0, hid, c1 + d, cup), (o2, out, hid, hid), (og, 1, d, d), (og + d, 1, d, d),
            (og + 2 * d, 1, out, out), (og + 2 * d + out, 1, out, out)]


def head_regions(C, hd, d, n):
    """dP1 (hd, 3), rows padded to 32 | dP2 (C, hd) | dW_j (d, C), j < n | dc1 (hd) | dc2 (C) in the record; returned as
    dP1, dc1, dP2, dc2, dW_0 .. dW_{n-1}"""
    o_p2 = hd * 32
    o_w = o_p2 + C * hd
    o_c1 = o_w + n * d * C
    return [(0, hd, 3, 32), (o_c1, 1, hd, hd), (o_p2, C, hd, hd), (o_c1 + hd, 1, C, C)] + \
           [(o_w + j * d * C, d, C, C) for j in range(n)]


def check_part_regions(regions, rec, what):
    """`regions` must end where the library's partial record of `rec` floats ends (rec = 0: no such instantiation).  A
    field added on one side only would otherwise put weight gradients at wrong offsets behind a plausible loss."""
    off, rows, _, ld = max(regions)
    if off + rows * ld != rec:
        raise L.PcrError("%s: the gradient regions end at float %d of a partial record, the library's record has %d"
                         % (what, off + rows * ld, rec))


# ---- what AttnTail / AttnHead share ----
def _chain_fwd(ctx, launch, p, tag, flops, nbytes, out_shape, tensors, images):
    """launch the forward of parameter block `p` into a new tensor; keep `tensors` and the image pairs for the backward"""
    out = _f32(*out_shape, device=tensors[0].device)
    p.outp = _p(out)
    with _prof(tag, flops, nbytes, arith="lib"):
        launch(ctypes.byref(p), L.stream_ptr())
    ctx.save_for_backward(*tensors, *[t for im in images for t in im])
    ctx.nkept = len(tensors)
    return out


def _chain_saved(ctx):
    """-> (the tensors _chain_fwd kept, the image pairs)"""
    saved = ctx.saved_tensors
    flat = saved[ctx.nkept:]
    return saved[:ctx.nkept], list(zip(flat[0::2], flat[1::2]))


def _chain_bwd(launch, groups, p, tag, flops, nbytes, g, rec, regions):
    """launch the backward of `p` (its input-gradient pointers set) for the output gradient g over groups(p) partial
    records of `rec` floats -> the `regions` of the record, each summed over the records"""
    check_part_regions(regions, rec, tag)
    nwg = groups(ctypes.byref(p))
    parts = _f32(nwg, rec, device=g.device)
    p.dout, p.parts, p.part_stride = _p(g), _p(parts), rec
    with _prof(tag, flops, nbytes, arith="lib"):
        launch(ctypes.byref(p), L.stream_ptr())
    return reduce_regions(parts, nwg, rec, regions)


def _tail_params(msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps, images, bf):
    B, d, Ln = msg.shape
    c1, hid, out = res.shape[1], W0.shape[0], W2.shape[0]
    p = _AttnTailP()
    p.B, p.L, p.d, p.c1, p.hid, p.out, p.residual, p.eps = B, Ln, d, c1, hid, out, int(residual), eps
    p.msg, p.res = _p(msg), _p(res)
    (p.wm, p.wmT), (p.w0, p.w0T), (p.w2, p.w2T) = [(_p(a), _p(b)) for a, b in images]
    p.g1, p.b1, p.g2, p.b2 = _p(g1.detach()), _p(b1.detach()), _p(g2.detach()), _p(b2.detach())
    _chain_precision(p, bf)
    return p, (B, d, Ln, c1, hid, out)


def _tail_work(B, d, Ln, c1, hid, out):
    """-> (profile tag with the direction left open, flops of the forward)"""
    return "attn_tail_%%s[d=%d,c1=%d,hid=%d,out=%d,L=%d]" % (d, c1, hid, out, Ln), \
        2.0 * B * Ln * (d * d + (c1 + d) * hid + hid * out)


class AttnTail(Function):
    """the tail of an attention block as ONE launch each way (pcr_attn_tail_{fwd,bwd}_f32):
    out = LN2(W2 relu(W0 [res ; LN1(Wm msg)])) [+ res]; nothing but msg and res is kept for the backward"""

    @staticmethod
    def forward(ctx, msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps):
        msg, res = _dev(msg), _dev(res)
        bf = _chain_bf()
        images = [_chain_images(Wm, bf), _chain_images(W0, bf), _chain_images(W2, bf)]
        p, (B, d, Ln, c1, hid, out) = _tail_params(msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps, images, bf)
        ctx.meta = (residual, eps, bf)
        tag, flops = _tail_work(B, d, Ln, c1, hid, out)
        return _chain_fwd(ctx, L.run.pcr_attn_tail_fwd_f32, p, tag % "fwd", flops, 4.0 * B * Ln * (d + c1 + out),
                          (B, out, Ln), (msg, res, Wm, g1, b1, W0, W2, g2, b2), images)

    @staticmethod
    def backward(ctx, g):
        (msg, res, Wm, g1, b1, W0, W2, g2, b2), images = _chain_saved(ctx)
        residual, eps, bf = ctx.meta
        p, (B, d, Ln, c1, hid, out) = _tail_params(msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps, images, bf)
        g = _dev(g)
        dmsg, dres = torch.empty_like(msg), torch.empty_like(res)
        p.dmsg, p.dres = _p(dmsg), _p(dres)
        tag, flops = _tail_work(B, d, Ln, c1, hid, out)
        lib = L.load()
        dWm, dW0, dW2, dg1, db1, dg2, db2 = _chain_bwd(
            L.run.pcr_attn_tail_bwd_f32, lib.pcr_attn_tail_groups, p, tag % "bwd", 3.0 * flops,
            4.0 * B * Ln * (2 * d + 2 * c1 + out), g, lib.pcr_attn_tail_part_floats(d, c1, hid, out),
            tail_regions(d, c1, hid, out))
        return dmsg, dres, dWm, dg1.view(d), db1.view(d), dW0, dW2, dg2.view(out), db2.view(out), None, None


def attn_tail(m, msg, res, residual):
    """fused tail of attention block `m` (merge / norm1 / mlp[0], mlp[2] / norm2), or None when the shape has no fused
    instantiation (the caller then runs the unfused graph)"""
    if not FUSED_CHAINS:
        return None
    merge, n1, mlp, n2 = m.merge, m.norm1, m.mlp, m.norm2
    d, c1 = msg.shape[1], res.shape[1]
    hid, out = mlp[0].weight.shape[0], mlp[2].weight.shape[0]
    if (merge.weight.shape != (d, d) or mlp[0].weight.shape[1] != c1 + d or mlp[2].weight.shape[1] != hid or
            getattr(n1, "num_groups", 1) != 1 or getattr(n2, "num_groups", 1) != 1 or
            n1.weight.numel() != d or n2.weight.numel() != out or n1.eps != n2.eps or
            not L.load().pcr_attn_tail_ok(d, c1, hid, out, int(bool(residual)))):
        return None
    L.require_default_eps(n1)
    return AttnTail.apply(msg, res, merge.weight, n1.weight, n1.bias, mlp[0].weight, mlp[2].weight, n2.weight, n2.bias,
                          bool(residual), float(n1.eps))


def _head_params(x, xyz, P1, c1, P2, c2, src, Ws, images, bf):
    B, C, Ln = x.shape
    hd, d, n = P1.shape[0], Ws[0].shape[0], len(Ws)
    p = _AttnHeadP()
    p.B, p.L, p.c, p.hd, p.d, p.np, p.src = B, Ln, C, hd, d, n, src
    p.x, p.xyz = _p(x), _p(xyz)
    p.p1, p.p2, p.p2T = _p(images[0][0]), _p(images[1][0]), _p(images[1][1])
    p.c1, p.c2 = _p(pad32(c1, hd)), _p(pad32(c2, C))
    for j in range(n):
        p.w[j], p.wT[j] = _p(images[2 + j][0]), _p(images[2 + j][1])
    _chain_precision(p, bf)
    return p, (B, C, Ln, hd, d, n)


def _head_work(B, C, Ln, hd, d, n):
    """-> (profile tag with the direction left open, flops of the forward)"""
    return "attn_head_%%s[c=%d,hd=%d,d=%d,n=%d,L=%d]" % (C, hd, d, n, Ln), 2.0 * B * Ln * (3 * hd + hd * C + n * d * C)


class AttnHead(Function):
    """the head of an attention block as ONE launch each way (pcr_attn_head_{fwd,bwd}_f32): fp = x + P2 relu(P1 xyz + c1)
    + c2, out (B, n d, L) = [W_j s_j] with s_j = fp (bit j of src) or x; nothing but x and xyz is kept for the backward"""

    @staticmethod
    def forward(ctx, x, xyz, P1, c1, P2, c2, src, *Ws):
        x, xyz = _dev(x), _dev(xyz)
        bf = _chain_bf()                                  # (P1: three input channels, an f32 image either way)
        images = [pack_both(P1), _chain_images(P2, bf)] + [_chain_images(W, bf) for W in Ws]
        p, (B, C, Ln, hd, d, n) = _head_params(x, xyz, P1, c1, P2, c2, src, Ws, images, bf)
        ctx.meta = (src, bf)
        tag, flops = _head_work(B, C, Ln, hd, d, n)
        return _chain_fwd(ctx, L.run.pcr_attn_head_fwd_f32, p, tag % "fwd", flops, 4.0 * B * Ln * (C + 3 + n * d),
                          (B, n * d, Ln), (x, xyz, P1, c1, P2, c2, *Ws), images)

    @staticmethod
    def backward(ctx, g):
        (x, xyz, P1, c1, P2, c2, *Ws), images = _chain_saved(ctx)
        src, bf = ctx.meta
        p, (B, C, Ln, hd, d, n) = _head_params(x, xyz, P1, c1, P2, c2, src, Ws, images, bf)
        g = _dev(g)
        dx = torch.empty_like(x)
        p.dx = _p(dx)
        tag, flops = _head_work(B, C, Ln, hd, d, n)
        lib = L.load()
        dP1, dc1, dP2, dc2, *dWs = _chain_bwd(
            L.run.pcr_attn_head_bwd_f32, lib.pcr_attn_head_groups, p, tag % "bwd", 3.0 * flops,
            4.0 * B * Ln * (2 * C + 3 + n * d), g, lib.pcr_attn_head_part_floats(C, hd, d, n, src),
            head_regions(C, hd, d, n))
        return (dx, None, dP1, dc1.view(hd), dP2, dc2.view(C), None, *dWs)


def attn_head(pos_mlp, x, xyz_cm, Ws, src):
    """fused head: position MLP `pos_mlp` = [Linear(3, hd), ReLU, Linear(hd, c)] added to x, then the projections Ws
    ((d, c) weights; bit j of src: projection j reads x + position code, else x) -> (B, len(Ws) d, L), or None when the
    shape has no fused instantiation"""
    if not FUSED_CHAINS:
        return None
    p1, p2 = pos_mlp[0], pos_mlp[2]
    C, d = x.shape[1], Ws[0].shape[0]
    if (p1.weight.shape[1] != 3 or p2.weight.shape != (C, p1.weight.shape[0]) or p1.bias is None or p2.bias is None or
            any(W.shape != (d, C) for W in Ws) or xyz_cm.shape[1] != 3 or xyz_cm.shape[2] != x.shape[2] or
            not L.load().pcr_attn_head_ok(C, p1.weight.shape[0], d, len(Ws), src)):
        return None
    return AttnHead.apply(x, xyz_cm, p1.weight, p1.bias, p2.weight, p2.bias, src, *Ws)


class LinAttnKV(Function):
    """LinAttn with k | v as the two channel halves of ONE (B,2d,Sk) tensor (the fused head's output): the gradient comes
    back as one buffer -- no slice / pad / add nodes in the autograd graph"""

    @staticmethod
    def forward(ctx, q, kv, H, eps):
        q, kv = _dev(q), _dev(kv)
        d = q.shape[1]
        out, A, ks = _linattn_fwd(q, kv[:, :d], kv[:, d:], H, eps)
        ctx.save_for_backward(q, kv, A, ks)
        ctx.meta = (H, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        q, kv, A, ks = ctx.saved_tensors
        H, eps = ctx.meta
        d = q.shape[1]
        dq, buf = torch.empty_like(q), torch.empty_like(kv)
        _linattn_bwd(q, kv[:, :d], kv[:, d:], A, ks, g.contiguous(), dq, buf[:, :d], buf[:, d:], H, eps)
        return dq, buf, None, None


class PoolPair(Function):
    """o (2P,C,L) -> (P,2C): [max, mean] over the point-concatenated pair (clouds p and p + P)"""

    @staticmethod
    def forward(ctx, o):
        o = _dev(o)
        twoP, C, Ln = o.shape
        P = twoP // 2
        pooled = _f32(P, 2 * C, device=o.device)
        arg = torch.empty((P, C), dtype=torch.int32, device=o.device)
        L.run.pcr_pool_pair_fwd_f32(o, pooled, arg, P, C, Ln, L.stream_ptr())
        ctx.save_for_backward(arg)
        ctx.dims = (P, C, Ln)
        return pooled

    @staticmethod
    def backward(ctx, g):
        arg, = ctx.saved_tensors
        P, C, Ln = ctx.dims
        g = g.contiguous()
        dout = _f32(2 * P, C, Ln, device=g.device)
        L.run.pcr_pool_pair_bwd_f32(g, arg, dout, P, C, Ln, L.stream_ptr())
        return dout


class PoolBoth(Function):
    """o (P,C,L) -> (P,2C): [max over L, mean over L] (get_pooled_feats 'both' on one tensor, ReIDNet.py:529-532)"""

    @staticmethod
    def forward(ctx, o):
        o = _dev(o)
        P, C, Ln = o.shape
        pooled = _f32(P, 2 * C, device=o.device)
        arg = torch.empty((P, C), dtype=torch.int32, device=o.device)
        if P:                                                # (no clouds: empty tensors, nothing to launch)
            L.run.pcr_pool_both_fwd_f32(o, pooled, arg, P, C, Ln, L.stream_ptr())
        ctx.save_for_backward(arg)
        ctx.dims = (P, C, Ln)
        return pooled

    @staticmethod
    def backward(ctx, g):
        arg, = ctx.saved_tensors
        P, C, Ln = ctx.dims
        g = g.contiguous()
        dout = _f32(P, C, Ln, device=g.device)
        if P:
            L.run.pcr_pool_both_bwd_f32(g, arg, dout, P, C, Ln, L.stream_ptr())
        return dout


class ChannelMax(Function):
    """x (B,C,L) -> (B,C/W,L): max over windows of W channels of every point (get_pooled_feats 'max', ReIDNet.py:145,
    526-528: nn.MaxPool1d(W) on the permuted tensor)"""

    @staticmethod
    def forward(ctx, x, W):
        x = _dev(x)
        B, C, Ln = x.shape
        y = _f32(B, C // W, Ln, device=x.device)
        arg = torch.empty((B, C // W, Ln), dtype=torch.int32, device=x.device)
        if B:                                              # (no clouds: empty tensors, nothing to launch)
            L.run.pcr_channel_max_fwd_f32(x, y, arg, B, C, Ln, W, L.stream_ptr())
        ctx.save_for_backward(arg)
        ctx.dims = (B, C, Ln, W)
        return y

    @staticmethod
    def backward(ctx, g):
        arg, = ctx.saved_tensors
        B, C, Ln, W = ctx.dims
        g = g.contiguous()
        dx = _f32(B, C, Ln, device=g.device)
        if B:
            L.run.pcr_channel_max_bwd_f32(g, arg, dx, B, C, Ln, W, L.stream_ptr())
        return dx, None


# ------------------------------------------------------------ pair lists (csrc/train_pair_kernels.hip) --
def _list_count(count, who):
    """count of a pair list: None (every slot) or a (1,) int32 device tensor"""
    if count is None:
        return None
    L.require_cuda(count)
    if count.dtype != torch.int32 or count.numel() != 1:
        raise L.PcrError("%s: count must be a (1,) int32 device tensor" % who)
    return count.reshape(1).contiguous()


def index_sum(src, idx, count, M):
    """src (P, ...) f32, idx (P) int32, count (1,) int32 or None -> dst (M, ...): dst[m] = the sum of the rows src[p] with
    idx[p] == m over p < min(count, P), added in increasing p from +0 (pcr_index_sum_f32: one owner per accumulator, no
    float atomics).  A row no live slot names is 0; an index outside [0, M) names no row."""
    src, idx = _dev(src), idx.contiguous()
    L.require_cuda(idx)
    L.require_i32(idx)
    P = src.shape[0]
    if idx.numel() != P:
        raise L.PcrError("index_sum: %d indices for %d rows" % (idx.numel(), P))
    R = 1
    for s in src.shape[1:]:
        R *= s
    dst = _f32(M, *src.shape[1:], device=src.device)
    if M and dst.numel():
        with _prof("index_sum[P=%d,M=%d,R=%d]" % (P, M, R), float(P) * R, 4.0 * (P + M) * R):
            L.run.pcr_index_sum_f32(src, idx, _list_count(count, "index_sum"), dst, P, M, R, L.stream_ptr())
    return dst


class PairGather(Function):
    """out[p] = x[idx[p]] over the first axis: x (M, ...) f32, idx (P) int32 on the device, count (1,) int32 or None ->
    (P, ...).  A slot whose index lies outside [0, M) is dead: it reads row 0 (its values are never used) and sends no
    gradient anywhere; neither does a slot from count on.  Backward: index_sum -- the gradient of object m is the sum of
    its slots' gradients in list order, bit-reproducible.  idx and count get no gradient."""

    @staticmethod
    def forward(ctx, x, idx, count=None):
        x = _dev(x)
        L.require_cuda(idx)
        L.require_i32(idx)
        idx = idx.contiguous()
        M = x.shape[0]
        safe = torch.where((idx >= 0) & (idx < M), idx, torch.zeros_like(idx))
        ctx.save_for_backward(idx, *(() if count is None else (_list_count(count, "PairGather"),)))
        ctx.M = M
        return x.index_select(0, safe.long())

    @staticmethod
    def backward(ctx, g):
        idx, *count = ctx.saved_tensors
        return index_sum(g, idx, count[0] if count else None, ctx.M), None, None


IndexSum = PairGather     # (named by its backward)


def pair_gather(x, idx, count=None):
    return PairGather.apply(x, idx, count)


def linattn_pairs_ok(d, H):
    """does the indexed attention core cover (d_model, heads)?  (pcr_linattn_pairs_ok: head widths 32 and 64)"""
    return bool(L.load().pcr_linattn_pairs_ok(int(d), int(H)))


class LinAttnPairs(Function):
    """The linear-attention core over a pair list (include/pcr.h section C3): qkv (M,3d,L) = the fused q | k | v projection
    per OBJECT, qi, si (R) int32 on the device -> (R,d,L): slot r = the queries of object qi[r] against the key / value
    state of object si[r].  The state A | ks is made once per object (state_fwd) however many slots read it.  Backward:
    apply_bwd leaves the slots' query gradients and [dA | dks] records, two index_sums carry them to the objects (list
    order, no float atomics), state_bwd turns the summed records into dk, dv; the gradient comes back as one (M,3d,L)
    buffer.  A slot with an index outside [0, M) is dead: zeros out, nothing back.  qi, si get no gradient."""

    @staticmethod
    def forward(ctx, qkv, qi, si, H, eps):
        qkv, qi, si = _dev(qkv), qi.contiguous(), si.contiguous()
        L.require_cuda(qi, si)
        L.require_i32(qi, si)
        M, d3, Ln = qkv.shape
        d, R = d3 // 3, qi.numel()
        if si.numel() != R or not linattn_pairs_ok(d, H):
            raise L.PcrError("LinAttnPairs: d = %d, H = %d, %d / %d indices (pcr_linattn_pairs_ok)" % (d, H, R, si.numel()))
        dev, dh = qkv.device, d // H
        A, ks = _f32(M, H, dh, dh, device=dev), _f32(M, H, dh, device=dev)
        out = _f32(R, d, Ln, device=dev)
        eps_t = torch.full((1,), float(eps), dtype=torch.float32, device=dev)
        bs = d3 * Ln
        with _prof("linattn_state_fwd[d=%d,L=%d]" % (d, Ln), 2.0 * M * Ln * d * dh, 4.0 * M * (2 * d * Ln + d * dh)):
            L.run.pcr_linattn_state_fwd_f32(qkv[:, d:2 * d], qkv[:, 2 * d:], bs, A, ks, M, Ln, d, H, L.stream_ptr())
        with _prof("linattn_apply_fwd[d=%d,L=%d]" % (d, Ln), 2.0 * R * Ln * d * dh, 4.0 * R * (2 * d * Ln + d * dh)):
            L.run.pcr_linattn_apply_fwd_f32(qkv, bs, A, ks, qi, si, eps_t, out, M, R, Ln, d, H, L.stream_ptr())
        # a slot is dead when EITHER index is: apply_bwd leaves its dqs / rec rows unwritten, so neither index_sum of the
        # backward may name an object for it (on the device: no host read, the launches stay capturable)
        live = (qi >= 0) & (qi < M) & (si >= 0) & (si < M)
        ctx.save_for_backward(qkv, A, ks, qi, si, eps_t, live)
        ctx.H = H
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, A, ks, qi, si, eps_t, live = ctx.saved_tensors
        H = ctx.H
        M, d3, Ln = qkv.shape
        d, R = d3 // 3, qi.numel()
        dev, dh = qkv.device, d // H
        dqs, rec = _f32(R, d, Ln, device=dev), _f32(R, H, dh * (dh + 1), device=dev)
        bs = d3 * Ln
        with _prof("linattn_apply_bwd[d=%d,L=%d]" % (d, Ln), 6.0 * R * Ln * d * dh, 4.0 * R * (3 * d * Ln + 2 * d * dh)):
            L.run.pcr_linattn_apply_bwd_f32(qkv, bs, A, ks, qi, si, eps_t, g.contiguous(), dqs, rec, M, R, Ln, d, H,
                                            L.stream_ptr())
        buf = torch.empty_like(qkv)
        sum_q, sum_s = torch.where(live, torch.stack([qi, si]), -1)     # dead in one list: dead in both
        buf[:, :d] = index_sum(dqs, sum_q, None, M)
        drec = index_sum(rec, sum_s, None, M)
        with _prof("linattn_state_bwd[d=%d,L=%d]" % (d, Ln), 4.0 * M * Ln * d * dh, 4.0 * M * (4 * d * Ln + d * dh)):
            L.run.pcr_linattn_state_bwd_f32(qkv[:, d:2 * d], qkv[:, 2 * d:], bs, drec, buf[:, d:2 * d], buf[:, 2 * d:], bs,
                                            M, Ln, d, H, L.stream_ptr())
        return buf, None, None, None, None


# --------------------------------------------------------------- PointNet pieces (csrc/train_bn_kernels.hip) --
class BnAct(Function):
    """act(BatchNorm(y)) with BATCH statistics over (B, L) per channel on a (B,C,L) tensor; act: None, "relu" or
    ("leaky", slope).  Running statistics are updated in place as nn.BatchNorm1d does in training mode.  (The
    Point-Transformer path folds its BatchNorms into the train-dense launches; PointNet's and DGCNN's stand between
    layers that cannot take them.)"""

    @staticmethod
    def forward(ctx, y, gamma, beta, bn, act, slope):
        y = _dev(y)
        B, C, Ln = y.shape
        _bn_refuse(bn)
        _require_batch(B * Ln, y.shape)
        nparts = _bn_nparts(B, C)
        part = _f32(nparts, 2, _c32(C), device=y.device)
        # sums of y - y[0][c][0] (first element of the channel as the offset): see pcr_bn_fwd_fin.shift0
        L.run.pcr_bn_sums_f32(y, None, None, None, 0, 0.0, None, 1, part, nparts, B, C, Ln, L.stream_ptr())
        n = _bn_batch_step(part, nparts, C, B * Ln, gamma, beta, bn, shift0=y, shift0_stride=Ln)
        z = _f32(B, C, Ln, device=y.device)
        L.run.pcr_bn_affine_f32(y, None, n["scale"], n["shift"], None, None, None, None, int(act), slope, z, B, C, Ln,
                                L.stream_ptr())
        ctx.save_for_backward(y, gamma)
        ctx.norm, ctx.act, ctx.slope, ctx.nparts = n, int(act), float(slope), nparts
        return z

    @staticmethod
    def backward(ctx, g):
        y, gamma = ctx.saved_tensors
        n, act, slope, nparts = ctx.norm, ctx.act, ctx.slope, ctx.nparts
        B, C, Ln = y.shape
        g = g.contiguous()
        part = _f32(nparts, 2, _c32(C), device=y.device)
        L.run.pcr_bn_sums_f32(y, g, n["scale"], n["shift"], act, slope, n["mean"], 0, part, nparts, B, C, Ln,
                              L.stream_ptr())
        k = bn_bwd_finalize(part, nparts, C, B * Ln, gamma, n["mean"], n["invstd"], centre=n["mean"])
        dy = _f32(B, C, Ln, device=y.device)
        kc = k["ka"] * k["dbeta"] * (-1.0 / (B * Ln))        # centred form: dy = ka g' + kb (y - mean) - ka dbeta / R
        L.run.pcr_bn_affine_f32(y, g, k["ka"], k["kb"], kc, n["scale"], n["shift"], n["mean"], act, slope, dy, B, C,
                                Ln, L.stream_ptr())
        return dy, k["dgamma"], k["dbeta"], None, None, None


def bn_act(y, bn, relu, slope=0.0):
    """relu: apply the activation z > 0 ? z : slope z after the norm (slope 0: ReLU)"""
    return BnAct.apply(y, bn.weight, bn.bias, bn, bool(relu), slope)


class EdgeConvTrain(Function):
    """One EdgeConv layer of DGCNN in training mode (dgcnn_orig.py:32-56, 127-143): Conv2d(2C -> Co, no bias) on
    [f_j - f_i ; f_i] + BatchNorm2d over all B N k edges (batch statistics) + LeakyReLU + max over the k neighbours.
    The conv is decomposed as in the inference path, W [f_j - f_i ; f_i] = W1 f_j + (W2 - W1) f_i: `tab` (B,2Co,N) =
    [W1 f ; (W2 - W1) f] comes from ONE train-dense launch (autograd carries the table gradient back into the weight),
    and the per-edge pre-activation y = tab[:Co][idx] + tab[Co:][i] is the first layer of the grouped set-abstraction
    MLP with no coordinate term -- pcr_sa_l1_{fwd,bwd}_f32 with the points as their own centres."""

    @staticmethod
    def forward(ctx, tab, idx, gamma, beta, bn, slope):
        tab, idx = _dev(tab), idx.contiguous()
        L.require_i32(idx)
        B, two_co, N = tab.shape
        Co = two_co // 2
        K = idx.shape[2]
        dev = tab.device
        _bn_refuse(bn)
        _require_batch(B * N * K, (B, Co, N, K))
        xyz0 = torch.zeros((B, N, 3), dtype=torch.float32, device=dev)       # (no coordinate term: zero weights below)
        wa0 = torch.zeros((Co, 3), dtype=torch.float32, device=dev)
        b0 = torch.zeros((Co,), dtype=torch.float32, device=dev)
        y = _f32(B, Co, N * K, device=dev)
        st = _f32(B, 2, _c32(Co), device=dev)
        L.run.pcr_sa_l1_fwd_f32(xyz0, idx, tab, wa0, b0, y, st, B, N, N, K, Co, L.stream_ptr())
        n = _bn_batch_step(st, B, Co, B * N * K, gamma, beta, bn)
        pooled = _f32(B, Co, N, device=dev)
        arg = torch.empty((B, Co, N), dtype=torch.int32, device=dev)
        yraw = _f32(B, Co, N, device=dev)
        L.run.pcr_edge_pool_fwd_f32(y, n["scale"], n["shift"], slope, pooled, arg, yraw, B, Co, N, K, L.stream_ptr())
        ctx.save_for_backward(idx, y, pooled, arg, yraw, gamma, xyz0)
        ctx.norm, ctx.slope, ctx.dims = n, float(slope), (B, Co, N, K)
        return pooled

    @staticmethod
    def backward(ctx, gp):
        idx, y, pooled, arg, yraw, gamma, xyz0 = ctx.saved_tensors
        n, slope = ctx.norm, ctx.slope
        B, Co, N, K = ctx.dims
        dev = y.device
        gp = gp.contiguous()
        R = B * N * K
        # the two sums of the BatchNorm backward: the routed gradient is non-zero on ONE edge per (channel, point)
        nparts = _bn_nparts(B, Co)
        part = _f32(nparts, 2, _c32(Co), device=dev)
        L.run.pcr_bn_sums_f32(yraw, gp, n["scale"], n["shift"], 1, slope, n["mean"], 0, part, nparts, B, Co, N,
                              L.stream_ptr())
        k = bn_bwd_finalize(part, nparts, Co, R, gamma, n["mean"], n["invstd"], centre=n["mean"])
        g = _f32(B, Co, N * K, device=dev)
        L.run.pcr_edge_pool_route_f32(gp, pooled, arg, slope, g, B, Co, N, K, L.stream_ptr())
        dtab = _f32(B, 2 * Co, N, device=dev)
        dwa_p = _f32(B, Co, 4, device=dev)
        L.run.pcr_sa_l1_bwd_f32(xyz0, idx, g, y, k["ka"], k["kb"], k["kc"], dtab, dwa_p, B, N, N, K, Co,
                                L.stream_ptr())
        return dtab, None, k["dgamma"], k["dbeta"], None, None


class Bmm(Function):
    """x (B,k,N), T (B,k,k) -> y[b] = T[b]^T x[b]  (torch.bmm(x^T, T)^T: the PointNet input / feature transforms)"""

    @staticmethod
    def forward(ctx, x, T):
        x, T = _dev(x), _dev(T)
        B, k, N = x.shape
        y = _f32(B, k, N, device=x.device)
        L.run.pcr_bmm_apply_f32(x, T, y, B, k, N, 0, L.stream_ptr())
        ctx.save_for_backward(x, T)
        return y

    @staticmethod
    def backward(ctx, g):
        x, T = ctx.saved_tensors
        B, k, N = x.shape
        g = g.contiguous()
        dx = dT = None
        if ctx.needs_input_grad[0]:
            dx = _f32(B, k, N, device=x.device)
            L.run.pcr_bmm_apply_f32(g, T, dx, B, k, N, 1, L.stream_ptr())
        if ctx.needs_input_grad[1]:
            dT = _f32(B, k, k, device=x.device)
            L.run.pcr_bmm_dt_f32(x, g, dT, B, k, N, L.stream_ptr())
        return dx, dT


# ------------------------------------------------------------------------------- auxiliary losses (pcr.h C2) --
AUX_INFO_KL_EMPTY, AUX_INFO_TRIPLET_NONE, AUX_INFO_TRIPLET_POOL = 1, 2, 4
_AUX = "pcr_amd.train_ops"


def _i32_dev(t, name, n):
    return L.tensor(t, _AUX, name, torch.int32, numel=n)


class KlPairs(Function):
    """h (2B, ...) = [h1 ; h2], match (B) int32, info (1) int32 -> (the unscaled kl term of get_kl_loss, ReIDNet.py:467-482,
    a 0-d tensor; kl (B) per pair, no gradient).  Forward and closed-form backward are pcr_kl_pairs_fwd / _bwd_f32."""

    @staticmethod
    def forward(ctx, h, match, info):
        h = _dev(h)
        L.require(h.dim() >= 2 and h.shape[0] >= 2 and h.shape[0] % 2 == 0, _AUX, "KlPairs: h must be (2B, ...), got %s",
                  tuple(h.shape))
        B = h.shape[0] // 2
        D = h[0].numel()
        match, info = _i32_dev(match, "match", B), _i32_dev(info, "info", 1)
        L.require_cuda(match, info)
        dev = h.device
        lse, cross, kl, loss = _f32(2 * B, device=dev), _f32(B, device=dev), _f32(B, device=dev), _f32(1, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        L.run.pcr_kl_pairs_fwd_f32(h, match, lse, cross, kl, loss, counts, info, B, D, L.stream_ptr())
        ctx.save_for_backward(h, match, lse, cross, counts)
        ctx.mark_non_differentiable(kl)
        return loss.reshape(()), kl

    @staticmethod
    def backward(ctx, g, _gkl):
        h, match, lse, cross, counts = ctx.saved_tensors
        B = h.shape[0] // 2
        dh = torch.empty_like(h)
        L.run.pcr_kl_pairs_bwd_f32(h, match, lse, cross, counts, g.reshape(1).float().contiguous(), dh, B, h[0].numel(),
                                   L.stream_ptr())
        return dh, None, None


def triplet_draw(ids, match, T, info, seed=None, rand=None):
    """ids (2B) int32, match (B) int32 -> neg (B, T) int32 (pcr_triplet_draw_i32).  seed: a device int64 tensor of one
    element (None: 0); rand (B T) int32: the words, in the place of W(seed, 3, pair, t)"""
    B, T = match.numel(), int(T)
    ids, match, info = _i32_dev(ids, "ids", 2 * B), _i32_dev(match, "match", B), _i32_dev(info, "info", 1)
    rand = L.tensor(rand, _AUX, "rand", torch.int32, numel=B * T, optional=True)
    if seed is not None:
        L.require(isinstance(seed, torch.Tensor) and seed.dtype == torch.int64 and seed.numel() == 1, _AUX,
                  "seed must be a device int64 tensor of one element")
    L.require(B >= 1 and bool(L.load().pcr_triplet_ok(B, T)), _AUX,
              "triplet: %d pairs with %d negatives each are beyond pcr_triplet_ok", B, T)
    L.require_cuda(ids, match, info, rand, seed)
    neg = torch.empty((B, T), dtype=torch.int32, device=ids.device)
    L.run.pcr_triplet_draw_i32(ids, match, rand, L.ptr(seed), neg, info, B, T, L.stream_ptr())
    return neg


def pair_dist(a, h):
    """a (B, D), h (R, D) -> dist (B, R) = || (a_i - h_r) + 1e-6 ||_2 (pcr_pair_dist_f32; no gradient: TripletLoss owns it)"""
    a, h = _dev(a), _dev(h)
    L.require(a.dim() == 2 and h.dim() == 2 and a.shape[1] == h.shape[1] and a.shape[0] and h.shape[0] and a.shape[1],
              _AUX, "pair_dist: a (B, D) and h (R, D) of one width, got %s and %s", tuple(a.shape), tuple(h.shape))
    dist = _f32(a.shape[0], h.shape[0], device=a.device)
    L.run.pcr_pair_dist_f32(a, h, dist, a.shape[0], h.shape[0], a.shape[1], L.stream_ptr())
    return dist


class TripletLoss(Function):
    """h (2B, ...) = [anchors ; positives], neg (B, T) int32, match (B) int32, hyper (2) f32 = (margin, alpha), info (1)
    -> (alpha * TripletMarginLoss(margin, p = 2) over the triplets (pair i, row B + i, row neg[i][t]) of the matching
    pairs, a 0-d tensor; dist (B, 2B) and count (1) int32, no gradient).  The anchors are rows of h: one gradient."""

    @staticmethod
    def forward(ctx, h, neg, match, hyper, info):
        h = _dev(h)
        L.require(h.dim() >= 2 and h.shape[0] >= 2 and h.shape[0] % 2 == 0, _AUX, "TripletLoss: h must be (2B, ...), got %s",
                  tuple(h.shape))
        B = h.shape[0] // 2
        hf = h.reshape(2 * B, -1)
        D = hf.shape[1]
        L.require(isinstance(neg, torch.Tensor) and neg.dim() == 2 and neg.shape[0] == B and neg.shape[1] >= 1, _AUX,
                  "TripletLoss: neg must be (%d, T)", B)
        T = neg.shape[1]
        neg, match, info = _i32_dev(neg, "neg", B * T), _i32_dev(match, "match", B), _i32_dev(info, "info", 1)
        hyper = L.tensor(hyper, _AUX, "hyper", torch.float32, numel=2)
        L.require(bool(L.load().pcr_triplet_ok(B, T)), _AUX,
                  "triplet: %d pairs with %d negatives each are beyond pcr_triplet_ok", B, T)
        L.require_cuda(neg, match, info, hyper)
        dev = h.device
        dist = _f32(B, 2 * B, device=dev)
        L.run.pcr_pair_dist_f32(hf, hf, dist, B, 2 * B, D, L.stream_ptr())
        E, pair_loss, loss = _f32(B, 2 * B, device=dev), _f32(B, device=dev), _f32(1, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        L.run.pcr_triplet_select_f32(dist, neg, match, hyper, E, pair_loss, loss, count, info, B, T, L.stream_ptr())
        ctx.save_for_backward(hf, E, hyper, count)
        ctx.shape = h.shape
        ctx.mark_non_differentiable(dist, count)
        return loss.reshape(()), dist, count

    @staticmethod
    def backward(ctx, g, _gd, _gc):
        hf, E, hyper, count = ctx.saved_tensors
        R, D = hf.shape
        B = R // 2
        da, dh = _f32(B, D, device=hf.device), _f32(R, D, device=hf.device)
        L.run.pcr_pair_dist_bwd_f32(hf, hf, E, g.reshape(1).float().contiguous(), hyper, count, da, dh, B, R, D,
                                    L.stream_ptr())
        dh[:B] += da
        return dh.view(ctx.shape), None, None, None, None
