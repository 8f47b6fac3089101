"""float64 restatement of the two fused per-token chains of the attention blocks in training mode
(pcr_attn_tail_{fwd,bwd}_f32, pcr_attn_head_{fwd,bwd}_f32; csrc/train_chain_kernels.hip), the conditioning of their test
inputs, and the builder of every case of tests/test_gpu_train_chain_forms.py.  Plain torch on the CPU, written from the
statements of include/pcr.h; nothing here imports pcr_amd.  Every function computes in the dtype of its inputs: float64
is the reference, the same call on float32 tensors is the "float32 evaluation of the same formula" (the yardstick y32).

    tail   out = LN2(W2 relu(W0 [res ; LN1(Wm msg)])) [+ res]          msg (B,d,L), res (B,c1,L)
    head   fp = x + P2 relu(P1 xyz + c1) + c2;  out = [W_j s_j],  s_j = fp (bit j of src) | x

Every backward is written out term by term (`tail_bwd_ref`, `head_bwd_ref`); test_train_chain_ref_cpu.py holds each to
float64 autograd of the blocks' own nn.Linear / nn.LayerNorm / ReLU formulation.

Arithmetics.  `arith` selects an OPERAND MODEL of the split-bf16 products, a yardstick and never the reference: both
operands of a product are split hi = bf16(v), lo = bf16(v - hi) (dense_ref.bf_split), the lo x lo term is dropped, the
sums stay in the dtype of the call.  "bf16x3" runs the gradient products (dx = W^T g, dW = g s^T) that way, "bf16x3_all"
the forward products too; P1 xyz (three input channels) is an f32 product in every arithmetic.  ysplit = that model in
float64 against the plain float64 reference.

Decisions.  Each chain takes ONE kind: the sign of a hidden pre-activation, h = W0 [res ; n1] in the tail, P1 xyz + c1 in
the head.  An element is MARGINAL when |h| < REL_DELTA max|h| (train_ref's margin, ~100 x the float32 error of h).
`condition_tail` moves ONE element of res per offending token -- channel argmax_c |W0[j, c]| of the offending row j, so
that h_j lands at +- 2 delta on its own side -- and `condition_head` one coordinate of xyz; the moved value is rounded
to float32 before the next check, because the device gets float32.  Moving one row of a token may push another of its
rows into the margin, hence the loop; a token that has not settled after MAX_PASSES is redrawn from the case's generator.
No token is left out of any comparison.

`fault=` plants the four negative controls of the CPU file into the written-out backward (scratch variants: nothing
else calls them)."""
import functools
import zlib

import torch

from dense_ref import bf_split
from train_ref import MAX_PASSES, REL_DELTA

F64 = torch.float64
NORM_EPS = 1e-5                       # nn.LayerNorm's default, the only eps the Function accepts
TILE = 64                             # kCT: tokens per tile
ARITHS = ("f32", "bf16x3", "bf16x3_all")
_SPLIT = {"f32": (False, False), "bf16x3": (False, True), "bf16x3_all": (True, True)}      # (forward, backward)
MOVED_CAP = 0.08                      # share of a case's tokens the conditioning may touch


# ------------------------------------------------------------------------------------------- products --
def _split(v):
    hi, lo = bf_split(v)
    return hi.to(v.dtype), lo.to(v.dtype)


def _mm(W, x, split):
    """W (o,i), x (B,i,L) -> (B,o,L)"""
    e = lambda a, b: torch.einsum("oi,bil->bol", a, b)          # noqa: E731
    if not split:
        return e(W, x)
    (Wh, Wl), (xh, xl) = _split(W), _split(x)
    return e(Wh, xh) + e(Wh, xl) + e(Wl, xh)


def _mmT(g, s, split):
    """g (B,o,L), s (B,i,L) -> (o,i) = sum over clouds and tokens of g s^T"""
    e = lambda a, b: torch.einsum("bol,bil->oi", a, b)          # noqa: E731
    if not split:
        return e(g, s)
    (gh, gl), (sh, sl) = _split(g), _split(s)
    return e(gh, sh) + e(gh, sl) + e(gl, sh)


def _ln(v, eps):
    """-> (x hat, rstd (B,1,L)): every token normalised over its channels, BIASED variance, eps inside the root"""
    c = v - v.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt((c * c).mean(dim=1, keepdim=True) + eps)
    return c * rstd, rstd


def _ln_bwd(dy, xh, rstd, g):
    """a = gamma dy;  dx = rstd (a - mean(a) - x hat mean(a x hat))"""
    a = dy * g.view(1, -1, 1)
    return rstd * (a - a.mean(dim=1, keepdim=True) - xh * (a * xh).mean(dim=1, keepdim=True))


def _ch(v):
    return v.view(1, -1, 1)


def _drop_last(g):
    """(planted fault) the last token of a partial tile left out of a sum over tokens"""
    if g.shape[2] % TILE == 0:
        return g
    g = g.clone()
    g[:, :, -1] = 0
    return g


# ----------------------------------------------------------------------------------------------- tail --
def tail_ref(msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps, arith="f32"):
    """-> (out (B,out,L), dict of the intermediates the backward needs: xh1, rstd1, U = [res ; n1], h = W0 U, f0 = relu(h),
    xh2, rstd2)"""
    fs = _SPLIT[arith][0]
    xh1, rstd1 = _ln(_mm(Wm, msg, fs), eps)
    U = torch.cat([res, xh1 * _ch(g1) + _ch(b1)], dim=1)
    h = _mm(W0, U, fs)
    f0 = torch.relu(h)
    xh2, rstd2 = _ln(_mm(W2, f0, fs), eps)
    out = xh2 * _ch(g2) + _ch(b2)
    if residual:
        out = out + res
    return out, dict(xh1=xh1, rstd1=rstd1, U=U, h=h, f0=f0, xh2=xh2, rstd2=rstd2)


def tail_bwd_ref(msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps, dout, arith="f32", fault=None):
    """-> dict(dmsg, dres, dWm, dg1, db1, dW0, dW2, dg2, db2), term by term, no autograd"""
    bs = _SPLIT[arith][1]
    c1 = res.shape[1]
    t = tail_ref(msg, res, Wm, g1, b1, W0, W2, g2, b2, residual, eps, arith)[1]
    tok = _drop_last if fault == "drop_last" else (lambda g: g)
    db2, dg2 = dout.sum(dim=(0, 2)), (dout * t["xh2"]).sum(dim=(0, 2))
    dE = _ln_bwd(dout, t["xh2"], t["rstd2"], g2)                       # through LN2 (the residual passes dout by)
    dW2 = _mmT(tok(dE), t["f0"], bs)
    dh = torch.where(t["h"] > 0, _mm(W2.t(), dE, bs), torch.zeros_like(dE[:, :1]))       # the ReLU mask on h > 0
    dW0 = _mmT(tok(dh), t["U"], bs)
    dU = _mm(W0.t(), dh, bs)
    dres = dU[:, :c1] + (dout if residual and fault != "no_resid" else 0.0)
    dn1 = dU[:, c1:]
    db1, dg1 = dn1.sum(dim=(0, 2)), (dn1 * t["xh1"]).sum(dim=(0, 2))
    dM = _ln_bwd(dn1, t["xh1"], t["rstd1"], g1)
    dWm = _mmT(tok(dM), msg, bs)
    dmsg = _mm(Wm.t(), dM, bs)
    Ln = msg.shape[2]
    if fault == "pad_beta" and Ln % TILE:
        # (planted fault) d beta1 summed over all 64 tokens of the partial tile: the padding tokens carry msg = res = 0, so
        # n1 = b1 there, and a d out that was not zero-filled -- here the cloud's own first tokens again
        pad = TILE - Ln % TILE
        z = lambda v: torch.zeros(v.shape[0], v.shape[1], pad, dtype=v.dtype)        # noqa: E731
        stale = dout[:, :, torch.arange(pad) % Ln]
        db1 = db1 + tail_bwd_ref(z(msg), z(res), Wm, g1, b1, W0, W2, g2, b2, residual, eps, stale, arith)["db1"]
    return dict(dmsg=dmsg, dres=dres.clone(), dWm=dWm, dg1=dg1, db1=db1, dW0=dW0, dW2=dW2, dg2=dg2, db2=db2)


# ----------------------------------------------------------------------------------------------- head --
def head_ref(x, xyz, P1, c1, P2, c2, Ws, src, arith="f32"):
    """-> (out (B, n d, L), dict(pre = P1 xyz + c1, h = relu(pre), fp)); bit j of src: projection j reads fp, else x"""
    fs = _SPLIT[arith][0]
    pre = _mm(P1, xyz, False) + _ch(c1)                       # three input channels: f32 in every arithmetic
    h = torch.relu(pre)
    fp = x + _mm(P2, h, fs) + _ch(c2)
    out = torch.cat([_mm(W, fp if (src >> j) & 1 else x, fs) for j, W in enumerate(Ws)], dim=1)
    return out, dict(pre=pre, h=h, fp=fp)


def head_bwd_ref(x, xyz, P1, c1, P2, c2, Ws, src, dout, arith="f32", fault=None):
    """-> dict(dx, dP1, dc1, dP2, dc2, dW_0 ..): d fp sums the fp-sourced projections, dx = d fp + the x-sourced ones"""
    bs = _SPLIT[arith][1]
    if fault == "src_x":                                       # (planted fault) the lowest fp-sourced projection reads x
        src = src & (src - 1)
    t = head_ref(x, xyz, P1, c1, P2, c2, Ws, src, arith)[1]
    tok = _drop_last if fault == "drop_last" else (lambda g: g)
    d = Ws[0].shape[0]
    G = [dout[:, j * d:(j + 1) * d] for j in range(len(Ws))]
    out = {"dW_%d" % j: _mmT(tok(G[j]), t["fp"] if (src >> j) & 1 else x, bs) for j in range(len(Ws))}
    dfp = torch.zeros_like(x)
    dxs = torch.zeros_like(x)
    for j, W in enumerate(Ws):
        if (src >> j) & 1:
            dfp = dfp + _mm(W.t(), G[j], bs)
        else:
            dxs = dxs + _mm(W.t(), G[j], bs)
    dh = torch.where(t["pre"] > 0, _mm(P2.t(), dfp, bs), torch.zeros_like(dfp[:, :1]))
    out.update(dx=dfp + dxs, dc2=dfp.sum(dim=(0, 2)), dP2=_mmT(tok(dfp), t["h"], bs), dc1=dh.sum(dim=(0, 2)),
               dP1=_mmT(tok(dh), xyz, bs))
    return out


# --------------------------------------------------------------------------------------- conditioning --
def tail_hidden(msg, res, p, eps=NORM_EPS):
    """float64 h = W0 [res ; LN1(Wm msg)] (B,hid,L) of float32 inputs"""
    q = {k: v.to(F64) for k, v in p.items()}
    return tail_ref(msg.to(F64), res.to(F64), q["Wm"], q["g1"], q["b1"], q["W0"], q["W2"], q["g2"], q["b2"], False, eps)[1]["h"]


def head_hidden(xyz, p):
    """float64 P1 xyz + c1 (B,hd,L) of float32 inputs"""
    return _mm(p["P1"].to(F64), xyz.to(F64), False) + _ch(p["c1"].to(F64))


def marginals(h, rel=REL_DELTA):
    """number of elements of h within delta = rel max|h| of zero"""
    return int((h.abs() < rel * h.abs().max()).sum())


def _condition(t, hidden, W, gen, rel):
    """t (B,c,L) float32, hidden(t) -> float64 h (B,hid,L) with dh_j / dt_c = W[j, c] -> (t', touched (B,L) bool, passes,
    tokens redrawn).  One element of t per offending token and pass."""
    W = W.to(F64)
    best = W.abs().argmax(dim=1)                                       # (hid): the channel with the most say in row j
    touched = torch.zeros(t.shape[0], t.shape[2], dtype=torch.bool)
    passes = redrawn = 0
    for _ in range(4):
        for _ in range(MAX_PASSES):
            h = hidden(t)
            delta = rel * float(h.abs().max())
            marg = h.abs() < delta
            if not bool(marg.any()):
                return t, touched, passes, redrawn
            passes += 1
            b, l = marg.any(dim=1).nonzero(as_tuple=True)              # offending tokens
            j = marg[b, :, l].int().argmax(dim=1)                      # ... and the first offending row of each
            hj = h[b, j, l]
            want = 2.0 * delta * torch.where(hj < 0, -torch.ones_like(hj), torch.ones_like(hj))
            t64 = t.to(F64)
            t64[b, best[j], l] += (want - hj) / W[j, best[j]]
            t = t64.to(torch.float32)                                  # the device gets float32
            touched[b, l] = True
        b, l = (hidden(t).abs() < delta).any(dim=1).nonzero(as_tuple=True)
        t = t.clone()
        t[b, :, l] = torch.randn(len(b), t.shape[1], generator=gen)    # did not settle: a fresh token, and on
        touched[b, l] = True
        redrawn += len(b)
    raise AssertionError("conditioning did not settle")


def condition_tail(msg, res, p, gen, eps=NORM_EPS, rel=REL_DELTA):
    c1 = res.shape[1]
    return _condition(res, lambda r: tail_hidden(msg, r, p, eps), p["W0"][:, :c1], gen, rel)


def condition_head(xyz, p, gen, rel=REL_DELTA):
    return _condition(xyz, lambda z: head_hidden(z, p), p["P1"], gen, rel)


# ------------------------------------------------------------------------- the launch plans, restated --
TAIL_SHAPES = [(32, 32, 64, 32), (64, 64, 128, 64), (64, 64, 128, 128), (64, 32, 128, 64), (64, 3, 128, 32)]   # d c1 hid out
HEAD_SHAPES = [(32, 32, 32, 3, 7), (64, 64, 64, 3, 7), (64, 64, 64, 2, 2), (128, 64, 64, 2, 2), (64, 64, 64, 3, 4)]
# every instantiation: a tail with out == c1 runs with and without the residual
TAIL_FORMS = [(s, r) for s in TAIL_SHAPES for r in ((False, True) if s[3] == s[1] else (False,))]
# one shape per plan.  tails: two workgroups per CU | the only plan without a buffer of its own for d out | CU = 67 of
# CUP32 = 96 columns live; heads: two workgroups per CU | c = 128 | the one with an x-sourced and an fp-sourced projection
# beside an x-sourced first one
TAIL_PLANS = [((32, 32, 64, 32), True), ((64, 64, 128, 128), False), ((64, 3, 128, 32), False)]
HEAD_PLANS = [(32, 32, 32, 3, 7), (128, 64, 64, 2, 2), (64, 64, 64, 3, 4)]
MAX_LDS, ROW_PITCH = 160 * 1024, 65                                   # kMaxDynLds, kCRP


def c32(n):
    return (n + 31) // 32 * 32


def tail_sep(shape):
    """TailShape::SEP: d out has LDS rows of its own in the backward"""
    d, c1, hid, out = shape
    return (d + out + d + c32(c1 + d) + hid + out) * ROW_PITCH * 4 + 10 * TILE * 4 <= MAX_LDS


def tail_lds(shape, bwd=True):
    d, c1, hid, out = shape
    rows_a = (d + out if tail_sep(shape) else max(d, out)) if bwd else d
    return ((rows_a + d + c32(c1 + d) + hid + out) * ROW_PITCH + 10 * TILE) * 4


def head_lds(shape):
    c, hd, d, n, _ = shape
    return (32 + 2 * c + hd + n * d) * ROW_PITCH * 4


def groups_cap(lds, cus):
    """tail_grid / head_grid: the grid is min(tiles, CUs x min(occupancy, 2))"""
    return cus * min(max(MAX_LDS // lds, 1), 2)


def multi_tile_B(cap):
    """the smallest B whose 3 B tiles exceed 2 cap: with three tiles per cloud some workgroups then walk three tiles"""
    return 2 * cap // 3 + 1


def tail_rec(shape):
    d, c1, hid, out = shape
    return d * d + hid * c32(c1 + d) + out * hid + 2 * d + 2 * out


def head_rec(shape):
    c, hd, d, n, _ = shape
    return hd * 32 + c * hd + n * d * c + hd + c


# ---------------------------------------------------------------------------------------------- cases --
EDGE_BL = [(2, 1), (2, 63), (2, 64), (2, 65), (3, 100), (2, 130)]
NOMINAL_CUS = 256                     # the CPU file builds the multi-tile rows for this many CUs (the MI355X)
POS_LAYOUTS = [(6, 64), (3, 128), (4, 96), (2, 192)]
SHUT_ROWS = (1, 5, 17)                # head variant "shut": hidden units closed on every token


def multi_rows(cus=NOMINAL_CUS):
    """[(kind, form, B, L, ariths)]: L = 132 under every arithmetic, L = 131 (scalar stores) under bf16x3"""
    rows = []
    for L, ar in ((132, ARITHS), (131, ("bf16x3",))):
        rows += [("tail", f, multi_tile_B(groups_cap(tail_lds(f[0]), cus)), L, ar) for f in TAIL_PLANS]
        rows += [("head", s, multi_tile_B(groups_cap(head_lds(s), cus)), L, ar) for s in HEAD_PLANS]
    return rows


def all_cases(cus=NOMINAL_CUS):
    """the key of every case the GPU file builds: (kind, form, B, L, variant)"""
    keys = [("tail", f, B, L, "plain") for f in TAIL_FORMS for B, L in EDGE_BL]
    keys += [("head", s, B, L, "plain") for s in HEAD_SHAPES for B, L in EDGE_BL]
    keys += [(k, f, B, L, "plain") for k, f, B, L, _ in multi_rows(cus)]
    keys += [("tail", f, 6, 64, "pos") for f in TAIL_PLANS] + [("head", s, 6, 64, "pos") for s in HEAD_PLANS]
    keys += [("tail", TAIL_PLANS[1], 2, 128, "plain"), ("head", HEAD_PLANS[2], 2, 128, "plain")]       # unaligned base
    keys += [("head", s, 3, 100, "shut") for s in HEAD_SHAPES]
    keys += [("tail", f, 3, 100, "stress") for f in TAIL_PLANS] + [("head", s, 3, 100, "stress") for s in HEAD_PLANS]
    return keys


# a case whose draw needs more than MOVED_CAP of its tokens touched gets another seed here, never a wider cap
SALT = {("tail", ((64, 32, 128, 64), False), 2, 63, "plain"): 1, ("head", (64, 64, 64, 3, 7), 2, 63, "plain"): 1}


def _gen(key):
    return torch.Generator().manual_seed((zlib.crc32(repr(key).encode()) + SALT.get(key, 0)) % (2 ** 31))


def tail_params(shape, g):
    """the initialisation of test_gpu_train_chain.py's Tail: weights randn / sqrt(fan-in), gamma 1 + randn / 2, beta randn / 2"""
    d, c1, hid, out = shape
    r = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    return dict(Wm=r(d, d) / d ** 0.5, W0=r(hid, c1 + d) / (c1 + d) ** 0.5, W2=r(out, hid) / hid ** 0.5,
                g1=1.0 + 0.5 * r(d), b1=0.5 * r(d), g2=1.0 + 0.5 * r(out), b2=0.5 * r(out))


def head_params(shape, g):
    """... and of its Head: weights randn / sqrt(fan-in), biases 0.3 randn"""
    c, hd, d, n, _ = shape
    r = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    p = dict(P1=r(hd, 3) / 3 ** 0.5, c1=0.3 * r(hd), P2=r(c, hd) / hd ** 0.5, c2=0.3 * r(c))
    p.update({"W_%d" % j: r(d, c) / c ** 0.5 for j in range(n)})
    return p


def build_case(key):
    """-> dict(kind, form, p = parameters, the device inputs (msg, res | x, xyz) and dout as float32 CPU tensors, share =
    tokens touched by the conditioning / tokens, passes, redrawn).  Seeded from the key alone.  Variants: "plain"; "pos" (the
    base layout of the position-independence rows); "stress" (every token's channel mean of msg | x at 10 sigma, and in the
    tail gamma1 with one negative and one zero channel; conditioned after the edit); "shut" (head: the hidden units SHUT_ROWS
    closed on every token)."""
    kind, form, B, Ln, variant = key
    g = _gen(key)
    r = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    if kind == "tail":
        shape, residual = form
        d, c1, hid, out = shape
        p = tail_params(shape, g)
        msg, res, dout = r(B, d, Ln), r(B, c1, Ln), r(B, out, Ln)
        if variant == "stress":
            msg = msg + 10.0
            p["g1"][3], p["g1"][7] = -p["g1"][3].abs() - 0.5, 0.0
        res, touched, passes, redrawn = condition_tail(msg, res, p, g)
        case = dict(msg=msg, res=res, residual=residual)
    else:
        shape = form
        c, hd, d, n, src = shape
        p = head_params(shape, g)
        x, xyz, dout = r(B, c, Ln), r(B, 3, Ln), r(B, n * d, Ln)
        if variant == "stress":
            x = x + 10.0
        if variant == "shut":
            p["P1"][list(SHUT_ROWS)], p["c1"][list(SHUT_ROWS)] = 0.0, -1.0      # P1 xyz + c1 = -1 whatever the token
        xyz, touched, passes, redrawn = condition_head(xyz, p, g)
        case = dict(x=x, xyz=xyz, src=src)
    case.update(kind=kind, form=form, shape=shape, p=p, dout=dout, share=float(touched.float().mean()), passes=passes,
                redrawn=redrawn, key=key)
    return case


def relayout(t, B, Ln):
    """(B0,C,L0) -> (B,C,Ln): the same B0 L0 = B Ln tokens in the same order, cut into clouds of Ln"""
    C = t.shape[1]
    return t.permute(1, 0, 2).reshape(C, B, Ln).permute(1, 0, 2).contiguous()


def with_layout(case, B, Ln):
    out = dict(case)
    for k in ("msg", "res", "x", "xyz", "dout"):
        if k in case:
            out[k] = relayout(case[k], B, Ln)
    return out


# ---------------------------------------------------------------------------------------- evaluations --
def evaluate(case, dtype=F64, arith="f32", fault=None):
    """-> (out, dict of every gradient) of a case in `dtype` under the operand model `arith`"""
    p = {k: v.to(dtype) for k, v in case["p"].items()}
    dout = case["dout"].to(dtype)
    if case["kind"] == "tail":
        a = (case["msg"].to(dtype), case["res"].to(dtype), p["Wm"], p["g1"], p["b1"], p["W0"], p["W2"], p["g2"], p["b2"],
             case["residual"], NORM_EPS)
        return tail_ref(*a, arith=arith)[0], tail_bwd_ref(*a, dout, arith=arith, fault=fault)
    n = case["shape"][3]
    a = (case["x"].to(dtype), case["xyz"].to(dtype), p["P1"], p["c1"], p["P2"], p["c2"], [p["W_%d" % j] for j in range(n)])
    src = case["src"]
    fsrc = src & (src - 1) if fault == "src_x" else src
    return head_ref(*a, fsrc, arith=arith)[0], head_bwd_ref(*a, src, dout, arith=arith, fault=fault)


def rel(a, b):
    return float((a.to(F64) - b.to(F64)).abs().max()) / max(1e-30, float(b.abs().max()))


def out_blocks(case, out):
    """the forward output tensor by tensor: every projection of a head is held to its own norm"""
    if case["kind"] == "tail":
        return {"out": out}
    d = case["shape"][2]
    return {"out_%d" % j: out[:, j * d:(j + 1) * d] for j in range(case["shape"][3])}


def compare(case, got, want):
    """(out, grads) x 2 -> (worst forward rel, worst gradient rel, {tensor: rel})"""
    fo = {k: rel(v, out_blocks(case, want[0])[k]) for k, v in out_blocks(case, got[0]).items()}
    gr = {k: rel(got[1][k], want[1][k]) for k in want[1]}
    return max(fo.values()), max(gr.values()), {**fo, **gr}


def yardsticks(case, want=None):
    """-> dict(y32 = (forward, gradients): the float32 CPU evaluation against float64, max over tensors; ysplit[arith] =
    (forward, gradients): the operand model in float64 against float64)"""
    want = want or evaluate(case)
    y = dict(y32=compare(case, evaluate(case, torch.float32), want)[:2], ysplit={})
    for ar in ARITHS[1:]:
        y["ysplit"][ar] = compare(case, evaluate(case, F64, ar), want)[:2]
    return y


# (forward, gradients) against float64, per arithmetic: DESIGN's bound for norm compositions; its split-bf16 backward
# bound (the forward there is the f32 one); TOL["bf16x3_all"] of test_gpu_train_chain.py
BOUNDS = {"f32": (2e-5, 2e-5), "bf16x3": (2e-5, 3e-5), "bf16x3_all": (5e-5, 5e-5)}
YARD = 8.0                            # margin on a CPU yardstick (test_gpu_train_attn_ops.py)


def bounds(arith, yard=None):
    """plain rows: BOUNDS.  Stress rows (yard = yardsticks(case)): max(that, YARD x the row's own yardstick) -- y32 where the
    phase runs f32 chains, the larger of y32 and ysplit where it runs split bf16, which accumulates in float32 all the same"""
    bf, bg = BOUNDS[arith]
    if yard is None:
        return bf, bg
    yf, yg = yard["y32"]
    if arith != "f32":
        yg = max(yg, yard["ysplit"][arith][1])
    if arith == "bf16x3_all":
        yf = max(yf, yard["ysplit"][arith][0])
    return max(bf, YARD * yf), max(bg, YARD * yg)


@functools.lru_cache(maxsize=8)
def reference(key):
    """(case, (out, grads) in float64) of a key: computed once, shared, never modified"""
    case = build_case(key)
    return case, evaluate(case)
