"""float64 references of the PointNet / DGCNN training ops (pcr_amd.train_ops: BnAct, EdgeConvTrain, Bmm, PoolBoth,
ChannelMax) and the conditioning of their test inputs.  Plain torch on the CPU, written from each operation's
definition; nothing here imports pcr_amd.

Every maximum is routed by an EXPLICIT rule -- the first index attaining it (`first_argmax`) -- and gathered, so a tie
never depends on which index torch.max happens to return.  Gradients of the normalising ops come from autograd on the
float64 graph; the routed ones are also written out (`*_bwd_ref`).

Conditioning.  A float32 kernel and a float64 reference may legitimately disagree on a MARGINAL decision: the sign of
z = scale y + shift at an activation, or the winner of a max whose top two differ by rounding.  One flipped decision
moves a gradient by a whole |g|; no tolerance absorbs that, so such elements are removed from the INPUT (never masked
in a comparison).  delta = REL_DELTA max|z|: the kernel evaluates z as one multiply-add of float32 scale and shift,
error a few 2^-24 (|scale y| + |shift|) ~ 1e-6 max|z|, so delta leaves a margin of ~100 x that error.  Editing y moves
the batch statistics a little, hence the loops: they run until the float64 reference has ZERO marginal decisions, which
is what each test asserts before it launches anything.  `condition_signs` serves BnAct; in EdgeConvTrain the sign and
the winner of a row live in one table, so `condition_edge` applies the sign rule and the max rule (raise the winner of a
row whose top two differ by less than delta, bit-equal ties left alone) in one loop.  PoolBoth and ChannelMax compare
their float32 inputs as they are -- no rounding precedes the decision, nothing to condition.

The second half of the file does the same for the launches of the grouped-MLP path (SaEdgeTrain / dense): the
references of pcr_sa_l1_*, pcr_tdense_*, pcr_sa_pool_* and the two finalize launches as include/pcr.h states them, and
the conditioning of THEIR inputs, where scale and shift are inputs of a launch rather than batch statistics."""
import torch

F64 = torch.float64
REL_DELTA = 1e-4
MAX_PASSES = 50


# ------------------------------------------------------------------------------------------ selections --
def first_argmax(v, dim):
    """index of the FIRST entry along `dim` that attains the maximum"""
    n = v.shape[dim]
    shape = [1] * v.dim()
    shape[dim] = n
    pos = torch.arange(n).view(shape).expand(v.shape)
    at_max = v == v.amax(dim=dim, keepdim=True)
    return torch.where(at_max, pos, torch.full_like(pos, n)).amin(dim=dim)


def _top_gap(v, dim):
    """(maximum, maximum - runner-up) along dim; the gap of a single entry is +inf"""
    if v.shape[dim] < 2:
        mx = v.amax(dim=dim)
        return mx, torch.full_like(mx, float("inf"))
    top = v.topk(2, dim=dim).values
    return top.select(dim, 0), top.select(dim, 0) - top.select(dim, 1)


# ------------------------------------------------------------------------------------------- BatchNorm --
def _bn(y, gamma, beta, eps, dims):
    """training-mode BatchNorm over `dims` (channel = dim 1): z, batch mean, BIASED variance, scale = gamma invstd"""
    mean = y.mean(dim=dims, keepdim=True)
    var = ((y - mean) ** 2).mean(dim=dims, keepdim=True)
    shape = [1, -1] + [1] * (y.dim() - 2)
    scale = gamma.view(shape) / torch.sqrt(var + eps)
    return scale * (y - mean) + beta.view(shape), mean.flatten(), var.flatten(), scale


def _unbiased(var, R):
    return var * (R / (R - 1.0))


def bn_act_ref(y, gamma, beta, eps, act, slope=0.0):
    """y (B,C,L) float64 -> (z, batch mean, UNBIASED variance): z = act(BatchNorm(y)) with biased statistics over
    (B, L); act false: no activation, else z > 0 ? z : slope z.  The last two feed the running update."""
    z, mean, var, _ = _bn(y, gamma, beta, eps, (0, 2))
    if act:
        z = torch.where(z > 0, z, slope * z)
    return z, mean.detach(), _unbiased(var.detach(), y.shape[0] * y.shape[2])


def running_update(running, value, momentum, steps=1):
    """`steps` updates r <- (1 - m) r + m value with the same batch"""
    for _ in range(steps):
        running = (1.0 - momentum) * running + momentum * value
    return running


def edge_pre(tab, idx):
    """y[b,c,n,k] = tab[b,c,idx[b,n,k]] + tab[b,Co+c,n]: (B,Co,N,K)"""
    B, two_co, N = tab.shape
    Co = two_co // 2
    li = idx.long()
    nb = torch.stack([tab[b, :Co][:, li[b]] for b in range(B)])
    return nb + tab[:, Co:].unsqueeze(3)


def edge_conv_ref(tab, idx, gamma, beta, eps, slope):
    """tab (B,2Co,N) float64, idx (B,N,K) -> (pooled (B,Co,N), arg, batch mean, unbiased variance): BatchNorm over all
    B N K edges, LeakyReLU, max over k routed to the FIRST k attaining it"""
    y = edge_pre(tab, idx)
    z, mean, var, _ = _bn(y, gamma, beta, eps, (0, 2, 3))
    a = torch.where(z > 0, z, slope * z)
    arg = first_argmax(a.detach(), 3)
    pooled = torch.gather(a, 3, arg.unsqueeze(3)).squeeze(3)
    return pooled, arg, mean.detach(), _unbiased(var.detach(), y.shape[0] * y.shape[2] * y.shape[3])


# ------------------------------------------------------------------------------------------------- bmm --
def bmm_ref(x, T):
    """y[b,j,n] = sum_i T[b,i,j] x[b,i,n]"""
    return torch.einsum("bij,bin->bjn", T, x)


def bmm_bwd_ref(x, T, g):
    """(dx, dT) of bmm_ref for the output gradient g"""
    return torch.einsum("bij,bjn->bin", T, g), torch.einsum("bin,bjn->bij", x, g)


# --------------------------------------------------------------------------------------------- pooling --
def pool_both_ref(o):
    """o (P,C,L) -> (pooled (P,2C) = [max over L, mean over L], arg (P,C) = first position of the maximum)"""
    arg = first_argmax(o, 2)
    mx = torch.gather(o, 2, arg.unsqueeze(2)).squeeze(2)
    return torch.cat([mx, o.mean(dim=2)], dim=1), arg


def pool_both_bwd_ref(g, arg, L):
    """g (P,2C) -> dout (P,C,L): the max half to position arg, the mean half / L to every position"""
    P, C = arg.shape
    dout = (g[:, C:] / L).unsqueeze(2).expand(P, C, L).clone()
    dout.scatter_add_(2, arg.unsqueeze(2), g[:, :C].unsqueeze(2))
    return dout


def channel_max_ref(x, W):
    """x (B,C,L) -> (y (B,C/W,L) = max over windows of W consecutive channels, arg = the first winning CHANNEL)"""
    B, C, L = x.shape
    G = C // W
    xv = x.view(B, G, W, L)
    aw = first_argmax(xv, 2)
    y = torch.gather(xv, 2, aw.unsqueeze(2)).squeeze(2)
    return y, aw + W * torch.arange(G).view(1, G, 1)


def channel_max_bwd_ref(g, arg, C):
    """g (B,C/W,L) -> dx (B,C,L): each gradient to its winning channel"""
    B, _, L = g.shape
    dx = torch.zeros(B, C, L, dtype=g.dtype)
    dx.scatter_add_(1, arg, g)
    return dx


# ---------------------------------------------------------------------------------------- conditioning --
def _sign(z):
    return torch.where(z < 0, -torch.ones_like(z), torch.ones_like(z))


def marginal_signs(y, gamma, beta, eps, rel=REL_DELTA):
    """number of elements of the float32 input y (B,C,L) whose z = BatchNorm(y) lies within delta of zero"""
    z = _bn(y.to(F64), gamma.to(F64), beta.to(F64), eps, (0, 2))[0]
    return int((z.abs() < rel * z.abs().max()).sum())


def condition_signs(y, gamma, beta, eps, rel=REL_DELTA):
    """y (B,C,L) float32 -> (y', number of elements moved): every element with |z| < delta is moved to +- 2 delta
    (its own side) by editing y, re-rounded to float32, until none is left.  A channel with gamma = 0 has z = beta
    everywhere: nothing to edit, beta itself must be clear of zero."""
    gamma, beta = gamma.to(F64), beta.to(F64)
    moved = 0
    for _ in range(MAX_PASSES):
        y64 = y.to(F64)
        z, mean, _, scale = _bn(y64, gamma, beta, eps, (0, 2))
        delta = rel * float(z.abs().max())
        marg = (z.abs() < delta) & (scale != 0).expand_as(z)
        if not bool(marg.any()):
            break
        moved += int(marg.sum())
        safe = torch.where(scale != 0, scale, torch.ones_like(scale))
        want = mean.view(1, -1, 1) + (2.0 * delta * _sign(z) - beta.view(1, -1, 1)) / safe
        y = torch.where(marg, want, y64).to(torch.float32)
    return y, moved


def edge_marginals(tab, idx, gamma, beta, eps, rel=REL_DELTA):
    """(marginal signs, marginal winners) of the EdgeConv tail on the float32 table: rows (b,c,n) whose maximum over k
    lies within delta of zero, and rows whose top two differ by less than delta without being bit-equal"""
    z = _bn(edge_pre(tab.to(F64), idx), gamma.to(F64), beta.to(F64), eps, (0, 2, 3))[0]
    delta = rel * float(z.abs().max())
    mx, gap = _top_gap(z, 3)
    return int((mx.abs() < delta).sum()), int(((gap > 0) & (gap < delta)).sum())


def condition_edge(tab, idx, gamma, beta, eps, rel=REL_DELTA):
    """tab (B,2Co,N) float32 -> (tab', rows moved).  A row whose pooled z is within delta of zero is shifted as a whole
    to +- 2 delta through its centre entry tab[b,Co+c,n] (the gaps inside the row stay); a row whose winner leads by
    less than delta is given a lead of 2 delta by raising the winner's neighbour entry tab[b,c,idx[b,n,arg]].  Exact
    ties (bit-equal entries: a neighbour listed twice, duplicated points) are left alone: they are the tie-rule cases.
    An edit can disturb another row that lists the same neighbour, so this repeats until nothing is marginal."""
    gamma, beta = gamma.to(F64), beta.to(F64)
    B, two_co, N = tab.shape
    Co = two_co // 2
    li = idx.long()
    moved = 0
    for _ in range(MAX_PASSES):
        t64 = tab.to(F64)
        z, _, _, scale = _bn(edge_pre(t64, idx), gamma, beta, eps, (0, 2, 3))
        delta = rel * float(z.abs().max())
        mx, gap = _top_gap(z, 3)
        live = (scale != 0).view(1, Co, 1).expand_as(mx)
        near_zero = (mx.abs() < delta) & live
        near_tie = (gap > 0) & (gap < delta) & live
        if not bool(near_zero.any() | near_tie.any()):
            break
        moved += int(near_zero.sum()) + int(near_tie.sum())
        safe = torch.where(scale != 0, scale, torch.ones_like(scale)).view(1, Co, 1)
        centre = t64[:, Co:] + torch.where(near_zero, (2.0 * delta * _sign(mx) - mx) / safe, torch.zeros_like(mx))
        nb = t64[:, :Co].clone()
        b, c, n = torch.nonzero(near_tie, as_tuple=True)
        if b.numel():
            j = li[b, n, first_argmax(z, 3)[b, c, n]]
            nb[b, c, j] = nb[b, c, j] + (2.0 * delta - gap[b, c, n]) / safe[0, c, 0]
        tab = torch.cat([nb, centre], dim=1).to(torch.float32)
    return tab, moved


def knn_ref(feat, K):
    """feat (B,C,N) -> idx (B,N,K) int32: the K nearest points in feature space (squared distance in float64, the
    lower index first on a tie), the point itself included.  Stands in for the device's kNN where there is none."""
    f = feat.to(F64).permute(0, 2, 1)
    sq = (f * f).sum(dim=2)
    d = sq.unsqueeze(2) + sq.unsqueeze(1) - 2.0 * f @ f.transpose(1, 2)
    return torch.sort(d, dim=2, stable=True).indices[:, :, :K].to(torch.int32).contiguous()


# =================================================================================== grouped-MLP launches --
# float64 references of the set-abstraction training launches (include/pcr.h section C: pcr_sa_l1_*, pcr_tdense_*,
# pcr_sa_pool_*, pcr_bn_*_finalize), each written from the launch's stated contract.  Backward values come from autograd
# on these graphs; the launches' dy is an INPUT of the linear map (`tdense_dy`), so a gradient is
# torch.autograd.grad(forward, leaves, dy).
def _ch(v):
    return v.view(1, -1, 1)


def sa_l1_ref(xyz, idx, tab, wa, bias):
    """y[b,c,s K + k] = wa[c] . (xyz[idx[b,s,k]] - xyz[b,s]) + bias[c] + tab[b,c,idx[b,s,k]] + tab[b,c1 + c,s]: (B,c1,S K);
    tab None: no table terms.  Centres are the first S points."""
    B, S, K = idx.shape
    c1 = wa.shape[0]
    li = idx.long()
    nb = torch.stack([xyz[b][li[b]] for b in range(B)])                       # (B,S,K,3)
    y = torch.einsum("cj,bskj->bcsk", wa, nb - xyz[:, :S].unsqueeze(2)) + bias.view(1, c1, 1, 1)
    if tab is not None:
        y = y + torch.stack([tab[b, :c1][:, li[b]] for b in range(B)]) + tab[:, c1:, :S].unsqueeze(3)
    return y.reshape(B, c1, S * K)


def sa_l1_rows(xyz, feats, idx):
    """the materialised input rows [dxyz, f_c, f_i - f_c] of the grouped MLP's first layer: (B, 3 + 2 D, S K)"""
    B, S, K = idx.shape
    li = idx.long()
    d = torch.stack([xyz[b][li[b]] for b in range(B)]) - xyz[:, :S].unsqueeze(2)            # (B,S,K,3)
    rows = [d.permute(0, 3, 1, 2)]
    if feats is not None:
        fc = feats[:, :, :S].unsqueeze(3)                                                    # (B,D,S,1)
        fi = torch.stack([feats[b][:, li[b]] for b in range(B)])                             # (B,D,S,K)
        rows += [fc.expand_as(fi), fi - fc]
    return torch.cat(rows, dim=1).reshape(B, -1, S * K)


def tdense_in(x, x2, isc, ish, in_relu):
    """f([x ; x2]): [relu](isc x + ish) on the channels of x (isc None: identity, and no ReLU), x2 as it is"""
    f = x
    if isc is not None:
        f = _ch(isc) * x + _ch(ish)
        if in_relu:
            f = torch.relu(f)
    return f if x2 is None else torch.cat([f, x2], dim=1)


def tdense_ref(x, x2, W, bias, isc, ish, in_relu, res, out_relu, with_pre=False):
    """y = [relu](W f([x ; x2]) + bias [+ res]); with_pre: also the value before res / relu (what `stats` sums)"""
    pre = torch.einsum("oc,bcl->bol", W, tdense_in(x, x2, isc, ish, in_relu))
    if bias is not None:
        pre = pre + _ch(bias)
    y = pre if res is None else pre + res
    if out_relu:
        y = torch.relu(y)
    return (y, pre) if with_pre else y


def stats_ref(y):
    """(2, C): sum and sum of squares over (B, L)"""
    return torch.stack([y.sum(dim=(0, 2)), (y * y).sum(dim=(0, 2))])


def route_ref(gp, argmax, pooled, K):
    """gp (B,C,S) -> (B,C,S K): every centre's gradient at row argmax of its K rows where pooled > 0 (pooled None: gp is
    zero there already), zero elsewhere"""
    B, C, S = gp.shape
    sel = gp if pooled is None else torch.where(pooled > 0, gp, torch.zeros_like(gp))
    full = torch.zeros(B, C, S, K, dtype=gp.dtype)
    full.scatter_(3, argmax.long().unsqueeze(3), sel.unsqueeze(3))
    return full.reshape(B, C, S * K)


def tdense_dy(mode, g, y=None, k=None, argmax=None, pooled=None, K=0):
    """the dy a backward launch forms while it loads its tiles: 0: g; 1: ka g + kb y + kc; 2: g [y > 0]; 3: as 1 on the
    routed pooled gradient"""
    if mode == 0:
        return g
    if mode == 2:
        return torch.where(y > 0, g, torch.zeros_like(g))
    if mode == 3:
        g = route_ref(g, argmax, pooled, K)
    return _ch(k["ka"]) * g + _ch(k["kb"]) * y + _ch(k["kc"])


def tdense_bwd_ref(dy, x, x2, W, isc, ish, in_relu):
    """float64 inputs -> dict(dx, dx2, dW, db, dstats): autograd of sum(dy (W f([x ; x2]) + bias)) -- dx is the gradient
    at f's ReLU ARGUMENT (masked by f > 0, not multiplied by isc: the BatchNorm backward below it does that through ka);
    dstats = (sum dx, sum dx x) per channel of x"""
    z = x if isc is None else _ch(isc) * x + _ch(ish)
    z = z.detach().requires_grad_(True)
    x2l = None if x2 is None else x2.detach().requires_grad_(True)
    Wl = W.detach().requires_grad_(True)
    bl = torch.zeros(W.shape[0], dtype=W.dtype, requires_grad=True)
    f = torch.relu(z) if (in_relu and isc is not None) else z
    pre = torch.einsum("oc,bcl->bol", Wl, f if x2l is None else torch.cat([f, x2l], dim=1)) + _ch(bl)
    leaves = [z, Wl, bl] + ([x2l] if x2l is not None else [])
    grads = torch.autograd.grad(pre, leaves, dy)
    dx = grads[0]
    return dict(dx=dx, dW=grads[1], db=grads[2], dx2=grads[3] if x2l is not None else None,
                dstats=torch.stack([dx.sum(dim=(0, 2)), (dx * x).sum(dim=(0, 2))]))


def sa_pool_ref(y, scale, shift, K):
    """y (B,C,S K) -> (pooled (B,C,S) = max_k relu(scale y + shift), the FIRST k attaining it, the raw y at that row)"""
    B, C, Ln = y.shape
    yv = y.view(B, C, Ln // K, K)
    a = torch.relu(scale.view(1, C, 1, 1) * yv + shift.view(1, C, 1, 1))
    arg = first_argmax(a, 3)
    return (torch.gather(a, 3, arg.unsqueeze(3)).squeeze(3), arg, torch.gather(yv, 3, arg.unsqueeze(3)).squeeze(3))


def pool_bwd_stats_ref(gp, pooled, ymax):
    """-> (gz = gp [pooled > 0], (2, C) sums S1 = sum gz, S2 = sum gz ymax over (B, S))"""
    gz = torch.where(pooled > 0, gp, torch.zeros_like(gp))
    return gz, torch.stack([gz.sum(dim=(0, 2)), (gz * ymax).sum(dim=(0, 2))])


def bn_fwd_consts_ref(part, C, R, gamma, beta, eps, shift0=None):
    """part (nparts, 2, CP) float64 partial sums of (y - shift0) and its square over R rows -> dict(mean, var (biased,
    clamped at zero), unbiased (R = 1: the biased one), invstd, scale = gamma invstd, shift = beta - mean scale,
    inv_scale = 1 / scale, 0 where scale is 0)"""
    s = part.sum(dim=0)[:, :C]
    mean0 = s[0] / R
    var = (s[1] / R - mean0 * mean0).clamp_min(0.0)
    mean = mean0 if shift0 is None else mean0 + shift0
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    inv = torch.where(scale != 0, 1.0 / torch.where(scale != 0, scale, torch.ones_like(scale)), torch.zeros_like(scale))
    return dict(mean=mean, var=var, unbiased=var * (R / (R - 1.0)) if R > 1 else var, invstd=invstd, scale=scale,
                shift=beta - mean * scale, inv_scale=inv)


def bn_bwd_consts_ref(part, C, R, gamma, mean, invstd, centre=None):
    """part (nparts, 2, CP) float64 partials of S1 = sum dyhat, S2 = sum dyhat (y - centre) -> dict(dbeta = S1, dgamma =
    invstd (S2 - (mean - centre) S1), ka = gamma invstd, kb = -ka dgamma invstd / R, kc = ka (dgamma invstd mean - S1) / R):
    dy = ka dyhat + kb y + kc is the BatchNorm backward"""
    s = part.sum(dim=0)[:, :C]
    off = mean if centre is None else mean - centre
    dgamma = invstd * (s[1] - off * s[0])
    ka = gamma * invstd
    return dict(dbeta=s[0], dgamma=dgamma, ka=ka, kb=-ka * dgamma * invstd / R, kc=ka * (dgamma * invstd * mean - s[0]) / R)


# ---- conditioning of the grouped-MLP inputs.  Here isc / ish are INPUTS of a launch, not batch statistics: one pass.
def relu_arg_marginals(x, isc, ish, rel=REL_DELTA):
    """number of elements of the float32 x (B,C,L) whose ReLU argument isc x + ish lies within delta of zero"""
    z = _ch(isc.to(F64)) * x.to(F64) + _ch(ish.to(F64))
    return int((z.abs() < rel * z.abs().max()).sum())


def condition_relu_args(x, isc, ish, rel=REL_DELTA):
    """x (B,C,L) float32 -> (x', moved): every ReLU argument z = isc x + ish with |z| < delta = rel max|z| goes to
    +- 2 delta on its own side by editing x (isc != 0)"""
    sc, sh = _ch(isc.to(F64)), _ch(ish.to(F64))
    z = sc * x.to(F64) + sh
    delta = rel * float(z.abs().max())
    marg = z.abs() < delta
    want = (2.0 * delta * _sign(z) - sh) / sc
    return torch.where(marg, want, x.to(F64)).to(torch.float32), int(marg.sum())


def value_marginals(y, rel=REL_DELTA):
    """number of elements of the float64 y within delta = rel max|y| of zero (the ReLU argument of an out_relu launch)"""
    return int((y.abs() < rel * y.abs().max()).sum())


def condition_out_relu(y_of, res, x, W, rel=REL_DELTA):
    """the ReLU argument y = y_of(x, res) (float64, from the float32 inputs) of an out_relu launch: every |y| < delta goes
    to +- 2 delta on its own side -- through res (B,cout,L) where the launch has one (an element of res moves one element
    of y), else through x (B,cin,L, no input ReLU): the token's column moves along W[o], the smallest change that moves
    y[b,o,l] by the wanted amount; that disturbs the token's other outputs a little, hence the passes.
    -> (x', res', moved)"""
    moved = 0
    for _ in range(MAX_PASSES):
        y = y_of(x, res)
        delta = rel * float(y.abs().max())
        marg = y.abs() < delta
        if not bool(marg.any()):
            return x, res, moved
        moved += int(marg.sum())
        step = torch.where(marg, 2.0 * delta * _sign(y) - y, torch.zeros_like(y))
        if res is not None:
            res = (res.to(F64) + step).to(torch.float32)
        else:
            W64 = W.to(F64)[:, :x.shape[1]]               # (the columns of x; an x2 behind them stays)
            x = (x.to(F64) + torch.einsum("oc,bol->bcl", W64 / (W64 * W64).sum(dim=1, keepdim=True), step)).to(torch.float32)
    raise AssertionError("conditioning did not settle")


def pool_marginals(y, scale, shift, K, rel=REL_DELTA):
    """(rows whose largest z = scale y + shift lies within delta of zero, rows whose top two z differ by less than delta
    without being bit-equal) of the float32 y (B,C,S K); channels with scale = 0 hold z = shift everywhere"""
    B, C, Ln = y.shape
    z = (scale.to(F64).view(1, C, 1, 1) * y.to(F64).view(B, C, Ln // K, K) + shift.to(F64).view(1, C, 1, 1))
    delta = rel * float(z.abs().max())
    mx, gap = _top_gap(z, 3)
    return int((mx.abs() < delta).sum()), int(((gap > 0) & (gap < delta)).sum())


def condition_pool(y, scale, shift, K, rel=REL_DELTA):
    """y (B,C,S K) float32 -> (y', rows moved): a row (b,c,s) whose winner leads by less than delta gets a lead of 2 delta
    (the winner's y is moved), then a row whose pooled z is within delta of zero is shifted as a whole to +- 2 delta.
    Bit-equal ties stay.  The two edits do not disturb each other or another row: one pass."""
    B, C, Ln = y.shape
    sc, sh = scale.to(F64).view(1, C, 1, 1), shift.to(F64).view(1, C, 1, 1)
    safe = torch.where(sc != 0, sc, torch.ones_like(sc))
    yv = y.to(F64).view(B, C, Ln // K, K).clone()
    z = sc * yv + sh
    delta = rel * float(z.abs().max())
    live = (sc != 0).view(1, C, 1).expand(B, C, Ln // K)
    mx, gap = _top_gap(z, 3)
    near_tie = (gap > 0) & (gap < delta) & live
    dz = torch.zeros_like(z).scatter_add(3, first_argmax(z, 3).unsqueeze(3),
                                         torch.where(near_tie, 2.0 * delta - gap, torch.zeros_like(gap)).unsqueeze(3))
    mx = (z + dz).amax(dim=3)
    near_zero = (mx.abs() < delta) & live
    dz = dz + torch.where(near_zero, 2.0 * delta * _sign(mx) - mx, torch.zeros_like(mx)).unsqueeze(3)
    yv = torch.where(dz != 0, yv + dz / safe, yv)
    return yv.reshape(B, C, Ln).to(torch.float32), int(near_tie.sum()) + int(near_zero.sum())


def condition_bn_through(make_y, push, gamma, beta, eps, rel=REL_DELTA):
    """BatchNorm + ReLU on a launch's OUTPUT y = make_y() (float64 (B,C,L), from float32 inputs): every z = BatchNorm(y)
    within delta of zero goes to +- 2 delta by push(dy), which edits the inputs so that y moves by the sparse dy.  The
    statistics move with the edit: repeated until nothing is marginal.  -> number of elements moved"""
    gamma, beta = gamma.to(F64), beta.to(F64)
    moved = 0
    for _ in range(MAX_PASSES):
        y = make_y()
        z, _, _, scale = _bn(y, gamma, beta, eps, (0, 2))
        delta = rel * float(z.abs().max())
        marg = (z.abs() < delta) & (scale != 0).expand_as(z)
        if not bool(marg.any()):
            return moved
        moved += int(marg.sum())
        safe = torch.where(scale != 0, scale, torch.ones_like(scale))
        push(torch.where(marg, (2.0 * delta * _sign(z) - z) / safe, torch.zeros_like(z)))
    raise AssertionError("conditioning did not settle")
