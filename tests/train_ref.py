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
their float32 inputs as they are -- no rounding precedes the decision, nothing to condition."""
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
