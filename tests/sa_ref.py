"""The grouped set-abstraction layer (gather, three 1x1 convolutions with eval-mode BatchNorm, ReLU, max over K) in float64,
stated from models/pointnet2_utils.py:242-288, 333-360 -- and the shape rules of the library's dispatcher (sa_make_plan and
the launch-shape rules of csrc/sa_kernels_impl.h) restated as pure functions, so that a test can say which kernel
instantiation a shape reaches without running it.  tests/test_sa_ref_cpu.py holds both to a second formulation, to the
library's exported shape queries and to the form the library itself reports (pcr_sa_launch_form);
tests/test_gpu_sa_forms.py holds every launch form to `sa_ref`."""
import torch
import torch.nn as nn
import torch.nn.functional as F

F64 = torch.float64
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2}


# ---- the layer -------------------------------------------------------------------------------------------------------
def layer(mode, D, widths, seed=None):
    """three Conv2d(1x1) + BatchNorm2d(eval) with non-trivial running statistics; mode 0: cin = 3 + 2 D, mode 1: 3 + D"""
    seed = 17 + 1000 * mode + D + sum(widths) + 7 * widths[0] if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    cin = 3 + (2 * D if mode == 0 else D)
    convs, bns = [], []
    for a, b in zip((cin,) + tuple(widths[:2]), widths):
        conv, bn = nn.Conv2d(a, b, 1), nn.BatchNorm2d(b)
        with torch.no_grad():
            bound = 1.0 / a ** 0.5
            conv.weight.copy_((torch.rand(b, a, 1, 1, generator=g) * 2 - 1) * bound)
            conv.bias.copy_((torch.rand(b, generator=g) * 2 - 1) * bound)
            bn.running_mean.copy_(torch.randn(b, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(b, generator=g) + 0.5)
            bn.weight.copy_(torch.rand(b, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(b, generator=g) * 0.1)
        convs.append(conv)
        bns.append(bn.eval())
    return convs, bns


def grouped_input(mode, xyz, feat, idx, centre_idx=None, coord_centre_idx=None, dtype=F64):
    """(B,S,K,cin): mode 0 = edge features [rel, cf, nb - cf], mode 1 = [rel, nb]; the centres are the first S points
    (prefix) or centre_idx.  coord_centre_idx (planted faults only): another centre for the coordinates alone"""
    B, S, K = idx.shape
    li = idx.long().cpu()
    x = xyz.cpu().to(dtype)
    bidx = torch.arange(B).view(B, 1, 1)
    ci = (torch.arange(S).view(1, S).expand(B, S) if centre_idx is None else centre_idx.long().cpu()).unsqueeze(2)
    cc = ci if coord_centre_idx is None else coord_centre_idx.long().cpu().unsqueeze(2)
    parts = [x[bidx, li] - x[bidx, cc]]
    if feat is not None:
        f_pm = feat.cpu().to(dtype).transpose(1, 2)
        nb = f_pm[bidx, li]
        if mode == 0:
            cf = f_pm[bidx, ci].expand(-1, -1, K, -1)
            parts += [cf, nb - cf]
        else:
            parts.append(nb)
    return torch.cat(parts, dim=-1)


def sa_rows(convs, bns, mode, xyz, feat, idx, centre_idx=None, coord_centre_idx=None):
    """the layer before its maximum: (B,S,K,c3) in float64, the BatchNorm folded into weight and shift"""
    x = grouped_input(mode, xyz, feat, idx, centre_idx, coord_centre_idx)
    for conv, bn in zip(convs, bns):
        w = conv.weight.detach().double().reshape(conv.weight.shape[0], -1)
        sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
        sh = (conv.bias.detach().double() - bn.running_mean.double()) * sc + bn.bias.detach().double()
        x = torch.relu(x @ (w * sc.unsqueeze(1)).t() + sh)
    return x


def sa_ref(convs, bns, mode, xyz, feat, idx, centre_idx=None):
    """(B,c3,S) float64"""
    return sa_rows(convs, bns, mode, xyz, feat, idx, centre_idx).max(dim=2)[0].transpose(1, 2)


def sa_ref32(convs, bns, mode, xyz, feat, idx, centre_idx=None):
    """the same layer as unfused torch float32 ops (conv, BatchNorm, ReLU, max): a yardstick, never a reference"""
    with torch.no_grad():
        x = grouped_input(mode, xyz, feat, idx, centre_idx, dtype=torch.float32).permute(0, 3, 1, 2).contiguous()
        for conv, bn in zip(convs, bns):
            x = F.relu(bn(conv(x)))
        return x.max(dim=3)[0]


def groups(B, N, S, K, kind, g):
    """ball-query shaped groups (ball_query_cuda.cu:43-47): cnt genuine entries, the rest repeat entry 0 -- and a group's
    genuine entries are DISTINCT points, a prefix of a per-group permutation (N >= K), so that every row of a group can
    own a channel's maximum and a kernel that leaves one out is seen.  kind: "rand" | "ones" | "full"."""
    assert N >= K
    idx = torch.rand(B, S, N, generator=g).argsort(dim=-1)[:, :, :K].to(torch.int32)
    if kind == "ones":
        cnt = torch.ones(B, S, dtype=torch.int32)
    elif kind == "full":
        cnt = torch.full((B, S), K, dtype=torch.int32)
    else:
        cnt = torch.randint(1, K + 1, (B, S), generator=g, dtype=torch.int32)
        cnt[:, ::7] = 1
        cnt[:, 3::11] = K
    k = torch.arange(K).view(1, 1, K)
    idx = torch.where(k < cnt.unsqueeze(-1), idx, idx[:, :, :1].expand(-1, -1, K))
    return idx.contiguous(), cnt.contiguous()


def maxima_at_the_ends(idx, cnt, rows):
    """reorder every group's genuine entries -- the group's maximum does not change -- so that its LAST genuine row owns
    the maximum of one channel and its FIRST row that of another (channels s and s + 1 of centre s).  An estimate of what a
    random order leaves to chance: a given row owns a channel's maximum with chance 1 / K, so at K = 176 and 32 channels
    a group's last row owns none with (1 - 1/176)^32 = 0.83, and all nine groups of a B = 3, S = 3 case at once with
    0.83^9 = 0.19 -- one such case in five could not see a kernel that drops that row.
    rows: sa_rows of the same idx, (B,S,K,c3)."""
    B, S, K = idx.shape
    c3 = rows.shape[-1]
    out = idx.clone()
    for b in range(B):
        for s in range(S):
            n = int(cnt[b, s])
            if n >= 2:
                perm = list(range(n))
                pa = int(rows[b, s, :n, s % c3].argmax())
                perm[pa], perm[n - 1] = perm[n - 1], perm[pa]
                pb = perm.index(int(rows[b, s, :n, (s + 1) % c3].argmax()))
                if pb != n - 1:
                    perm[pb], perm[0] = perm[0], perm[pb]
                out[b, s, :n] = idx[b, s, perm]
            out[b, s, n:] = out[b, s, 0]
    return out.contiguous()


def row_table(xyz, idx, cnt, centre_idx=None):
    """the ball query's row table (pcr_ball_query_rows_f32) built from idx / cnt: per item of 16 centres, the rows of its
    centres back to back, ceil2(max(cnt, 1)) each: (point index as bits, dx, dy, dz)"""
    import numpy as np
    B, S, K = idx.shape
    tab = np.zeros((B, (S + 15) // 16, 16 * K, 4), dtype=np.float32)
    xn, cn, ixn = xyz.cpu().numpy(), cnt.cpu().numpy(), idx.cpu().numpy()
    cen = None if centre_idx is None else centre_idx.cpu().numpy()
    for b in range(B):
        for it in range((S + 15) // 16):
            r = 0
            for c in range(it * 16, min(S, it * 16 + 16)):
                ci = c if cen is None else int(cen[b, c])
                for k in range((max(int(cn[b, c]), 1) + 1) & ~1):
                    i = int(ixn[b, c, k])
                    tab[b, it, r, 0] = np.int32(i).view(np.float32)
                    tab[b, it, r, 1:] = xn[b, i] - xn[b, ci]
                    r += 1
    return torch.from_numpy(tab).reshape(-1)


# ---- the dispatcher's shape rules (sa_make_plan and the helpers above it, csrc/sa_kernels_impl.h) ---------------------
MAX_LDS = 160 * 1024


def ceil32(x):
    return (x + 31) & ~31


def ways(n):
    return 1 if n >= 3 else (2 if n == 2 else 4)


def tile_rows(c2, c3):
    return 64 if (ceil32(c2) > 128 or ceil32(c3) > 128) else 128


def tile_shape_ok(c2, c3):
    v = (ways(ceil32(c2) >> 5), ways(ceil32(c3) >> 5))
    return v == (1, 1) if tile_rows(c2, c3) == 64 else v in ((1, 1), (2, 1), (2, 2), (4, 4))


def wsplit_shape(c1, c2, c3, K):
    return (c1, c2, c3) == (128, 128, 256) and 1 <= K <= 64


def sas_k_ok(K):
    return K >= 1 and K % 16 == 0 and any((32 * nb) % K == 0 for nb in (1, 2, 3))


def sas_fixed_lds(c1, c3):
    ncb, ncb3 = c1 >> 5, c3 >> 5
    return (2 * ncb * ncb * 128 + 2 * ncb * ncb3 * 128) * 16 + (2 * c1 + c3) * 4 + ncb * 64 * 16


def sas_rag_lds(c1, c3, K, waves, tab):
    return sas_fixed_lds(c1, c3) + waves * (16 * c3 + (0 if tab else 16 * K) + ((16 * K // 2 + 15) // 16) * 4) * 4


def sas_shape(c1, c2, c3, K, both_forms):
    if c1 != c2 or c3 not in (c2, 2 * c2) or c1 not in (32, 64, 128) or not sas_k_ok(K):
        return False
    return sas_fixed_lds(c1, c3) + 16 <= MAX_LDS and (not both_forms or sas_rag_lds(c1, c3, K, 8, False) <= MAX_LDS)


def uses_row_table(c1, c2, c3, K, prec):
    return int(prec != 0 and tile_shape_ok(c2, c3) and sas_shape(c1, c2, c3, K, True))


def krow_uses_tiles(c1, c2, c3, K, prec):
    return int(prec != 0 and wsplit_shape(c1, c2, c3, K))


def tables_take_xyz(mode, D, c1, c2, c3, K, prec):
    return int(prec != 0 and mode == 0 and D >= 1 and c2 == c3 and sas_shape(c1, c2, c3, K, False))


def claim_ws_ints(c1, c2, c3, K, N, prec):
    if prec == 0 or c1 != c2 or c2 != c3 or K % 16 or K < 16:
        return 0
    return 8 * 1024 if (N >= 1024 and c1 <= 64 and c3 <= 64) else 0


def tile_ws_ints(B, S, K, c2, c3):
    if min(B, S, K, c2, c3) < 1 or K > tile_rows(c2, c3):
        return 0
    rows = tile_rows(c2, c3)
    per_tile = rows // ((K + 1) & ~1)
    maxT = (S + per_tile - 1) // per_tile
    flat = (((B + 2) & ~1) + B * 2 * maxT + 3) & ~3
    return flat + B * maxT * 4 + B * maxT * 4 + B * maxT * rows * 4


def krow_tile_choice(c1, c2, c3, K):
    """the K-row tile kernel's cost model: (cpw, TB) or None"""
    maxe = K % 16 == 0
    rowsC = max(c1, ceil32(c2), 0 if maxe else ceil32(c3))
    n2, n3 = ceil32(c2) >> 5, ceil32(c3) >> 5
    wy = ways(min(n2, n3))
    nr = 4 if max(n2, n3) > 8 else (2 if max(n2, n3) > 4 else 1)
    best, best_cost = None, 1e30
    for cpw in range(1, max(192 // K, 1) + 1):
        tb = (cpw * K + 31) // 32
        if tb > 6 or (nr == 4 and tb > 2):
            continue
        stage = max(6 * 32 * tb + cpw * c1 + 32, ceil32(c3) * 2 * tb if maxe else 0)
        lds = (rowsC * (32 * tb + 1) + stage) * 4
        tbw = (tb + wy - 1) // wy
        regs = nr * tbw * 16 + 70
        if lds > 150 * 1024 or regs > 250:
            continue
        wgs = min((160 * 1024) // ((lds + 2047) // 2048 * 2048), 512 // ((regs + 7) // 8 * 8), 8)
        if wgs < 1:
            continue
        cost = (32.0 * tb / (cpw * K)) * (float(tbw * wy) / tb) * (1.0 + 1.0 / wgs)
        if cost < best_cost - 1e-9:
            best, best_cost = (cpw, tb), cost
    return best


def _unit(prec, mode, D, c1, c2, c3, K, has_cnt, asked):
    """one arithmetic unit's sa_make_plan: (family, template arguments) or None (= -1, the caller goes on)"""
    if prec != 0 and ((c1 & 31) or (c2 & 31)):
        return None
    if (c1 & 7) or max(c1, c2, c3) > 512 or (D and (2 * c1 if mode == 0 else c1) > 1024):
        return None
    n1, n2, n3 = ceil32(c1) >> 5, ceil32(c2) >> 5, ceil32(c3) >> 5
    w1, w2, w3 = ways(n1), ways(n2), ways(n3)
    wsplit = prec != 0 and wsplit_shape(c1, c2, c3, K)
    ROWS = tile_rows(c2, c3)
    # (engine.SaPlan.run hands the tile workspace to ragged launches and to the cout-split shape, when K fits a tile)
    tile_ws = mode == 1 and K <= ROWS and (has_cnt or krow_uses_tiles(c1, c2, c3, K, asked))
    if tile_ws and (has_cnt or wsplit) and max(c1, c2, c3) <= 256:
        if prec != 0 and not tile_shape_ok(c2, c3):
            return None
        if prec != 0 and sas_shape(c1, c2, c3, K, True):
            ncb, ncb3 = c1 >> 5, c3 >> 5
            return ("stream_rag", (1, 1) if (ncb, ncb3) == (1, 1) else (1, 2) if ncb == 1 else (2, 2) if ncb3 == 2 else (2, 4))
        lds = (max(c1, ceil32(c2)) * (ROWS + 1) + ceil32(c3) * (ROWS // 2) + 3 * c1 + ceil32(c1) + ceil32(c2) + ceil32(c3) +
               8 * (ROWS + 1)) * 4
        if lds <= 150 * 1024:
            if prec != 0 and ROWS == 64 and wsplit:
                return ("wsplit", (4, 8))
            l1m = n1 <= 4
            if ROWS == 64:
                if (w2, w3) == (1, 1):
                    return ("rag_tile", (2, 2, 1, 1, 1, 1) if (n2 <= 4 and l1m and w1 == 1) else
                            (2, 2, 1, 1, 1, 0) if n2 <= 4 else (2, 2, 1, 1, 2, 0))
                return ("rag_tile", (2, 2, 0, 0, 1 if n2 <= 4 else 2, 0))           # (f32 unit only: tile_shape_ok above)
            if (w2, w3) == (1, 1):
                return ("rag_tile", (4, 1, 1, 1, 1, 0))
            if (w2, w3) == (2, 1):
                return ("rag_tile", (4, 1, 2, 1, 1, 2) if (l1m and w1 == 2 and not D) else (4, 1, 2, 1, 1, 0))
            if (w2, w3) in ((2, 2), (4, 4)):
                return ("rag_tile", (4, 1, w2, w3, 1, 0))
            return ("rag_tile", (4, 1, 0, 0, 1, 0))
    maxe = K % 16 == 0
    nr = 4 if max(n2, n3) > 8 else (2 if max(n2, n3) > 4 else 1)
    nr2 = 4 if nr == 4 else (2 if n2 > 4 else 1)
    if prec != 0 and (not maxe or nr > 2 or not (w2 == w3 or ((w2, w3) == (2, 1) and nr == 1))):
        return None
    choice = krow_tile_choice(c1, c2, c3, K)
    if choice is None:
        return None
    l1m = n1 <= 4 and n2 <= 4 and w1 == w2 and (prec != 0 or w2 == w3) and c1 % 4 == 0
    if prec != 0 and maxe and sas_shape(c1, c2, c3, K, mode == 1):
        return ("stream", (c1 >> 5, c3 >> 5))
    tb = choice[1]
    if prec != 0:
        if nr2 == 1 and not l1m:
            return None
        if (w2, w3) in ((4, 4), (2, 2), (2, 1)):
            form = (1, w2, w3)
        elif (w2, w3) == (1, 1):
            form = (1, 1, 1) if nr == 1 else (2, 1, 1, 1) if nr2 == 1 else (2, 1, 1)
        else:
            return None
        return ("krow_tile", (tb,) + form + ("maxe",))
    if nr == 4:
        form = (4, 1, 1, 4)
    elif w2 == w3 and w2 in (2, 4):
        form = (1, 4, 4, 1, 4) if (w2 == 4 and c1 <= 32 and c2 <= 32) else (1, w2, w3)
    elif w2 == w3:
        form = (1, 1, 1) if nr == 1 else (2, 1, 1, 1) if nr2 == 1 else (2, 1, 1)
    else:
        form = (1, 0, 0) if nr == 1 else (2, 0, 0, 1) if nr2 == 1 else (2, 0, 0)
    return ("krow_tile", (tb,) + form + ("maxe" if maxe else "full",))


def dispatch(mode, D, c1, c2, c3, K, precision, has_cnt, fast=True):
    """(unit that runs the launch: 0 f32 / 1 bf16x3 / 2 bf16, kernel family, template arguments).  has_cnt counts only
    in mode 1 (engine.SaPlan.run).  krow_tile: (TB, NR, W2, W3[, NR2[, RKB]], "maxe" | "full"); rag_tile: (TB, NR, A2,
    A3, NR2, W1); stream / stream_rag / wsplit: (NCB, NCB3)."""
    has_cnt = bool(has_cnt) and mode == 1
    if fast:
        for prec in ((precision, 0) if precision else (0,)):
            got = _unit(prec, mode, D, c1, c2, c3, K, has_cnt, precision)
            if got:
                return (prec,) + got
    return (0, "generic", ())


def generic_fits(mode, D, c1, c2, c3, K):
    """does the generic kernel hold one centre's K rows in LDS?  Where dispatch() says `generic` and this says no, the
    launch is refused (PCR_ERR_INVALID: sa_plan_generic) -- e.g. 128/128/128 without the fast operands at K >= 129
    (two 128-row buffers of 161 columns are 165 504 bytes)."""
    c8 = lambda x: (x + 7) & ~7                                                          # noqa: E731
    rows = max(c8(3 + (2 * D if mode == 0 else D)), c8(c2)) + max(c8(c1), c3)
    tb = (K + 31) // 32
    return (rows * (32 * tb + 1) + 32 * tb) * 4 <= MAX_LDS


def stream_rag_variant(c1, c3, K, with_table):
    """which of the ragged stream kernel's three forms: 12-wave table, 8-wave table, 8-wave index"""
    if not with_table:
        return "idx8"
    return "tab12" if sas_rag_lds(c1, c3, K, 12, True) <= MAX_LDS else "tab8"


FAMILIES = ("generic", "krow_tile", "rag_tile", "stream", "stream_rag", "wsplit")      # PCR_SA_* of include/pcr.h
VARIANTS = ("idx8", "tab8", "tab12")                                                  # form[2] of a stream_rag launch


def from_library(form):
    """pcr_sa_launch_form's ints -> (a dispatch() result, the ragged stream kernel's variant or None).  The library fills
    every template default in and adds the arguments the unit fixes (PREC, IMG, LO, TAB, WAVES), which are checked and
    dropped here.  dispatch() spells a K-row tile form the way its launcher does -- NR2 where it differs from NR, where
    RKB follows it, and in the four-round form -- so those defaults are taken out again."""
    unit, family, variant, n = form[:4]
    a, fam = tuple(form[4:4 + n]), FAMILIES[family]
    assert all(v == 0 for v in form[4 + n:]) and (variant == 0 or fam == "stream_rag")
    lo = int(unit == 1)
    if fam == "krow_tile":
        tb, nr, w2, w3, maxe, nr2, rkb, prec, img = a
        assert prec == unit and img == int(unit != 0 and nr2 == 1) and maxe in (0, 1)
        args = (tb, nr, w2, w3) + ((nr2, rkb) if rkb else (nr2,) if (nr2 != nr or nr == 4) else ()) + ("maxe" if maxe else "full",)
    elif fam == "rag_tile":
        args = a[:6]
        assert a[6:] == (unit,)
    elif fam in ("stream", "wsplit"):
        args = a[:2]
        assert a[2:] == (lo,)
    elif fam == "stream_rag":
        args = a[:2]
        assert a[2:] == (lo,) + ((0, 8), (1, 8), (1, 12))[variant]
    else:
        args = a
        assert a == () and unit == 0
    return (unit, fam, args), (VARIANTS[variant] if fam == "stream_rag" else None)


def form_name(d):
    """a dispatch() result as the text the row tables carry, e.g. 'f32 krow_tile<3,1,4,4,1,4,maxe>'"""
    unit, family, args = d
    return "%s %s<%s>" % (("f32", "bf16x3", "bf16")[unit], family, ",".join(str(a) for a in args))
