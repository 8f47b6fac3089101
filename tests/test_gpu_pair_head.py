"""GPU: the pair head over embeddings (pcr_pair_head_f32, csrc/pair_kernels.hip; pcr_amd/pairs_head.py) against the float64
restatement of tests/pair_ref.py (held to account by tests/test_pair_ref_cpu.py).

Rows (F, groups, M): (128, 32, 37) the config's shape, (64, 16, 5), (32, 8, 1); P over 1, 31, 33, 65, 1000 (one pair, one
short of a 32-pair tile, one past it, one past two tiles, many tiles); lists with i == j and repeated pairs; inputs times
1 and times 3.  Per row:
  (1) err = max|got - ref| / max|ref| <= 2e-6 (bound (1) of tests/test_gpu_dense_forms.py, the project's f32 bound); the
      same quantity of the yardstick route (torch.cat([emb[i], emb[j]]) + the dense / GroupNorm launches in f32 mode) is
      printed beside it;
  (2) a second run is bit-equal;
  (3) the first and the last pair scored alone, and a pair moved to another position, keep their bits;
  (4) logits inside a larger buffer filled with a NaN pattern: every word written, the neighbours untouched;
  (5) count in {0, 1, 37, P}: logits[:count] are the un-gated bits, logits[count:] dead_value exactly, and poisoning
      pairs[count:] with 2^30 changes nothing;
  (6) a live index of -1 or M gives NaN for that pair alone;
  (7) captured in a graph with count rewritten between replays (5 -> 2 -> 0), each replay equals its eager result;
  (8) refused shapes (F = 48; group size 2) raise and write nothing;
  (9) pcr_last_launch_arith() names f32."""
import ctypes

import pytest
import torch

import pair_ref as R

pytestmark = pytest.mark.gpu

ROWS = [(128, 32, 37), (64, 16, 5), (32, 8, 1)]
PS = (1, 31, 33, 65, 1000)
NAN_BITS = 0x7FC12345


def _head(inp):
    """the [LinearRes, Linear] module holding the row's weights"""
    from mmdet3d.models.lanegcn_nets import LinearRes
    n = inp["n"]
    res, out = LinearRes(n, n, norm="GN", ng=inp["groups"]), torch.nn.Linear(n, 1)
    assert res.norm1.num_groups == inp["groups"]
    with torch.no_grad():
        res.linear1.weight.copy_(inp["w1"])
        res.linear2.weight.copy_(inp["w2"])
        res.norm1.weight.copy_(inp["gn1_g"])
        res.norm1.bias.copy_(inp["gn1_b"])
        res.norm2.weight.copy_(inp["gn2_g"])
        res.norm2.bias.copy_(inp["gn2_b"])
        out.weight.copy_(inp["w_out"].view(1, -1))
        out.bias.copy_(inp["b_out"])
    return torch.nn.Sequential(res, out).cuda().eval()


class Case:
    def __init__(self, Fw, groups, M, scale, seed=0):
        from pcr_amd import pairs_head
        self.inp = R.make_inputs(Fw, groups, M, seed=seed, scale=scale)
        self.M = M
        self.head = _head(self.inp)
        self.plan = pairs_head.plan(self.head, torch.device("cuda", torch.cuda.current_device()))
        self.emb = self.inp["emb"].cuda()
        self.u, self.v = pairs_head.tables(self.plan, self.emb)

    def run(self, pairs, **kw):
        from pcr_amd import pairs_head
        return pairs_head.pair_logits(self.plan, self.emb, self.u, self.v, pairs, **kw)

    def yardstick(self, pairs):
        """the same logits through the launches the library already had: gathered rows + dense / GroupNorm, f32 mode"""
        from pcr_amd import engine, rows
        i, j = pairs[:, 0].long().cuda(), pairs[:, 1].long().cuda()
        x = torch.cat([self.emb[i], self.emb[j]], dim=1).t().contiguous().unsqueeze(0)
        with engine.precision("f32"):
            return rows.downsample_points(self.head, x).reshape(-1)


def dev_count(c):
    return torch.tensor([c], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("Fw,groups,M", ROWS)
def test_pair_head_row(Fw, groups, M):
    from pcr_amd import _lib as L
    fails = []
    for scale in (1.0, 3.0):
        case = Case(Fw, groups, M, scale)
        for P in PS:
            pairs = R.make_pairs(M, P, seed=P)
            ref = R.head_direct(case.inp, pairs)
            got = case.run(pairs.cuda())
            assert L.load().pcr_last_launch_arith() == 0                                          # (9) PCR_PREC_F32
            torch.cuda.synchronize()
            e, ey = R.err(got.cpu(), ref), R.err(case.yardstick(pairs).cpu(), ref)
            print("F=%d groups=%d M=%d x%g P=%d: err %.3g (%.2f of bound), yardstick route %.3g"
                  % (Fw, groups, M, scale, P, e, e / R.BOUND, ey))
            if not e <= R.BOUND:                                                                  # (1)
                fails.append("P=%d x%g: err %.3g > %.3g" % (P, scale, e, R.BOUND))
            if not torch.equal(case.run(pairs.cuda()), got):                                      # (2)
                fails.append("P=%d: a second run differs" % P)
            # (3) alone, and moved to another position
            for k in (0, P - 1):
                alone = case.run(pairs[k:k + 1].cuda())
                if not torch.equal(alone, got[k:k + 1]):
                    fails.append("P=%d: pair %d scored alone differs" % (P, k))
            if P >= 33:
                moved = torch.cat([pairs[7:], pairs[:7]]).cuda()
                if not torch.equal(case.run(moved), torch.cat([got[7:], got[:7]])):
                    fails.append("P=%d: the list rotated by 7 differs" % P)
            # (4) inside a larger buffer
            big = torch.full((P + 48,), NAN_BITS, dtype=torch.int32, device="cuda")
            view = big.view(torch.float32)[16:16 + P]
            case.run(pairs.cuda(), out=view)
            if not (big[:16] == NAN_BITS).all() or not (big[16 + P:] == NAN_BITS).all():
                fails.append("P=%d: words outside logits were written" % P)
            if not torch.equal(view, got):
                fails.append("P=%d: logits in a larger buffer differ / not every word written" % P)
            # (5) gating
            poisoned_all = torch.full_like(pairs, 2 ** 30).cuda()
            for c in sorted({0, 1, 37, P}):
                if c > P:
                    continue
                for pp in (pairs.cuda(), torch.cat([pairs[:c].cuda(), poisoned_all[c:]])):
                    g = case.run(pp, count=dev_count(c), dead_value=-7.5)
                    if not (torch.equal(g[:c], got[:c]) and bool((g[c:] == -7.5).all())):
                        fails.append("P=%d count=%d: gated logits differ" % (P, c))
            # (6) out-of-range indices
            for bad in (-1, M):
                for col in (0, 1):
                    k = P // 2
                    pb = pairs.clone()
                    pb[k, col] = bad
                    g = case.run(pb.cuda())
                    keep = torch.ones(P, dtype=torch.bool, device="cuda")
                    keep[k] = False
                    if not (bool(torch.isnan(g[k])) and torch.equal(g[keep], got[keep])):
                        fails.append("P=%d: index %d in column %d" % (P, bad, col))
    assert not fails, fails


@pytest.mark.parametrize("Fw,groups,M", ROWS)
def test_captured_graph_follows_the_count(Fw, groups, M):
    case = Case(Fw, groups, M, 1.0)
    P = 33
    pairs = R.make_pairs(M, P, seed=5).cuda()
    t = dev_count(5)
    out = torch.empty(P, dtype=torch.float32, device="cuda")
    want = {c: case.run(pairs, count=dev_count(c), dead_value=-1.0).clone() for c in (5, 2, 0)}      # eager (and warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.run(pairs, count=t, dead_value=-1.0, out=out)
    for c in (5, 2, 0):
        t.fill_(c)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[c]), c
        assert bool((out[c:] == -1.0).all())


def test_refused_shapes_raise_and_write_nothing():
    from pcr_amd import _lib as L
    from pcr_amd import abi, pairs_head
    dev = torch.device("cuda", torch.cuda.current_device())
    # through the wrapper: F = 48 (n = 96, groups of 8) and group size 2 (n = 64, 32 groups)
    for Fw, groups in ((48, 12), (32, 32)):
        inp = R.make_inputs(Fw, groups, 3, seed=1)
        with pytest.raises(L.PcrError):
            pairs_head.plan(_head(inp), dev)
    # and at the library's own boundary, with real tensors behind every pointer
    good = Case(32, 8, 3, 1.0)
    for Fw, groups in ((48, 12), (32, 32)):
        n = 2 * Fw
        logits = torch.full((8,), NAN_BITS, dtype=torch.int32, device="cuda")
        big = torch.zeros(3 * n * n, dtype=torch.float32, device="cuda")
        pairs = torch.zeros((8, 2), dtype=torch.int32, device="cuda")
        p = abi.PairHeadParams()
        p.M, p.F, p.n, p.groups, p.P = 3, Fw, n, groups, 8
        for f in ("emb", "u", "v", "w2p", "gn1_g", "gn1_b", "gn2_g", "gn2_b", "w_out", "b_out"):
            setattr(p, f, big.data_ptr())
        p.pairs, p.logits = pairs.data_ptr(), logits.data_ptr()
        with pytest.raises(L.PcrError, match="pcr_pair_head_f32 failed"):
            L.run.pcr_pair_head_f32(ctypes.byref(p), None, None, L.stream_ptr())
        torch.cuda.synchronize()
        assert bool((logits == NAN_BITS).all())
    assert good.run(R.make_pairs(3, 4, seed=0).cuda()).shape == (4,)
