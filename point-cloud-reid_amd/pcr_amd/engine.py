"""Host side of the fused model kernels (include/pcr.h, section B): weight packing, eval-mode
BatchNorm folding, parameter structs and launches.  PyTorch only supplies device memory and the
current HIP stream.  Every entry point requires device tensors and raises if libpcr_hip.so is
missing -- there is no CPU path here (the CPU restatement lives under oracle/ and is test-only).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from ._lib import _p
from .abi import AttnParams, HeadParams, LiveParams, SaParams

# Arithmetic of the MFMA-bound layers (include/pcr.h PCR_PREC_*):
#   "f32"    f32-input MFMA, exact fmaf chains (the reference's arithmetic, 157 TFLOP/s peak);
#   "bf16x3" split bf16: every product as three bf16 MFMAs with f32 accumulation -- logits within 2-3e-5 of "f32" on
#            the bench batches (a fifth of the 1e-4 parity bound; tests/test_gpu_precision.py sweeps input scale,
#            weight seeds and BatchNorm statistics), every golden inside 1e-4 -- at ~5x the rate per product;
#   "bf16"   plain bf16 activations / weights, f32 accumulation: BASELINE config 2 as stated; ~1e-3 on the logits.
# Default "bf16x3"; PCR_PRECISION in the environment or set_precision() change it (plans are rebuilt lazily because
# the launch parameter is read per call).
import os as _os
PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2}
PRECISION = _os.environ.get("PCR_PRECISION", "bf16x3")
if PRECISION not in PRECISIONS:
    raise L.PcrError("PCR_PRECISION must be one of %s" % sorted(PRECISIONS))


KV_SPLITS = int(os.environ["PCR_KV_SPLITS"]) if os.environ.get("PCR_KV_SPLITS") else None   # None: pcr_attn_kv_splits
# decides; an int forces the token split of the attention kv launches (tests, tuning)


def set_precision(name):
    """-> previous setting"""
    global PRECISION
    if name not in PRECISIONS:
        raise L.PcrError("precision must be one of %s" % sorted(PRECISIONS))
    prev, PRECISION = PRECISION, name
    return prev


class precision:
    """with engine.precision("f32"): ..."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = set_precision(self.name)

    def __exit__(self, *exc):
        set_precision(self.prev)
        return False


# ---- split-bf16 guard (round 5) --------------------------------------------------------------------
# "bf16x3" drops the lo x lo term of every product: ~2^-17 of |w| |x| per term.  Against the 1e-4 parity bound that is a
# comfortable 1-3e-5 on the logits for the seeded weights, but a checkpoint whose FOLDED BatchNorm layers cancel large
# terms (running statistics far from the data: variance / 4 with means x 3 put the SSG logits at 9.7e-5) spends nearly
# all of it.  Nothing in the weights alone tells -- the cancellation depends on the data -- and neither does the deviation
# of a single launch (measured, tools/guard_sweep.py: the grouped-SA launches deviate by 0.8-1.1e-5 of their output's
# scale for the seeded AND for the shifted statistics; what differs is how the layers behind them amplify it).  So the
# guard measures what the bound is about: ReIDNet.calibrate_precision() runs the hot path on a calibration batch in f32
# and in split bf16 and picks, per model and weight version, the first LEVEL whose logits stay within GUARD_BOUND (half the
# parity bound) of the f32 path's:
#   0  every matrix phase in split bf16 (what "bf16x3" means for a well-conditioned checkpoint);
#   1  the launches that carry folded BatchNorm scales (the grouped SA MLPs: `guarded`) in f32, the rest in split bf16;
#   2  the whole path in f32.
# ReIDNet applies the level on every inference entry point, and every one of them that sees raw clouds (siamese_forward,
# forward_inference, forward_test; the match-only ones through the xyz they are handed) calibrates on its first batch
# after the weights changed (round 6; ADVICE r5: the tracker entry points ran unguarded until calibrate_precision was
# called by hand); bench.py calibrates before its capture (and reports level + measured deviations as config.guard).
# Run-time SENTINEL (round 6): the cancellation is data dependent, so one calibration batch is a
# margin, not a property -- every GUARD_EVERY-th inference batch of a weight version, up to GUARD_SENTINEL_PAIRS pairs of
# the LIVE batch (rotating through it) are re-run in f32 and at the current level BEFORE the batch itself is computed;
# on a breach of GUARD_BOUND the level of that weight version is raised to the first one that holds and the event is
# logged ("pcr_amd.guard") and kept in guard_state()["sentinel"].  The bound is half the parity bound, so a drift is
# caught at 5e-5 on the sample before it costs 1e-4 on a logit; PCR_GUARD_EVERY=1 checks every batch (a property at
# ~2 x 8 small pairs per batch), 0 switches the sentinel off.  Nothing is measured inside a HIP-graph capture (host
# reads): captured launches keep the level the model had when they were captured.
# PCR_GUARD=0 switches the guard off; PCR_GUARD_BOUND moves the bound.
GUARD = _os.environ.get("PCR_GUARD", "1") != "0"
GUARD_BOUND = float(_os.environ.get("PCR_GUARD_BOUND", "5e-5"))
# CALIBRATION accepts a level only at GUARD_ACCEPT x the bound: the deviation of a fresh batch of the same distribution was
# measured at up to 1.3x (near the bound; 1.5x further below it) that of the calibration batch (tools/guard_cases.py,
# profiles/r06m_guard_cases.txt: a 128-point Point-Transformer at input scale 0.1 calibrated at 4.65e-5 and returned 5.95e-5
# on the next batch).  The sentinel keeps the bound itself: it measures the live batch.
GUARD_ACCEPT = float(_os.environ.get("PCR_GUARD_ACCEPT", "0.9"))
GUARD_EVERY = int(_os.environ.get("PCR_GUARD_EVERY", "64"))
GUARD_SENTINEL_PAIRS = int(_os.environ.get("PCR_GUARD_SENTINEL_PAIRS", "8"))
_LEVEL = 0


class guard_level:
    """with engine.guard_level(n): the launches inside run at guard level n (see above); a no-op unless the arithmetic
    mode is bf16x3"""

    def __init__(self, level):
        self.level = int(level)

    def __enter__(self):
        global _LEVEL
        self.prev_level, _LEVEL = _LEVEL, self.level
        self.prev_prec = set_precision("f32") if (self.level >= 2 and PRECISION == "bf16x3") else None

    def __exit__(self, *exc):
        global _LEVEL
        _LEVEL = self.prev_level
        if self.prev_prec is not None:
            set_precision(self.prev_prec)
        return False


def guarded(fn):
    """fn() = the launches of a plan that carries folded BatchNorm scales: in f32 from guard level 1 on"""
    if _LEVEL >= 1 and PRECISION == "bf16x3":
        with precision("f32"):
            return fn()
    return fn()


# claimed work items for the wave-autonomous K-row SA kernel on clouds of >= 1024 points (pcr_sa_params.claim_ws, ABI 16;
# PCR_SA_CLAIMS=0 / engine.SA_CLAIMS = False: fixed-stride items -- same bits, tests/test_gpu_sa_claims.py)
SA_CLAIMS = _os.environ.get("PCR_SA_CLAIMS", "1") != "0"

# tables WITH the coordinate term for the wave-autonomous K-row SA kernel in the bf16 modes (pcr_dense_pm_xyz_f32 /
# pcr_sa_params.pq_has_xyz, ABI 17; PCR_SA_XYZ_TABLES=0 / engine.SA_XYZ_TABLES = False: the coordinate term on the matrix core
# inside the launch, as in the f32 mode -- tests/test_gpu_sa_xyz_tables.py holds the two forms against each other)
SA_XYZ_TABLES = _os.environ.get("PCR_SA_XYZ_TABLES", "1") != "0"

# bench.py sets this to a list to collect (kernel, start_event, end_event, algorithmic flops,
# algorithmic bytes, issued flops, arithmetic) per launch; events are recorded on the stream the kernels are launched on.
PROFILE = None
ARITH_NAMES = {0: "f32", 1: "bf16x3", 2: "bf16"}


class _prof:
    def __init__(self, name, flops=0.0, nbytes=0.0, exec_flops=None, arith=None):
        # flops: the reference's op count for this piece of work (what "achieved" is quoted against);
        # exec_flops: what the launch really issues on the matrix core, where the two differ;
        # arith: "lib" = ask the library which arithmetic the launch REALLY ran its matrix phases in
        # (pcr_last_launch_arith: a requested precision is only a request), a name = fixed, None = not a matrix launch
        self.name, self.flops, self.nbytes, self.arith = name, flops, nbytes, arith
        self.exec_flops = flops if exec_flops is None else exec_flops

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e1.record()
            arith = self.arith
            if arith == "lib":
                arith = ARITH_NAMES.get(L.load().pcr_last_launch_arith(), "f32")
            PROFILE.append((self.name, self.e0, self.e1, self.flops, self.nbytes, self.exec_flops, arith))
        return False


def _dev32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def pack_weight(w, device):
    """(cout, cin[, 1[, 1]]) weight -> packed MFMA A-operand image on `device` (host-side pack)."""
    w2 = w.detach().reshape(w.shape[0], -1).to("cpu", torch.float32).contiguous().numpy()
    cout, cin = w2.shape
    lib = L.load()
    n = lib.pcr_packed_weight_floats(cout, cin)
    out = np.empty(n, np.float32)
    L.run.pcr_pack_weight_f32(w2.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p))
    return torch.from_numpy(out).to(device)


def pack_weight_bf(w, device):
    """(cout, cin[, 1[, 1]]) weight -> bf16 hi / lo image for the bf16 matrix core (pcr_pack_weight_bf16x2_f32)"""
    w2 = w.detach().reshape(w.shape[0], -1).to("cpu", torch.float32).contiguous().numpy()
    cout, cin = w2.shape
    lib = L.load()
    n = lib.pcr_packed_weight_bf16_floats(cout, cin)
    out = np.empty(n, np.float32)
    L.run.pcr_pack_weight_bf16x2_f32(w2.ctypes.data_as(ctypes.c_void_p), cout, cin,
                                     out.ctypes.data_as(ctypes.c_void_p))
    return torch.from_numpy(out).to(device)


def pack_weight_dual(w, device):
    """the packed f32 image of `w` with its bf16 hi / lo image attached (`._pcr_bf`): what `dense` / `rows.dense_gn` need to
    run a wide per-point layer on the bf16 matrix core in the "bf16x3" / "bf16" modes (pcr_dense_prec_f32); layers whose
    shape the bf16 kernel does not cover simply never look at it"""
    wp = pack_weight(w, device)
    cout, cin = w.shape[0], int(np.prod(w.shape[1:]))
    if L.load().pcr_dense_prec_ok(cin, cout, 1) or L.load().pcr_dense_xpm_prec_ok(cin, cout, 1):
        wp._pcr_bf = pack_weight_bf(w, device)
    return wp


def fold_bn(bn, conv_bias, device):
    """eval-mode BatchNorm after a conv with bias -> per-channel (scale, shift) applied to W x."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    bias = conv_bias.detach().double() if conv_bias is not None else 0.0
    shift = (bias - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()
    return _dev32(scale.float(), device), _dev32(shift.float(), device)


def param_version(module):
    """cheap fingerprint of a module's parameters/buffers: re-pack when anything was updated"""
    return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))


# ------------------------------------------------------------------------------ launches --
def knn_prefix(xyz, S, K):
    """xyz (B,N,3) device -> idx (B,S,K) int32: K nearest of all N for the first S points."""
    L.require_cuda(xyz)
    assert xyz.is_contiguous() and xyz.dtype == torch.float32
    B, N, _ = xyz.shape
    idx = torch.empty((B, S, K), dtype=torch.int32, device=xyz.device)
    with _prof("knn_prefix[N=%d,S=%d,K=%d]" % (N, S, K), 8.0 * B * S * N, 12.0 * B * N + 4.0 * B * S * K):
        L.run.pcr_knn_prefix_f32(xyz, idx, B, N, S, K, L.stream_ptr())
    return idx


def knn_prefix2(xyz, S, K, S2, K2):
    """two levels on the same cloud in one launch (pcr_knn_prefix2_f32): -> idx (B,S,K), idx2 (B,S2,K2), entry for entry
    what knn_prefix(xyz, S, K) and knn_prefix(xyz, S2, K2) return; S2 <= S, K2 >= K"""
    L.require_cuda(xyz)
    assert xyz.is_contiguous() and xyz.dtype == torch.float32 and S2 <= S and K2 >= K
    B, N, _ = xyz.shape
    if S2 == 0 or B == 0:
        return knn_prefix(xyz, S, K), torch.empty((B, S2, K2), dtype=torch.int32, device=xyz.device)
    idx = torch.empty((B, S, K), dtype=torch.int32, device=xyz.device)
    idx2 = torch.empty((B, S2, K2), dtype=torch.int32, device=xyz.device)
    with _prof("knn_prefix2[N=%d,S=%d,K=%d,S2=%d,K2=%d]" % (N, S, K, S2, K2), 8.0 * B * S * N,
               12.0 * B * N + 4.0 * B * (S * K + S2 * K2)):
        L.run.pcr_knn_prefix2_f32(xyz, idx, idx2, B, N, S, K, S2, K2, L.stream_ptr())
    return idx, idx2


class SaPlan:
    """packed 3-layer grouped MLP (conv+BN(eval)+ReLU x3 + max over K)"""

    def __init__(self, convs, bns, device, mode, fast=True):
        assert len(convs) == 3 and len(bns) == 3, "the fused SA kernel covers 3-layer MLPs"
        self.mode = mode
        self.cin = convs[0].weight.shape[1]
        self.couts = [c.weight.shape[0] for c in convs]
        self.wp = [pack_weight(c.weight, device) for c in convs]
        folded = [fold_bn(b, c.bias, device) for c, b in zip(convs, bns)]
        self.scale = [f[0] for f in folded]
        self.shift = [f[1] for f in folded]
        # decomposed first layer (include/pcr.h, pcr_sa_params): W1 = [Wa | Wc | Wf] (edge) or [Wa | Wf]
        w1 = convs[0].weight.detach().reshape(self.couts[0], -1).double().cpu()
        D = (self.cin - 3) // 2 if mode == 0 else self.cin - 3
        self.D = D
        sc1 = self.scale[0].detach().double().cpu().unsqueeze(1)      # fast path wants scale[0] folded in
        self.wa = _dev32((w1[:, :3] * sc1).float(), device)
        self.wa_packed = pack_weight((w1[:, :3] * sc1).float(), device)    # the same (c1,3) matrix as an MFMA operand
        # [wa | shift]: the cout-split kernel multiplies it with (dx, dy, dz, 1)
        self.wa_shift_packed = pack_weight(torch.cat([w1[:, :3] * sc1, self.shift[0].detach().double().cpu().unsqueeze(1)],
                                                     dim=1).float(), device)
        self.wpq = None
        self.fast = fast
        # layers 2, 3 with the BatchNorm scale folded into the weights and the shift padded to 32
        self.wps, self.shift_pad, self.wps_bf = [], [], []
        for l in (1, 2):
            w = convs[l].weight.detach().reshape(self.couts[l], -1).double().cpu()
            sc = self.scale[l].detach().double().cpu().unsqueeze(1)
            self.wps.append(pack_weight((w * sc).float(), device))
            self.wps_bf.append(pack_weight_bf((w * sc).float(), device))
            pad = torch.zeros((self.couts[l] + 31) // 32 * 32, dtype=torch.float32, device=device)
            pad[:self.couts[l]] = self.shift[l]
            self.shift_pad.append(pad)
        if D > 0:
            if mode == 0:
                wc, wf = w1[:, 3:3 + D], w1[:, 3 + D:3 + 2 * D]
                stacked = torch.cat([wf * sc1, (wc - wf) * sc1], dim=0)
            else:
                stacked = w1[:, 3:3 + D] * sc1
            self.wpq = pack_weight(stacked.float(), device)
            self.wpq_bf = pack_weight_bf(stacked.float(), device)
            if mode == 0:
                # (ABI 17) the coordinate term and the shift as table columns (pcr_dense_pm_xyz_f32): P rows {+wa, 0}, Q rows
                # {-wa, shift}, so that a row of layer 1 is relu(P'[i] + Q'[c]) in the wave-autonomous K-row kernel
                wa64 = w1[:, :3] * sc1
                sh64 = self.shift[0].detach().double().cpu().unsqueeze(1)
                self.wxyz = _dev32(torch.cat([torch.cat([wa64, torch.zeros_like(sh64)], dim=1),
                                              torch.cat([-wa64, sh64], dim=1)], dim=0).float().contiguous(), device)

    def wants_row_table(self, N, K, min_radius, B=1, S=1):
        """does the ragged launch of this layer read the ball query's row table (ops.ball_query_rows)?  Everything the
        library's own dispatch (sa_make_plan / sas_launch_ok) looks at besides the shape is honoured here too -- the
        PCR_SA_NO_STREAM diagnostic and the 32-bit centre count -- so that a caller which drops its index tensor on this
        answer is never refused by the launch."""
        lib = L.load()
        if os.environ.get("PCR_SA_NO_STREAM") or int(B) * int(S) >= 2 ** 31:
            return False
        return bool(self.fast and self.mode == 1 and lib.pcr_ball_query_rows_ok(N, K, min_radius or 0.0) and
                    lib.pcr_sa_uses_row_table(self.couts[0], self.couts[1], self.couts[2], K, PRECISIONS[PRECISION]))

    def run(self, xyz, feat, idx, centre_idx=None, cnt=None, out_point_major=False, rows=None, K=None):
        """rows: the ball query's row table (ops.ball_query_rows, with cnt; idx may then be None and K is given).
        cnt (B,S) int32: genuine-hit counts of a ball query (ops.ball_query_cnt); when given (mode 1) the
        MLP runs only on the distinct rows of every group -- same result, K/cnt times less work.
        feat (B,D,N) may be contiguous or the transposed view of a contiguous (B,N,D) tensor (point-major);
        out_point_major: the result is the (B,c3,S) VIEW of a contiguous (B,S,c3) tensor (a centre's channels
        are written as one run; our own consumers read that layout directly)."""
        B, N, _ = xyz.shape
        if rows is not None:
            S = cnt.shape[1]
            assert cnt is not None and self.wants_row_table(N, K, 0.0, B, S), "row table given to a layer that does not read it"
            L.require_cuda(xyz, cnt, rows)
            assert rows.is_contiguous() and rows.numel() == L.load().pcr_ball_query_rows_floats(B, S, K)
        else:
            L.require_cuda(xyz, idx)
            _, S, K = idx.shape
        D = 0 if feat is None else feat.shape[1]
        want = 3 + (2 * D if self.mode == 0 else D)
        assert want == self.cin, "feature width %d does not match the first conv (%d)" % (want, self.cin)
        feat, feat_pm = as_cm_or_pm(feat)
        assert xyz.is_contiguous() and (idx is None or idx.is_contiguous())
        out = torch.empty((B, S, self.couts[2]) if out_point_major else (B, self.couts[2], S),
                          dtype=torch.float32, device=xyz.device)
        p = SaParams()
        p.mode, p.B, p.N, p.S, p.K, p.D = self.mode, B, N, S, K, D
        p.c1, p.c2, p.c3 = self.couts
        p.xyz, p.feat, p.idx, p.centre_idx = _p(xyz), _p(feat), _p(idx), _p(centre_idx)
        for i in range(3):
            p.wp[i], p.scale[i], p.shift[i] = _p(self.wp[i]), _p(self.scale[i]), _p(self.shift[i])
        p.out = _p(out)
        p.feat_point_major, p.out_point_major = int(feat_pm), int(bool(out_point_major))
        ragged = cnt is not None and self.fast and self.mode == 1
        if cnt is not None:
            assert cnt.is_contiguous() and cnt.dtype == torch.int32 and cnt.shape == (B, S)
        # (shapes whose K-row evaluation runs on the tile plan as well -- the cout-split kernel -- take the workspace too)
        tiled = ragged or (self.fast and self.mode == 1 and L.load().pcr_sa_krow_uses_tiles(
            self.couts[0], self.couts[1], self.couts[2], K, PRECISIONS[PRECISION]))
        if tiled:
            # the persistent tile-list kernel (distinct rows only)
            n_ws = L.load().pcr_sa_tile_ws_ints(B, S, K, self.couts[1], self.couts[2])
            if n_ws > 0:
                tile_ws = torch.empty((n_ws,), dtype=torch.int32, device=xyz.device)
                p.tile_ws = _p(tile_ws)
            if ragged:
                p.cnt = _p(cnt)
                p.row_tab = _p(rows)
        if self.fast:
            p.wa = _p(self.wa)
            p.wa_packed = _p(self.wa_packed)
            p.wa_shift_packed = _p(self.wa_shift_packed)
            p.precision = PRECISIONS[PRECISION]
            # ABI 16: item counters for the wave-autonomous K-row kernel on large clouds (the launch zeroes them itself)
            n_claim = 0 if (ragged or not SA_CLAIMS) else L.load().pcr_sa_claim_ws_ints(
                self.couts[0], self.couts[1], self.couts[2], K, N, PRECISIONS[PRECISION])
            if n_claim > 0:
                claim_ws = torch.empty((n_claim,), dtype=torch.int32, device=xyz.device)
                p.claim_ws = _p(claim_ws)
            for i in range(2):
                p.wps[i], p.shift_pad[i] = _p(self.wps[i]), _p(self.shift_pad[i])
                p.wps_bf[i] = _p(self.wps_bf[i])
            if D:
                c1_, c2_, c3_ = self.couts
                pqw = (2 if self.mode == 0 else 1) * self.couts[0]
                ws = torch.empty((B, N, pqw), dtype=torch.float32, device=xyz.device)
                p.wpq, p.pq_ws = _p(self.wpq), _p(ws)
                # the per-point tables of the decomposed first layer, as its own (profiled) launch
                with _prof("sa_tables[D=%d,out=%d,N=%d]" % (D, pqw, N), 2.0 * B * N * D * pqw,
                           4.0 * B * N * (D + pqw), arith="lib"):
                    if PRECISION == "f32":
                        L.run.pcr_dense_pm_f32(feat, self.wpq, ws, B, D, pqw, N, int(feat_pm), L.stream_ptr())
                    elif (SA_XYZ_TABLES and not ragged and not tiled and idx is not None and
                          L.load().pcr_sa_tables_take_xyz(self.mode, D, c1_, c2_, c3_, K, PRECISIONS[PRECISION])):
                        # the K-row kernel's shapes: tables WITH the coordinate term and the shift (exact f32 fmas on top of
                        # the feature product), and the launch below adds P'[i] + Q'[c] and nothing else in its first layer
                        # (prefix sampling: the centres are the first S points, and only centres' Q rows are ever read)
                        q_rows = min(N, (S + 63) // 64 * 64) if centre_idx is None else N
                        q_rows = q_rows if q_rows % 64 == 0 else N
                        L.run.pcr_dense_pm_xyz_f32(feat, self.wpq_bf, xyz, self.wxyz, ws, B, D, pqw, N, int(feat_pm),
                                                   PRECISIONS[PRECISION], q_rows, c1_ if q_rows < N else pqw,
                                                   L.stream_ptr())
                        p.pq_has_xyz = 1
                    else:   # the tables on the bf16 matrix core too (the layer-1 MFMAs on the coordinates stay f32)
                        L.run.pcr_dense_pm_prec_f32(feat, self.wpq_bf, ws, B, D, pqw, N, int(feat_pm),
                                                    PRECISIONS[PRECISION], L.stream_ptr())
                p.pq_ready = 1
        c1, c2, c3 = self.couts
        flops = 2.0 * B * S * K * (self.cin * c1 + c1 * c2 + c2 * c3)
        nbytes = 4.0 * B * (3 * N + D * N + S * K + c3 * S)
        exec_flops = 2.0 * B * S * K * (c1 * c2 + c2 * c3) if self.fast else flops
        if ragged:   # rows really evaluated: ceil2(max(cnt,1)) per centre (only computed while profiling)
            rows = float(((cnt.clamp(1, K) + 1) // 2 * 2).sum().item()) if PROFILE is not None else 0.0
            exec_flops = 2.0 * rows * (c1 * c2 + c2 * c3)
        name = "sa_ragged" if ragged else "sa_fused"
        with _prof("%s[D=%d,c=%d/%d/%d,N=%d,S=%d,K=%d]" % (name, D, c1, c2, c3, N, S, K), flops, nbytes, exec_flops,
                   arith="lib"):
            L.run.pcr_sa_mlp_f32(ctypes.byref(p), L.stream_ptr())
        return out.transpose(1, 2) if out_point_major else out


def _live_block(live):
    """live = (count, period, offset) -> pcr_live: count a (1,) int32 device tensor (the pair count of a fixed-shape list,
    read by the launch itself), cloud b is live iff b % period < clamp(count - offset, 0, period)"""
    count, period, offset = live
    L.require_cuda(count)
    if count.dtype != torch.int32 or count.numel() < 1 or not count.is_contiguous():
        raise L.PcrError("live: count must be a contiguous int32 device tensor of at least one element")
    if int(period) < 1 or int(offset) < 0:
        raise L.PcrError("live: period must be positive and offset non-negative, got %r, %r" % (period, offset))
    lv = LiveParams()
    lv.count, lv.period, lv.offset = _p(count), int(period), int(offset)
    return lv


class AttnPlan:
    """packed linear-attention block.  `m` exposes pos-MLP (name given), q/k/v/merge projections,
    mlp.{0,2}, norm1/norm2 as in the reference's Self_Attention / FP_SA / corss_attention."""

    def __init__(self, m, pos_name, device, nhead, q_pos, k_pos, residual, final=None):
        pos = getattr(m, pos_name)
        L.require_default_eps(m.norm1, m.norm2)
        self.device = device
        self.nhead, self.q_pos, self.k_pos, self.residual = nhead, int(q_pos), int(k_pos), int(residual)
        self.d = d = m.q_proj.weight.shape[0]
        self.c1 = m.q_proj.weight.shape[1]
        self.c2 = m.k_proj.weight.shape[1]
        self.cout = m.mlp[2].weight.shape[0]
        # fold the second pos-MLP Linear (W2, b2) into the projections, in fp64 (include/pcr.h)
        f64 = lambda x: x.detach().double().cpu()
        W2, b2 = f64(pos[2].weight), f64(pos[2].bias)                 # (c2, d), (c2)
        Wq, Wk, Wv = f64(m.q_proj.weight), f64(m.k_proj.weight), f64(m.v_proj.weight)
        if q_pos:
            wq = torch.cat([Wq, Wq @ W2], dim=1)
            bq = Wq @ b2
        else:
            wq, bq = Wq, torch.zeros(d, dtype=torch.float64)
        kz = (Wk @ W2) if k_pos else torch.zeros(d, d, dtype=torch.float64)
        wkv = torch.cat([torch.cat([Wk, kz], dim=1), torch.cat([Wv, Wv @ W2], dim=1)], dim=0)
        bkv = torch.cat([(Wk @ b2) if k_pos else torch.zeros(d, dtype=torch.float64), Wv @ b2])
        self.t = dict(
            pos0_w=_dev32(pos[0].weight, device), pos0_b=_dev32(pos[0].bias, device),
            wq=pack_weight(wq.float(), device), bq=_dev32(bq.float(), device),
            wkv=pack_weight(wkv.float(), device), bkv=_dev32(bkv.float(), device),
            wmerge=_dev32(m.merge.weight, device),
            wmlp0=pack_weight(m.mlp[0].weight, device), wmlp2=pack_weight(m.mlp[2].weight, device),
            ln1_g=_dev32(m.norm1.weight, device), ln1_b=_dev32(m.norm1.bias, device),
            ln2_g=_dev32(m.norm2.weight, device), ln2_b=_dev32(m.norm2.bias, device))
        if d <= 128:
            if d % 32 == 0 and (d // nhead) % 32 == 0:
                # the tile kv kernel folds the merge projection on the matrix core from this image (heads of whole
                # 32-channel blocks; else its scalar loop)
                self.t["wmerge_packed"] = pack_weight(m.merge.weight, device)
            # the same matrices as bf16 hi / lo images: the dense phases of both kernels in "bf16x3" / "bf16" mode
            if (d == 64 and self.c2 in (64, 128)) or (d == 32 and self.c2 == 32) or d == 128:   # the wave-autonomous kv kernels' shapes; d = 128: the tile kernel's projection
                self.t["wkv_bf"] = pack_weight_bf(wkv.float(), device)
            if d == 64 and self.c1 % 16:        # c1 = 3: mlp[0] with the feature columns padded to a 16-channel step
                w0 = m.mlp[0].weight.detach().float().cpu()
                pad = torch.zeros(w0.shape[0], 16 * ((self.c1 + 15) // 16) - self.c1)
                self.t["wmlp0_bf_xpad"] = pack_weight_bf(torch.cat([w0[:, :self.c1], pad, w0[:, self.c1:]], dim=1), device)
            self.t.update(wq_bf=pack_weight_bf(wq.float(), device),
                          wmlp0_bf=pack_weight_bf(m.mlp[0].weight, device), wmlp2_bf=pack_weight_bf(m.mlp[2].weight, device))
        if d > 128:
            # d_model 256 / 512 (mul = 2 / 4 configs): the kv kernel splits a cloud over d/64 workgroups; band g needs
            # the K rows [64g, 64g+64) and the V rows of its head of the fused projection (include/pcr.h)
            dh = d // nhead
            if d % 64 or dh % 64 or dh > 256:
                raise L.PcrError("attention with d_model %d, %d heads is not covered (heads of 64..256 channels)" % (d, nhead))
            imgs, biases = [], []
            for g in range(d // 64):
                hd = (64 * g) // dh
                rows = torch.cat([torch.arange(64 * g, 64 * g + 64), torch.arange(d + hd * dh, d + (hd + 1) * dh)])
                imgs.append(pack_weight(wkv[rows].float(), device))
                biases.append(bkv[rows].float())
            self.t["wkv_wide"] = torch.cat(imgs).contiguous()
            self.t["bkv_wide"] = _dev32(torch.cat(biases), device)
            self.t["wmerge_packed"] = pack_weight(m.merge.weight, device)
        self.cfinal = 0
        if final is not None:
            self.t["wfinal"] = pack_weight(final.weight, device)
            if d <= 128:
                self.t["wfinal_bf"] = pack_weight_bf(final.weight, device)
            self.cfinal = final.weight.shape[0]
            bpad = torch.zeros((self.cfinal + 31) // 32 * 32, dtype=torch.float32, device=device)
            bpad[:self.cfinal] = final.bias.detach().to(device).float()
            self.t["bfinal"] = bpad

    def _params(self, B, Lq, Sk, feat_q, xyz_q, feat_k, xyz_k, kv, out, kv_index=None, q_index=None):
        p = AttnParams()
        p.B, p.Lq, p.Sk = B, Lq, Sk
        p.c1, p.c2, p.d, p.cout, p.nhead = self.c1, self.c2, self.d, self.cout, self.nhead
        p.q_pos, p.residual = self.q_pos, self.residual
        p.feat_q, p.xyz_q, p.feat_k, p.xyz_k = _p(feat_q), _p(xyz_q), _p(feat_k), _p(xyz_k)
        p.kv_index, p.q_index = _p(kv_index), _p(q_index)
        for k, v in self.t.items():
            setattr(p, k, _p(v))
        p.cfinal = self.cfinal
        p.kv, p.out = _p(kv), _p(out)
        p.precision = PRECISIONS[PRECISION]
        return p

    def live_ok(self):
        """can kv(.., live=) / apply(.., live=) be honoured for this block (pcr_attn_live_ok: the shape decides, never the
        batch)?"""
        dummy = torch.empty(0)
        p = self._params(1, 32, 32, dummy, None, dummy, None, dummy, dummy)
        p.feat_q = p.feat_k = p.xyz_q = p.xyz_k = p.kv = p.out = 1        # (only tested against NULL)
        return bool(L.load().pcr_attn_live_ok(ctypes.byref(p)))

    def kv(self, feat_k, xyz_k, live=None, out=None):
        """key-side state of every cloud: (B, d*d + d) per-cloud images (reusable across many queries).
        live = (count, period, offset) (pcr_live; only where live_ok says so): dead clouds are neither read nor written --
        their rows of the result hold whatever the buffer held.  out: the (B, d*d + d) buffer to write into."""
        L.require_cuda(feat_k, xyz_k)
        assert feat_k.is_contiguous() and xyz_k.is_contiguous() and feat_k.dtype == torch.float32
        B, c2, Sk = feat_k.shape
        assert c2 == self.c2
        lib = L.load()
        if out is not None:
            L.require_cuda(out)
            assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, lib.pcr_attn_kv_floats(self.d))
        kv = out if out is not None else torch.empty((B, lib.pcr_attn_kv_floats(self.d)), dtype=torch.float32,
                                                     device=feat_k.device)
        p = self._params(B, 1, Sk, feat_k, xyz_k, feat_k, xyz_k, kv, kv)
        d = self.d
        # token split (the library's suggestion for this launch shape): partial matrices + a fold launch
        ns = lib.pcr_attn_kv_splits(B, Sk, d) if KV_SPLITS is None else KV_SPLITS
        if live is not None and ns > 1:
            raise L.PcrError("a gated kv launch takes whole clouds (kv_splits = %d)" % ns)
        if ns > 1:
            part = torch.empty((B, ns, lib.pcr_attn_kv_floats(d)), dtype=torch.float32, device=feat_k.device)
            p.kv_splits, p.kv_part = ns, _p(part)
        kv_flops = 2.0 * B * Sk * (3 * d + d * c2 + 2 * c2 * d + d * d / self.nhead)   # reference's op count
        with _prof("attn_kv[d=%d,c2=%d,Sk=%d]" % (d, c2, Sk), kv_flops, 4.0 * B * (c2 * Sk + 3 * Sk + d * d + d),
                   arith="lib"):
            if live is not None:
                L.run.pcr_attn_kv_live_f32(ctypes.byref(p), ctypes.byref(_live_block(live)), L.stream_ptr())
            else:
                L.run.pcr_attn_kv_f32(ctypes.byref(p), L.stream_ptr())
        kv._pcr_precision = PRECISION      # the per-cloud matrix is an image of this kind: apply() must match
        return kv

    def pool_ok(self, Lq, Sk):
        """can apply(.., pooled=True) be honoured for this block in the current arithmetic (pcr_attn_apply_pool_ok: the
        launch shape and the mode decide, never the batch)?"""
        dummy = torch.empty(0)
        p = self._params(1, Lq, Sk, dummy, None, dummy, None, dummy, dummy)
        p.feat_q = p.feat_k = p.xyz_k = p.kv = p.out = 1        # (only tested against NULL)
        return bool(L.load().pcr_attn_apply_pool_ok(ctypes.byref(p)))

    def apply(self, feat_q, xyz_q, kv, Sk, kv_index=None, q_index=None, n_out=None, pooled=False, live=None, out=None):
        """query side: n_out virtual clouds (default: one per query cloud); virtual cloud b takes its tokens
        from cloud q_index[b] (default b) and the key-side state kv[kv_index[b]] (default b).
        pooled (ABI 16; only where pool_ok says so): the block output is not written -- returns (B, 2, cout) = every
        virtual cloud's per-channel [maximum | sum] over its Lq tokens.
        live = (count, period, offset) (pcr_live; only where live_ok says so): dead virtual clouds are neither read (their
        q_index / kv_index entries included) nor written; a pooled result then starts as zeros, because what follows reads
        it in full, an un-pooled one holds whatever its buffer held.  out: the buffer to write into."""
        L.require_cuda(feat_q, kv)
        assert feat_q.is_contiguous() and feat_q.dtype == torch.float32 and (xyz_q is None or xyz_q.is_contiguous())
        Bq, c1, Lq = feat_q.shape
        assert c1 == self.c1
        made = getattr(kv, "_pcr_precision", PRECISION)
        if (made == "f32") != (PRECISION == "f32") and self.d <= 128:
            raise L.PcrError("attention state was built in %r mode and is applied in %r mode: the per-cloud matrix is "
                             "stored in the arithmetic's own layout" % (made, PRECISION))
        B = n_out if n_out is not None else Bq
        shape = (B, 2, self.cout) if pooled else (B, self.cfinal or self.cout, Lq)
        if out is not None:
            L.require_cuda(out)
            assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == shape
        if pooled:
            if out is None:
                out = (torch.zeros if live is not None else torch.empty)(shape, dtype=torch.float32, device=feat_q.device)
            p = self._params(B, Lq, Sk, feat_q, xyz_q, feat_q, xyz_q if xyz_q is not None else feat_q, kv, None,
                             kv_index, q_index)
            p.pool_out = _p(out)
        else:
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=feat_q.device)
            p = self._params(B, Lq, Sk, feat_q, xyz_q, feat_q, xyz_q if xyz_q is not None else feat_q, kv, out,
                             kv_index, q_index)
        d = self.d
        ap_flops = 2.0 * B * Lq * (c1 * d + d * d / self.nhead + d * d + (c1 + d) * 2 * d + 2 * d * self.cout
                                   + self.cout * self.cfinal + (self.q_pos * (3 * d + d * c1)))
        with _prof("attn_apply[d=%d,c1=%d,out=%d,Lq=%d%s]" % (d, c1, self.cfinal or self.cout, Lq, ",pooled" if pooled else ""),
                   ap_flops, 4.0 * B * (c1 * Lq + d * d + d + (2 if pooled else Lq) * (self.cfinal or self.cout)), arith="lib"):
            if live is not None:
                L.run.pcr_attn_apply_live_f32(ctypes.byref(p), ctypes.byref(_live_block(live)), L.stream_ptr())
            else:
                L.run.pcr_attn_apply_f32(ctypes.byref(p), L.stream_ptr())
        return out

    def run(self, feat_q, xyz_q, feat_k, xyz_k, kv_index=None):
        """feat_q (B,c1,Lq), feat_k (B,c2,Sk), xyz (B,L,3) -> (B, cfinal or cout, Lq)"""
        assert feat_k.shape[0] == feat_q.shape[0]
        kv = self.kv(feat_k, xyz_k)
        return self.apply(feat_q, xyz_q, kv, feat_k.shape[2], kv_index=kv_index)


class HeadPlan:
    """pool 'both' over point-concatenated pairs + LinearRes(GN) + Linear(.,1)"""

    def __init__(self, linres, out_linear, device):
        if getattr(linres, "transform", None) is not None:
            raise L.PcrError("pcr_pool_head_f32 covers LinearRes with n_in == n_out only")
        L.require_default_eps(linres.norm1, linres.norm2)
        self.n = linres.linear1.weight.shape[0]
        self.groups = linres.norm1.num_groups
        self.t = dict(w1=_dev32(linres.linear1.weight, device), w2=_dev32(linres.linear2.weight, device),
                      gn1_g=_dev32(linres.norm1.weight, device), gn1_b=_dev32(linres.norm1.bias, device),
                      gn2_g=_dev32(linres.norm2.weight, device), gn2_b=_dev32(linres.norm2.bias, device),
                      w_out=_dev32(out_linear.weight, device), b_out=_dev32(out_linear.bias, device),
                      w1t=_dev32(linres.linear1.weight.detach().t().contiguous(), device),
                      w2t=_dev32(linres.linear2.weight.detach().t().contiguous(), device))

    def run(self, o, want_pooled=False, live=None, dead_value=0.0):
        """o (2P, C, L): clouds p and p+P are pair p -> logits (P) [, pooled (P,2C)]
        live = (count, period, offset) (pcr_live, pairs in place of clouds): the clouds of a dead pair are not read, its logit
        is dead_value and its pooled row zeros"""
        L.require_cuda(o)
        assert o.is_contiguous() and o.dtype == torch.float32
        twoP, C, Lp = o.shape
        P = twoP // 2
        assert 2 * C == self.n, "pooled width %d != match head width %d" % (2 * C, self.n)
        logits = torch.empty((P,), dtype=torch.float32, device=o.device)
        pooled = torch.empty((P, 2 * C), dtype=torch.float32, device=o.device) if want_pooled else None
        p = HeadParams()
        p.P, p.C, p.L, p.groups = P, C, Lp, self.groups
        p.o = _p(o)
        for k, v in self.t.items():
            setattr(p, k, _p(v))
        p.pooled, p.logits = _p(pooled), _p(logits)
        with _prof("pool_head", 4.0 * P * (2 * C) ** 2, 4.0 * twoP * C * Lp):
            if live is not None:
                L.run.pcr_pool_head_live_f32(ctypes.byref(p), ctypes.byref(_live_block(live)),
                                             ctypes.byref(ctypes.c_float(dead_value)), L.stream_ptr())
            else:
                L.run.pcr_pool_head_f32(ctypes.byref(p), L.stream_ptr())
        return (logits, pooled) if want_pooled else logits


def as_cm_or_pm(x):
    """(tensor the kernels can read, is_point_major) for a (B,C,L) feature tensor: contiguous = channel-major;
    the transposed view of a contiguous (B,L,C) tensor = point-major, passed through as it is; anything else is
    made contiguous."""
    if x is None or x.is_contiguous():
        return x, False
    if x.dim() == 3 and x.transpose(1, 2).is_contiguous():
        return x, True
    return x.contiguous(), False


def dense(x, wp, cout, scale=None, shift=None, act=0):
    """x (B,cin,L) (channel-major, or the transposed view of a point-major tensor) -> (B,cout,L) through
    pcr_dense_f32 / pcr_dense_xpm_f32 (wp packed)."""
    L.require_cuda(x)
    assert x.dtype == torch.float32
    x, x_pm = as_cm_or_pm(x)
    B, cin, Ln = x.shape
    y = torch.empty((B, cout, Ln), dtype=torch.float32, device=x.device)
    lib = L.load()
    bf = getattr(wp, "_pcr_bf", None)
    if PRECISION != "f32" and bf is not None and not x_pm and lib.pcr_dense_prec_ok(cin, cout, Ln):
        # the wide per-point layers (PointNet convs, DGCNN conv5, LinearRes rows) on the bf16 matrix core
        with _prof("dense[cin=%d,cout=%d,L=%d]" % (cin, cout, Ln), 2.0 * B * Ln * cin * cout, 4.0 * B * Ln * (cin + cout),
                   arith="lib"):
            L.run.pcr_dense_prec_f32(x, bf, scale, shift, y, B, cin, cout, Ln, act, PRECISIONS[PRECISION],
                                     L.stream_ptr())
        return y
    if PRECISION != "f32" and bf is not None and x_pm and lib.pcr_dense_xpm_prec_ok(cin, cout, Ln):
        # a point-major tensor (the last SA layer's output) straight into the bf16 matrix core: a token's row is the operand
        with _prof("dense[cin=%d,cout=%d,L=%d]" % (cin, cout, Ln), 2.0 * B * Ln * cin * cout, 4.0 * B * Ln * (cin + cout),
                   arith="lib"):
            L.run.pcr_dense_xpm_prec_f32(x, bf, scale, shift, y, B, cin, cout, Ln, act, PRECISIONS[PRECISION],
                                         L.stream_ptr())
        return y
    fn = L.run.pcr_dense_xpm_f32 if x_pm else L.run.pcr_dense_f32
    with _prof("dense[cin=%d,cout=%d,L=%d]" % (cin, cout, Ln), 2.0 * B * Ln * cin * cout, 4.0 * B * Ln * (cin + cout),
               arith="lib"):
        fn(x, wp, scale, shift, y, B, cin, cout, Ln, act, L.stream_ptr())
    return y
