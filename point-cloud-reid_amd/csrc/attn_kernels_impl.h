// Linear-attention kernels (pcr_attn_kv_f32 / pcr_attn_apply_f32).  Body of two translation units:
//   attn_kernels.hip      PCR_ATTN_PREC 0  f32-input MFMA, every shape, and the C-ABI entry points
//   attn_kernels_bf3.hip  PCR_ATTN_PREC 1  the dense phases of the apply kernel (Q, message, feed-forward, cov_final) as
//                                          split bf16 on v_mfma_f32_32x32x16_bf16 for d_model <= 128; the kv kernel
//                                          writes the per-cloud matrix as a bf16 image; exports pcr_attn_{kv,apply}_bf3
#pragma once
#ifndef PCR_ATTN_PREC
#define PCR_ATTN_PREC 0
#endif
#include "tile_dense.h"
#include "wave_trace.h"

#include <stdio.h>

#include <initializer_list>
#include <type_traits>
#include <vector>

namespace {
constexpr int kAPrec = PCR_ATTN_PREC;
// -------------------------------------------------------------- linear attention ----
struct AttnArgs {
  pcr_attn_params p;
  int dbg;   // diagnostics (tuning builds): 256 = stamp the shader clock; 512 = attn_kv_stream64_kernel multiplies an all-zero
             // key-position block too (PCR_ATTN_KV_FULL)
  int wpc;   // attn_kv_stream128_kernel: waves per cloud (1, 2, 4), a function of Sk only
  // gated launches only (pcr_live, the GATE instantiations below); the un-gated kernels never read these
  const int *live_count;
  int live_period, live_offset;
};

// ---- gated launches (pcr_live): which virtual clouds of a launch are live ------------------------------------------------
// n = clamp(*count - offset, 0, period) pairs of every period are live: cloud b iff b % period < n.  The count is ONE load
// per workgroup from a kernel-argument address, broadcast through readfirstlane, so every branch on it is wave-uniform.
// The persistent kernels walk the compact index v in [0, total) of the live clouds only and map it back:
// b = (v / n) period + v % n -- for the matching stages' two runs [0, n) and [period, period + n) that is
// v < n ? v : v - n + period.  Dead clouds are never indexed: neither their q_index / kv_index entries nor their features are
// read, nothing of theirs is written.
struct LiveWalk {
  unsigned n, period;
  long total;   // live clouds of the launch
  __device__ __forceinline__ long map(long v) const {
    const unsigned q = (unsigned)v / n;
    return (long)q * period + ((unsigned)v - q * n);
  }
};
__device__ __forceinline__ unsigned live_pairs(const AttnArgs &a) {
  int c = __builtin_amdgcn_readfirstlane(*a.live_count);
  c = c < 0 ? 0 : c;
  c -= a.live_offset;
  return (unsigned)(c < 0 ? 0 : (c > a.live_period ? a.live_period : c));
}
__device__ __forceinline__ LiveWalk live_walk(const AttnArgs &a) {
  LiveWalk w;
  w.n = live_pairs(a);
  w.period = (unsigned)a.live_period;
  const unsigned B = (unsigned)a.p.B, full = B / w.period, rem = B - full * w.period;
  w.total = (long)full * w.n + (rem < w.n ? rem : w.n);
  return w;
}
// the tile kernels (one workgroup per cloud): is cloud b live?  Workgroup-uniform, asked before any barrier.
__device__ __forceinline__ bool live_cloud(const AttnArgs &a, unsigned b) {
  return b % (unsigned)a.live_period < live_pairs(a);
}

// shader-clock stamps of the wave-autonomous kv kernel (trace builds only: -DPCR_SA_TRACE_BUILD, PCR_ATTN_TRACE=<file>);
// one record of kATraceMarks stamps per cloud round of waves 0 and 5 of the first workgroups
constexpr int kATraceWgs = 512, kATraceRecs = 24, kATraceMarks = 8;
using AttnTrace = WaveTrace<0, kATraceRecs, kATraceMarks, 2 * kATraceWgs>;
__device__ unsigned long long g_attn_trace[AttnTrace::kCap * AttnTrace::kWords];

// Algebra used by both kernels (the host folds it into the weights, see AttnPlan in
// pcr_amd/engine.py): with h = relu(W0 xyz + b0) the position encoding is W2 h + b2, so
//   Wq (x + W2 h + b2) = [Wq | Wq W2] [x ; h] + Wq b2        (one dense instead of three)
//   [K ; V] pre-activation = [[Wk | kpos Wk W2] ; [Wv | Wv W2]] [x ; h] + [kpos Wk b2 ; Wv b2]
// and the merge projection is folded into the per-cloud KV matrix by the kv kernel:
//   merge(msg)[o] = sum_dd M[o][dd] Q'[dd],  M[o][dd] = sum_{v in head(dd)} Wm[o][v] KV[dd][v],
//   Q'[dd] = Q[dd] * Sk / (Q_head . ksum_head + 1e-6).

// hidden = relu(W0 xyz + b0) for the T tokens of a tile -> dst rows [0,d) ([d][RP]); zero xyz beyond L
__device__ __forceinline__ void pos_hidden(float *dst, int RP, const float *P, const float *w0,
                                           const float *b0, int d, int T) {
  for (int e = threadIdx.x; e < d * T; e += blockDim.x) {
    const int o = e / T, t = e - o * T;
    const float v = w0[o * 3] * P[t] + w0[o * 3 + 1] * P[RP + t] + w0[o * 3 + 2] * P[2 * RP + t] + b0[o];
    dst[o * RP + t] = fmaxf(v, 0.f);
  }
}

__device__ __forceinline__ void load_xyz3(float *P, int RP, const float *xyz, int L, int t0, int T) {
  for (int e = threadIdx.x; e < 3 * T; e += blockDim.x) {
    const int c = e / T, t = e - c * T;
    P[c * RP + t] = t0 + t < L ? xyz[(size_t)(t0 + t) * 3 + c] : 0.f;
  }
}

// merge fold of one cloud from its head-masked KV in LDS (KVl [dd][d + 1]) and total key sums (s_kt [d]):
// M[o][dd] = sum_{v in head(dd)} Wm[o][v] KV[dd][v], written as the packed A-operand image (f32 or bf16 hi / lo), then ksum
__device__ __forceinline__ void attn_kv_fold_write(const pcr_attn_params &p, const float *KVl, const float *s_kt, size_t b) {
  const int d = p.d, dh = d / p.nhead, ld = d + 1, tid = threadIdx.x;
  float *kv = p.kv + b * ((size_t)d * d + d);
  // e = (o = e / d, dd = e % d) advances by kThreads: one division per thread, then increments; the head of dd is
  // re-derived only when dd changes (never for d = 32 / 64 / 128, where kThreads % d == 0)
  const int d_o = kThreads / d, d_dd = kThreads - d_o * d;
  int o = tid / d, dd = tid - o * d;
  int v0 = (dd / dh) * dh;
  for (int e = tid; e < d * d; e += kThreads, o += d_o, dd += d_dd) {
    if (dd >= d) {
      dd -= d;
      o++;
    }
    if (d_dd) v0 = (dd / dh) * dh;
    const float *wm = p.wmerge + (size_t)o * d + v0;
    const float *kr = KVl + dd * ld + v0;
    float m = 0.f;
#pragma unroll 8
    for (int v = 0; v < dh; v++) m += wm[v] * kr[v];   // (unrolled: batches of independent loads)
    if constexpr (kAPrec == 0) {
      const int kb = dd >> 3, rem = dd & 7;
      kv[(((size_t)kb * d + o) * 2 + (rem & 1)) * 4 + (rem >> 1)] = m;
    } else {
      // the bf16 A-operand image of M (cout o, cin dd; tile_dense.h: accumulator-order K inside a 16-channel step)
      const int s16 = dd >> 4, kk = dd & 15;
      const int hh = (kk >> 2) & 1, jj = (kk & 3) + ((kk >> 3) << 2);
      const size_t unit = (((size_t)s16 * (d >> 5) + (o >> 5)) * 2) * 64 + hh * 32 + (o & 31);
      const __bf16 hi = (__bf16)m;
      const __bf16 lo = (__bf16)(m - (float)hi);
      __bf16 *img = reinterpret_cast<__bf16 *>(kv);
      img[unit * 8 + jj] = hi;
      img[(unit + 64) * 8 + jj] = lo;
    }
  }
  __syncthreads();
  if (tid < d) kv[(size_t)d * d + tid] = s_kt[tid];
}

// The same fold on the matrix core (round 5): per head, M[:, head] = Wm[:, head] KV_head^T is a dense call over k = v with
// the head's k-blocks of the packed merge weights (p.wmerge_packed) as the A operand and the TRANSPOSED KV tile in LDS as
// the B operand (KVt [v][ld], token = dd).  The scalar loop above costs every thread d d / 256 dot products of dh terms
// whose weights it fetches from global memory one float at a time -- 40-100 us per cloud at d = 128, the larger part of
// the tile kernel's launch (pt128: one 32-token tile per cloud and 0.27 ms; pt1024: a third of 0.72 ms) -- against ~4 us of
// MFMAs.  Heads of whole 32-channel blocks only (the caller falls back otherwise); the k-steps run in the loop's order.
__device__ __forceinline__ void attn_kv_fold_mfma(const pcr_attn_params &p, const float *KVt, const float *s_kt, size_t b) {
  const int d = p.d, dh = d / p.nhead, ld = d + 1, tid = threadIdx.x;
  float *kv = p.kv + b * ((size_t)d * d + d);
  for (int hd = 0; hd < p.nhead; hd++) {
    const float *wm = p.wmerge_packed + (size_t)(hd * dh / 8) * d * 8;
    tile_dense(KVt + (size_t)(hd * dh) * ld + hd * dh, dh, ld, dh >> 5, wm, d, [&](float m, int o, int t) {
      const int dd = hd * dh + t;
      if constexpr (kAPrec == 0) {
        const int kb = dd >> 3, rem = dd & 7;
        kv[(((size_t)kb * d + o) * 2 + (rem & 1)) * 4 + (rem >> 1)] = m;
      } else {
        const int s16 = dd >> 4, kk = dd & 15;
        const int hh = (kk >> 2) & 1, jj = (kk & 3) + ((kk >> 3) << 2);
        const size_t unit = (((size_t)s16 * (d >> 5) + (o >> 5)) * 2) * 64 + hh * 32 + (o & 31);
        const __bf16 hi = (__bf16)m;
        const __bf16 lo = (__bf16)(m - (float)hi);
        __bf16 *img = reinterpret_cast<__bf16 *>(kv);
        img[unit * 8 + jj] = hi;
        img[(unit + 64) * 8 + jj] = lo;
      }
    });
  }
  __syncthreads();
  if (tid < d) kv[(size_t)d * d + tid] = s_kt[tid];
}

// One workgroup per key-side cloud, token tiles of T = 32*TB (TB = 2 for d <= 64, 1 for d = 128).
// kv image per cloud: packed (d x d) matrix M (merge folded in, see above) followed by ksum[d].
// LDS: XH [c2 + d] key features ; hidden -- the fused K/V projection (2d <= c2 + d rows) is written IN PLACE over
// it (barrier between k-loop and epilogue) -- and P [3]; after the loop KVl [d][d+1].  34 KB at d = c2 = 64, so four
// workgroups share a CU; the next tile's features are fetched into registers while this tile is on the matrix core.
//   WSEL: dense shape of the 2d-row projection (2 / 1 / 1 for d = 32 / 64 / 128), NTW: KV tiles per wave (1 / 1 / 4)
// BFP (bf unit only): the K / V projection as split bf16 on the wkv_bf image (the caller checks it is there)
template <int TB, int NR, int WSEL, int NTW, bool BFP = false>
__device__ __forceinline__ void attn_kv_body(const AttnArgs &a) {
  constexpr int T = 32 * TB, RP = T + 1;
  constexpr int NPF = 4;   // 16-byte feature pieces per thread and tile held in registers (c2 * T / 4 / 256 <= NPF)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  const int d = p.d, c2 = p.c2;
  float *XH = smem;
  float *KB = XH;             // rows [0,d) after the projection
  float *VB = XH + d * RP;    // rows [d,2d)
  float *P = XH + (c2 + d) * RP;
  float *s_w0 = P + 3 * RP, *s_b0 = s_w0 + 3 * d;   // staged pos-MLP first layer
  // [256] partial key sums, beyond both the loop's buffers and the KVl / total-sum overlay used after it
  const int tail_a = (c2 + d + 3) * RP + 4 * d, tail_b = d * (d + 1) + d;
  float *s_ks = smem + (tail_a > tail_b ? tail_a : tail_b);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const size_t b = blockIdx.x;
  for (int e = tid; e < 3 * d; e += kThreads) s_w0[e] = p.pos0_w[e];
  for (int e = tid; e < d; e += kThreads) s_b0[e] = p.pos0_b[e];
  const float *feat = p.feat_k + b * c2 * p.Sk;
  const float *xyz = p.xyz_k + b * p.Sk * 3;
  const int nb = d >> 5, nT = nb * nb;
  const int dh = d / p.nhead;
  const float sk = (float)p.Sk;
  const float *bkv = p.bkv;

  f32x16 acc[NTW];
#pragma unroll
  for (int i = 0; i < NTW; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
  int tile_ib[NTW];   // KV tile (ib, jb) of this wave's it-th item: the division is done once, not per token tile
#pragma unroll
  for (int it = 0; it < NTW; it++) tile_ib[it] = (wave + 4 * it) / nb;
  // key sums: thread (row = tid % d, part = tid / d) adds up its share of the tokens of every tile
  const int krow = tid % d, kpart = tid / d, kparts = kThreads / d;
  float ksum = 0.f;

  // feature tile prefetch (whole, aligned tiles: one 16-byte piece per (row, 4 tokens); others go the plain way)
  const int Q = T >> 2, npieces = c2 * Q;
#ifndef PCR_KV_PREFETCH
#define PCR_KV_PREFETCH 1
#endif
  const bool vec_ok = PCR_KV_PREFETCH && ((p.Sk & 3) == 0) && ((reinterpret_cast<size_t>(feat) & 15) == 0) && npieces <= NPF * kThreads;
  f32x4 pf[NPF];
  auto fetch = [&](int t0) {
#pragma unroll
    for (int u = 0; u < NPF; u++) {
      const int e = tid + u * kThreads;
      const int c = e / Q, q = e - c * Q;
      const bool ok = e < npieces;
      pf[u] = *reinterpret_cast<const f32x4 *>(feat + (size_t)(ok ? c : 0) * p.Sk + t0 + 4 * (ok ? q : 0));
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < NPF; u++) {
      const int e = tid + u * kThreads;
      if (e < npieces) {
        const int c = e / Q, q = e - c * Q;
        float *dst = XH + c * RP + 4 * q;
        dst[0] = pf[u][0];
        dst[1] = pf[u][1];
        dst[2] = pf[u][2];
        dst[3] = pf[u][3];
      }
    }
  };
  // token split (kv_splits > 1): workgroup (b, y) takes the tiles [y * tps, (y + 1) * tps) of its cloud and leaves its
  // raw partial KV / key sums in kv_part; attn_kv_fold_kernel adds the partials in order and folds the merge projection
  const int nsplit = p.kv_splits > 1 ? p.kv_splits : 1;
  const int ntile = (p.Sk + T - 1) / T, tps = (ntile + nsplit - 1) / nsplit;
  const int t_lo = (int)blockIdx.y * tps * T;
  const int t_hi = (t_lo + tps * T) < p.Sk ? (t_lo + tps * T) : p.Sk;
  bool have = false;   // the registers hold the tile about to be processed
  if (vec_ok && t_lo + T <= p.Sk && t_lo < t_hi) {
    fetch(t_lo);
    have = true;
  }
  for (int t0 = t_lo; t0 < t_hi; t0 += T) {
    const int valid = p.Sk - t0;
    if (have) stash();
    else load_tile(XH, RP, feat, c2, c2, p.Sk, t0, T);
    load_xyz3(P, RP, xyz, p.Sk, t0, T);
    __syncthreads();
    // the next tile is whole: it is requested AFTER the projection's k-loop (the dense call's hook) and stored at the top of
    // the next round.  (Requested here, before the projection, it was older than the first refill of the projection's
    // weight ring -- a wave's vector loads retire in order, so the ring's first wait sat out the whole HBM round trip
    // and the prefetch overlapped nothing; behind the k-loop it has the epilogue and the KV MFMAs to land.  Explicit wave /
    // tile splits only: the generic split runs the hook before its k-loop, i.e. as before.)
    have = vec_ok && t0 + 2 * T <= p.Sk && t0 + T < t_hi;
    pos_hidden(XH + c2 * RP, RP, P, s_w0, s_b0, d, T);
    __syncthreads();
    // (whole-tile epilogue: a 32-cout block is all K or all V, so the branch is wave-uniform)
    // (f32-input MFMA in both units: this kernel is one workgroup per cloud walking its token tiles serially -- latency,
    // not the matrix pipe, bounds it, and the bf16 form's operand conversion measured 0-15 % SLOWER here)
    auto kv_epi = [&](const f32x16 &acc, int cb, int tb, int l31, int h) {
      const int t = tb * 32 + l31;
      float *dst = XH + (cb * 32 + 4 * h) * RP + t;
      const bool live = t < valid;
      if (cb * 32 < d) {
#pragma unroll
        for (int r = 0; r < 16; r++) dst[((r & 3) + 8 * (r >> 2)) * RP] = live ? elu1(acc[r]) : 0.f;
      } else {
#pragma unroll
        for (int r = 0; r < 16; r++) dst[((r & 3) + 8 * (r >> 2)) * RP] = live ? acc[r] / sk : 0.f;
      }
    };
    auto kv_hook = [&]() { if (have) fetch(t0 + T); };
    // (biases seed the accumulators.  Round 5: with the fold on the matrix core and the prefetch behind the k-loop the
    // projection's 256 f32 MFMAs of 64 cycles per wave and tile ARE the tile's time for long key sets, so the bf unit runs
    // them as split bf16 like the streaming kernels do -- explicit wave / tile splits, wkv_bf given)
    if constexpr (BFP && kAPrec != 0 && WSEL != 0)
      tile_dense2p<kAPrec, TB, NR, WSEL, true>(XH, c2 + d, p.wkv_bf, 2 * d, true, kv_epi, bkv, nullptr, kv_hook);
    else
      tile_dense2<TB, NR, WSEL, true>(XH, c2 + d, p.wkv, 2 * d, true, kv_epi, bkv, nullptr, kv_hook);
    __syncthreads();
    {
      const float *row = KB + krow * RP;
      for (int t = kpart; t < T; t += kparts) ksum += row[t];
    }
#pragma unroll
    for (int it = 0; it < NTW; it++) {
      const int item = wave + 4 * it;
      if (item < nT) {
        const int ib = tile_ib[it], jb = item - ib * nb;
        const float *ap = KB + (ib * 32 + l31) * RP + h;
        const float *bp = VB + (jb * 32 + l31) * RP + h;
#pragma unroll 4
        for (int ks = 0; ks < T / 2; ks++)
          acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * ks], bp[2 * ks], acc[it], 0, 0, 0);
      }
    }
    __syncthreads();   // K / V live in XH: the next tile may only be written once every wave is done with them
  }
  if (nsplit > 1) {   // raw partials: [d][d] KV (row dd, column v), then d key sums
    float *part = p.kv_part + ((size_t)b * nsplit + blockIdx.y) * ((size_t)d * d + d);
    s_ks[tid] = ksum;
#pragma unroll
    for (int it = 0; it < NTW; it++) {
      const int item = wave + 4 * it;
      if (item < nT) {
        const int ib = tile_ib[it], jb = item - ib * nb;
#pragma unroll
        for (int r = 0; r < 16; r++)
          part[(size_t)(ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * d + jb * 32 + l31] = acc[it][r];
      }
    }
    __syncthreads();
    if (tid < d) {
      float s = 0.f;
      for (int pp = 0; pp < kparts; pp++) s += s_ks[pp * d + tid];
      part[(size_t)d * d + tid] = s;
    }
    return;
  }
  // KV (head-masked) -> LDS [dd][d+1], then fold the merge projection and write the packed image
  float *KVl = smem;
  const int ld = d + 1;
  const bool mfma_fold = p.wmerge_packed != nullptr && (dh & 31) == 0 && (d & 31) == 0;
  float *s_kt = smem + d * ld;   // [d] total key sums
  s_ks[tid] = ksum;
#pragma unroll
  for (int it = 0; it < NTW; it++) {
    const int item = wave + 4 * it;
    if (item < nT) {
      const int ib = tile_ib[it], jb = item - ib * nb;
      const int v = jb * 32 + l31;
      const int hv = v / dh;
      const bool aligned = (dh & 31) == 0;           // heads made of whole 32-blocks: one test per tile
      const bool same_blk = (ib * 32) / dh == hv;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int dd = ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool same = aligned ? same_blk : (dd / dh == hv);
        if (mfma_fold) KVl[v * ld + dd] = same ? acc[it][r] : 0.f;     // (transposed: the fold's B operand)
        else KVl[dd * ld + v] = same ? acc[it][r] : 0.f;
      }
    }
  }
  __syncthreads();
  if (tid < d) {
    float s = 0.f;
    for (int pp = 0; pp < kparts; pp++) s += s_ks[pp * d + tid];
    s_kt[tid] = s;
  }
  if (mfma_fold) attn_kv_fold_mfma(p, KVl, s_kt, b);
  else attn_kv_fold_write(p, KVl, s_kt, b);
}

template <int TB, int NR, int WSEL, int NTW>
__global__ __launch_bounds__(kThreads) void attn_kv_kernel(AttnArgs a) {
  attn_kv_body<TB, NR, WSEL, NTW>(a);
}
// the same body held to a third of the register file (three workgroups per CU): worth 5-15 % for d = 64 / 128 even
// where it costs a few spilled registers, not for d = 32 (already three per CU on its own)
template <int TB, int NR, int WSEL, int NTW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_kv_kernel_o3(AttnArgs a) {
  attn_kv_body<TB, NR, WSEL, NTW>(a);
}
// ... gated (pcr_live): the workgroup of a dead cloud leaves at entry
template <int TB, int NR, int WSEL, int NTW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_kv_kernel_o3_live(AttnArgs a) {
  if (!live_cloud(a, blockIdx.x)) return;
  attn_kv_body<TB, NR, WSEL, NTW>(a);
}
// ... and to half of it: the d = 128 shape, whose LDS allows two workgroups per CU and no more
template <int TB, int NR, int WSEL, int NTW, bool BFP = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_kv_kernel_o2(AttnArgs a) {
  attn_kv_body<TB, NR, WSEL, NTW, BFP>(a);
}

// ---- wave-autonomous form for d = c2 = 64 (the shape of six of pt1024's eight kv launches, of every gallery / SSG kv
// launch): a WAVE owns a 32-token block end to end, no workgroup barrier inside a cloud's token loop.
//   * lane (t = lane % 32, h = lane / 32) loads / computes the channels k = 2 s + h of token t: feature channels
//     (s < 32, coalesced 128-byte rows of the channel-major input) and the position-MLP hidden channels (s >= 32);
//     register s IS the A operand of k-step s of the TRANSPOSED projection  Y^T[token][cout] = [x ; h]^T W^T;
//   * the B operand W^T comes from an LDS copy of the packed weight image, one ds_read_b128 per (cout block, four k-steps);
//   * the accumulators of the transposed projection hold, in lane (cout c, h), the tokens 8 g + 4 h + q of output channel c
//     -- which is exactly an MFMA operand of KV[dd][v] += sum_t K[dd][t] V[v][t] with the contraction index (step r,
//     half h) <-> token 8 (r / 4) + 4 h + r % 4, the same assignment for the K and the V operand: after elu + 1 / the
//     1 / Sk scale, accumulator register r of a K block and of a V block go straight into the 64 KV MFMAs.  No LDS
//     round trip, no transposition, no barrier between the 256 projection MFMAs and the 64 KV MFMAs of a block;
//   * eight waves (two per SIMD: one's loads / hidden layer / epilogue under the other's MFMAs) share one 64 KB weight
//     image; a workgroup is persistent over clouds and takes CPG = 8 / min(4, Sk / 32) clouds at a time (round 6; before:
//     min(8, Sk / 32) waves per cloud), so key sets of any length occupy every wave; the waves of a cloud add their KV in
//     wave order (fixed).
// Same per-cloud result whatever the batch (shape-only dispatch); rounding differs from the tile kernel's in the
// last bits (different summation order, 1 / Sk as a multiplication).
constexpr int kKvsWaves = 8;
// DIAG: the heads are at most 32 channels wide (nhead >= 2), so KV[dd][v] is only needed where dd and v lie in the same
// 32-block: the two off-diagonal 32 x 32 tiles are neither accumulated (32 of a block's 320 MFMAs, 32 registers) nor
// reduced.  The merge weights sit in LDS (the fold reads d * dh of them per output row; from global that was a chain
// of L2 latencies per cloud).
// BF: the projection as split bf16 (x = hi + lo, W = hi + lo from the pcr_pack_weight_bf16x2_f32 image wkv_bf; the three
// products W_hi x_hi + W_hi x_lo + W_lo x_hi on v_mfma_f32_32x32x16_bf16, f32 accumulate: 96 MFMAs of 32 cycles instead
// of 256 of 64 per block).  Lane (t, h) then holds the channels 16 s + bf_kpos(h, .) of a 16-channel step -- the K order
// of the weight image -- so eight loaded / computed values convert into one A operand (bf_split8); K / V, the KV
// accumulation and the merge fold stay f32.
// XS: 16-channel steps of the key features in the BF form (c2 = 64 or 128: the FP_SA blocks)
// ONEW (round 4; short key sets, Sk <= 128: every gallery / SSG matching launch): ONE wave per cloud.  The trace of the
// 36864-cloud gallery launch (tools/trace_attn.py) put 58 % of a workgroup round into what follows the blocks: four
// wave-order reduction rounds through LDS with a barrier each, the fold, the closing barrier.  A wave that takes all of a
// cloud's blocks needs none of it: the KV tile is accumulated TRANSPOSED (V as the A operand: lane = dd, register r =
// v 8 g + 4 h + q), which makes register r of the tile the A operand of fold step r as it stands (contraction over the v
// pairs (v_r, v_r + 4) instead of (2 s, 2 s + 1): other rounding in the last bits, still one fixed order per cloud), the
// key sums never leave the wave, and eight clouds are in flight per workgroup with no barrier after the staging.
// GATE (pcr_live): the rounds walk the compact index of the live clouds; a slot past their end is a dead slot of the
// un-gated walk (it stays inside the barriers); a workgroup with no round at all leaves before it stages anything.
template <bool DIAG, bool BF, int XS = 4, bool ONEW = false, bool GATE = false>
__global__ __launch_bounds__(64 * kKvsWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void attn_kv_stream64_kernel(AttnArgs a) {
  static_assert(BF || XS == 4, "the f32 form is c2 = 64 only");
  constexpr int D = 64, LD = D + 1, KVS = D * LD + D;   // per-cloud reduction area: KVl [64][65] + key sums [64]
  constexpr int NKV = DIAG ? 2 : 4;
  constexpr int C2 = 16 * XS, WU = BF ? (XS + 4) * 512 : 4096, MINW = XS == 8 ? 4 : 2;   // weight image: 16-byte units
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  f32x4 *s_w = reinterpret_cast<f32x4 *>(smem);                   // [16 kb][128 couts][2 halves]: 64 KB
  f32x4 *s_p0 = reinterpret_cast<f32x4 *>(smem + 4 * WU);         // [64] {w0x, w0y, w0z, b0}
  float *s_bkv = smem + 4 * WU + 256;                             // [128]
  float *s_wm = s_bkv + 128;                                      // [64][65] merge weights
  float *s_red = s_wm + D * LD;                                   // [CPG][KVS]
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  LiveWalk lw{};
  if constexpr (GATE) {
    lw = live_walk(a);
    if ((long)blockIdx.x * (kKvsWaves / (ONEW ? 1 : 4)) >= lw.total) return;   // (cpg >= this: no round for this workgroup)
  }
  // The K rows x hidden columns of the image are all zeros in every block built without k_pos (FP_SA, both
  // corss_attention stages: wkv = [[Wk, 0], [Wv, Wv W2]]).  The staging copy looks: it ORs the magnitude bits (a -0.0 is a
  // zero) of the units of that block -- bf16 image: steps s2 >= XS, cout blocks 0 and 1, both parts; f32 image: k-blocks
  // kb >= 8, couts < 64 -- into s_kz.  kfull, one scalar per wave: the block holds a nonzero (or dbg 512 asks), and the
  // block loop runs the K half of the hidden steps too.
  // s_kz is the pad word of s_wm's last row, element [D - 1][D]: the rows are LD = D + 1 floats apart against bank conflicts
  // and hold D weights, so neither the staging below nor a fold (columns < D) touches it, and the plans' LDS size has it.
  static_assert(LD > D, "s_kz takes the pad column of s_wm's last row");
  unsigned *s_kz = reinterpret_cast<unsigned *>(s_wm + (D - 1) * LD + D);
  if (tid == 0) *s_kz = 0u;
  __syncthreads();
  {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(BF ? p.wkv_bf : p.wkv);   // (WU 16-byte units: 4096, or 6144 at XS = 8)
    unsigned nz = 0u;
    for (int e = tid; e < WU; e += 64 * kKvsWaves) {
      const f32x4 u = src[e];
      s_w[e] = u;
      const bool kz = BF ? ((e >> 9) >= XS && ((e >> 7) & 3) < 2) : ((e >> 8) >= 8 && ((e >> 1) & 127) < D);
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 ub = __builtin_bit_cast(u32x4, u);
      if (kz) nz |= (ub[0] | ub[1] | ub[2] | ub[3]) & (BF ? 0x7FFF7FFFu : 0x7FFFFFFFu);
    }
    if (nz) atomicOr(s_kz, 1u);
    for (int e = tid; e < D * D; e += 64 * kKvsWaves) s_wm[(e >> 6) * LD + (e & 63)] = p.wmerge[e];
    if (tid < D) s_p0[tid] = f32x4{p.pos0_w[3 * tid], p.pos0_w[3 * tid + 1], p.pos0_w[3 * tid + 2], p.pos0_b[tid]};
    if (tid < 2 * D) s_bkv[tid] = p.bkv[tid];
  }
  __syncthreads();
  const bool kfull = __builtin_amdgcn_readfirstlane((int)*s_kz) != 0 || (a.dbg & 512) != 0;
  const int nblk = p.Sk >> 5;
  // waves per cloud: min(4, Sk / 32) rounded down to a power of two, at least MINW -- i.e. two or four clouds per workgroup
  // round.  (Until round 6 a cloud took up to EIGHT waves: at Sk = 1024 the eight partial KV tiles then met in eight
  // barrier-separated rounds, and that reduction + the fold were 30 % of a round; with four waves a cloud's blocks amortise
  // them twice as well.  In-process A/B, profiles/r06_kv_wpc_ab.txt: kv[c2=64,Sk=1024] 0.182 -> 0.162 ms, [Sk=512] 0.119 ->
  // 0.095, [c2=128,Sk=512] 0.174 -> 0.149, [c2=128,Sk=256] 0.127 -> 0.095.  TWO waves per cloud measured another 5 % at
  // 1024 clouds per launch but leave half the chip idle from 512 clouds down -- pt4096's batch: 0.30 -> 0.51 ms -- and the
  // choice may not look at the batch: a pair's bits must not depend on the batch it travels in.)  Shape-only, like the rest.
  constexpr int kMaxWpc = 4;
  const int wpc = nblk < kMaxWpc ? nblk : kMaxWpc;
  int wpc2 = 1;
  while (wpc2 * 2 <= wpc) wpc2 *= 2;
  if (wpc2 < MINW) wpc2 = MINW;                                   // (c2 = 128: LDS holds two clouds' reduction areas)
  if constexpr (ONEW) wpc2 = 1;
  const int cpg = kKvsWaves / wpc2;                               // clouds per workgroup round
  const int cslot = wave / wpc2, wsub = wave - cslot * wpc2;      // this wave's cloud slot and rank inside it
  const float inv_sk = 1.0f / (float)p.Sk;
  float bias[4];
#pragma unroll
  for (int cb = 0; cb < 4; cb++) bias[cb] = s_bkv[cb * 32 + j];
  const int dh = D / p.nhead;
  // trace builds: waves 0 and 5 of the first workgroups stamp the shader clock
  AttnTrace trace;
  if constexpr (kTraceBuild)
    trace.begin((a.dbg & 256) && lane == 0 && (wave == 0 || wave == 5) && blockIdx.x < kATraceWgs,
                g_attn_trace, 2 * blockIdx.x + (wave ? 1 : 0));
  const long nB = GATE ? lw.total : (long)p.B;
  for (long c0 = (long)blockIdx.x * cpg; c0 < nB; c0 += (long)gridDim.x * cpg) {
    const bool live = c0 + cslot < nB;
    const long b = GATE ? (live ? lw.map(c0 + cslot) : 0) : c0 + cslot;
    trace.mark(4);
    f32x16 kv[NKV];
#pragma unroll
    for (int i = 0; i < NKV; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) kv[i][r] = 0.f;
    float ks0 = 0.f, ks1 = 0.f;
    if (live) {
      const float *feat = p.feat_k + (size_t)b * C2 * p.Sk;
      const float *xyz = p.xyz_k + (size_t)b * p.Sk * 3;
      const __amdgpu_buffer_rsrc_t rfeat =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(feat), 0, C2 * p.Sk * 4, 0x00020000);
      for (int blk = wsub; blk < nblk; blk += wpc2) {
        asm volatile("" ::: "memory");   // (the weight reads below stay inside the block loop: hoisted, they are 256 registers)
        trace.mark(0);
        const int t = blk * 32 + j;
        const float px = xyz[3 * t], py = xyz[3 * t + 1], pz = xyz[3 * t + 2];
        f32x16 acc[4];
        if constexpr (!BF) {
          float xr[64];
          {
            // buffer loads: ONE address register (lane part) + a scalar offset per channel pair
            const int vo = (h * p.Sk + t) * 4;
#pragma unroll
            for (int s2 = 0; s2 < 32; s2++)
              xr[s2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rfeat, vo, s2 * 2 * p.Sk * 4, 0));
          }
#pragma unroll
          for (int s2 = 0; s2 < 32; s2++) {
            const f32x4 w = s_p0[2 * s2 + h];
            const float v = w[0] * px + w[1] * py + w[2] * pz + w[3];
            xr[32 + s2] = fmaxf(v, 0.f);
          }
          // (all 32 feature loads are in flight above and land HERE: left alone, the register allocator sinks each load
          // to just before its MFMA and every k-step waits out a full memory latency)
#pragma unroll
          for (int s2 = 0; s2 < 32; s2++) asm volatile("" : "+v"(xr[s2]));
#pragma unroll
          for (int cb = 0; cb < 4; cb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[cb][r] = 0.f;   // (the bias joins in the epilogue: seeded, 64 registers of copies were live through the load phase)
          // cout blocks CB0 .. 3 of k-block kb: CB0 = 2 leaves out the K rows (their weight reads too)
          auto project = [&](auto first, int kb) {
            constexpr int CB0 = decltype(first)::value;
            f32x4 w[4];
#pragma unroll
            for (int cb = CB0; cb < 4; cb++) w[cb] = s_w[((kb * 128 + cb * 32 + j) << 1) + h];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
              for (int cb = CB0; cb < 4; cb++)
                acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[4 * kb + i], w[cb][i], acc[cb], 0, 0, 0);
          };
#pragma unroll
          for (int kb = 0; kb < 8; kb++) project(std::integral_constant<int, 0>{}, kb);
          // the hidden channels: the K rows only where their weights are not all zeros (kfull: wave-uniform, a scalar branch)
          if (kfull) {
#pragma unroll
            for (int kb = 8; kb < 16; kb++) project(std::integral_constant<int, 0>{}, kb);
          } else {
#pragma unroll
            for (int kb = 8; kb < 16; kb++) project(std::integral_constant<int, 2>{}, kb);
          }
        } else {
          float xf[8 * XS];
          {
            const int vo = (4 * h * p.Sk + t) * 4;
#pragma unroll
            for (int e = 0; e < 8 * XS; e++) {
              const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);   // + 4 h: in the lane offset
              xf[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rfeat, vo, ch * p.Sk * 4, 0));
            }
          }
          // (measured and dropped: the NEXT block's loads requested behind this block's, into the registers its split frees.
          // At XS = 4 it fits without scratch (231 registers against 194) and measured no gain -- +1.7 % at Sk = 1024; at
          // XS = 8 it spills 144 bytes: profiles/r16_kv64_skip_ab.txt, r16_kv64_skip_kres.txt)
#pragma unroll
          for (int e = 0; e < 8 * XS; e++) asm volatile("" : "+v"(xf[e]));   // (the loads land here, see the f32 form)
#pragma unroll
          for (int cb = 0; cb < 4; cb++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[cb][r] = 0.f;
          trace.mark(1);
          const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(s_w) + lane;
          // cout blocks CB0 .. 3 of step s2 with the A operand (xh, xl): CB0 = 2 leaves out the K rows (their weight reads too)
          auto project = [&](auto first, int s2, const bf16x8 xh, const bf16x8 xl) {
            constexpr int CB0 = decltype(first)::value;
            bf16x8 wh[4], wl[4];
#pragma unroll
            for (int cb = CB0; cb < 4; cb++) {
              wh[cb] = wb[((s2 * 4 + cb) * 2) * 64];
              wl[cb] = wb[((s2 * 4 + cb) * 2 + 1) * 64];
            }
#pragma unroll
            for (int cb = CB0; cb < 4; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, wh[cb], acc[cb], 0, 0, 0);
#pragma unroll
            for (int cb = CB0; cb < 4; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl, wh[cb], acc[cb], 0, 0, 0);
#pragma unroll
            for (int cb = CB0; cb < 4; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, wl[cb], acc[cb], 0, 0, 0);
          };
          // hidden channels 16 s2 + bf_kpos(h, .), the steps after the features': the operand of a step is formed right
          // before the step's MFMAs (all four ahead of the feature phase, they held 32 registers through it for nothing)
          auto hidden = [&](auto first, int s2) {
            asm volatile("" ::: "memory");   // (... and stays there: the hidden layer's rows are not read ahead)
            float hv[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
              const f32x4 w = s_p0[16 * s2 + bf_kpos(0, e) + 4 * h];
              const float v = w[0] * px + w[1] * py + w[2] * pz + w[3];
              hv[e] = relu_i(v);
            }
            bf16x8 hh, hl;
            bf_split8(hv, hh, hl, true);
            project(first, XS + s2, hh, hl);
          };
#pragma unroll
          for (int s2 = 0; s2 < XS; s2++) {   // the feature steps, split one at a time: eight registers of operands, not 8 XS
            float xv[8];
#pragma unroll
            for (int e = 0; e < 8; e++) xv[e] = xf[8 * s2 + e];
            bf16x8 xh, xl;
            bf_split8(xv, xh, xl, true);
            project(std::integral_constant<int, 0>{}, s2, xh, xl);
          }
          // the K rows of the hidden steps only where their weights are not all zeros (kfull: wave-uniform, a scalar branch)
          if (kfull) {
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) hidden(std::integral_constant<int, 0>{}, s2);
          } else {
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) hidden(std::integral_constant<int, 2>{}, s2);
          }
        }
        trace.mark(2);
#pragma unroll
        for (int r = 0; r < 16; r++) {
          acc[0][r] = elu1(acc[0][r] + bias[0]);
          acc[1][r] = elu1(acc[1][r] + bias[1]);
          acc[2][r] = (acc[2][r] + bias[2]) * inv_sk;
          acc[3][r] = (acc[3][r] + bias[3]) * inv_sk;
          ks0 += acc[0][r];
          ks1 += acc[1][r];
        }
#pragma unroll
        for (int i = 0; i < NKV; i++) {
          const int ib = DIAG ? i : (i >> 1), jb = DIAG ? i : (i & 1);
          // (round 6, measured and dropped: this accumulation as split bf16 too -- registers [8 st, 8 st + 8) of a K block and of a
          // V block hold the same eight tokens, so one bf_split8 of each feeds a 16-token step: 6 MFMAs of 32 cycles instead of 16
          // of 64 per tile.  kv[d=64,Sk=1024] 0.177 -> 0.166 ms, gallery128 -0.12 ms -- and the headline's deviation from the f32
          // path 2.7e-5 -> 3.2e-5, one case of the margin sweep past 5e-5: the KV state feeds every query token, its rounding does
          // not average out.  Stays f32.)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            if constexpr (ONEW) kv[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[2 + jb][r], acc[ib][r], kv[i], 0, 0, 0);
            else kv[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[ib][r], acc[2 + jb][r], kv[i], 0, 0, 0);
          }
        }
        trace.mark(3);
      }
    }
    trace.mark(5);
    ks0 += __shfl_xor(ks0, 32, 64);
    ks1 += __shfl_xor(ks1, 32, 64);
    if constexpr (ONEW) {
      // kv[i]: lane (dd = 32 ib + j, h), register r <-> v = 32 jb + 8 g + 4 h + q; fold tile (o block, dd block) from registers
      if (live) {
        float *kvo = p.kv + (size_t)b * ((size_t)D * D + D);
        bf16x8 *img = reinterpret_cast<bf16x8 *>(kvo);
#pragma unroll
        for (int db = 0; db < 2; db++) {
          const int hd = (db * 32 + j) / dh;
#pragma unroll
          for (int ob = 0; ob < 2; ob++) {
            f32x16 m;
#pragma unroll
            for (int r = 0; r < 16; r++) m[r] = 0.f;
#pragma unroll
            for (int i = 0; i < NKV; i++) {
              const int ib = DIAG ? i : (i >> 1), jb = DIAG ? i : (i & 1);
              if (ib != db) continue;
              const float *wr = s_wm + (ob * 32 + j) * LD + jb * 32 + 4 * h;
#pragma unroll
              for (int r = 0; r < 16; r++) {
                const int vl = (r & 3) + 8 * (r >> 2);
                const float av = (jb * 32 + vl + 4 * h) / dh == hd ? kv[i][r] : 0.f;
                m = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wr[vl], m, 0, 0, 0);
              }
            }
#pragma unroll
            for (int G = 0; G < 2; G++) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = m[8 * G + e];
              bf16x8 hi, lo;
              bf_split8(v, hi, lo, true);
              const size_t unit = (((size_t)(db * 2 + G) * (D >> 5) + ob) * 2) * 64 + h * 32 + j;
              img[unit] = hi;
              img[unit + 64] = lo;
            }
          }
        }
        if (h == 0) {
          kvo[(size_t)D * D + j] = ks0;
          kvo[(size_t)D * D + 32 + j] = ks1;
        }
      }
      trace.mark(6);
      trace.mark(7);
      trace.next();
      continue;
    }
    // the waves of a cloud add their KV / key sums into the cloud's LDS area in wave order
    float *KVl = s_red + cslot * KVS, *s_kt = KVl + D * LD;
    for (int round = 0; round < wpc2; round++) {
      if (wsub == round) {
#pragma unroll
        for (int i = 0; i < NKV; i++) {
          const int ib = DIAG ? i : (i >> 1), jb = DIAG ? i : (i & 1);
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int dd = ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, v = jb * 32 + j;
            float *dst = KVl + dd * LD + v;
            *dst = round == 0 ? kv[i][r] : *dst + kv[i][r];
          }
        }
        if (h == 0) {
          s_kt[j] = round == 0 ? ks0 : s_kt[j] + ks0;
          s_kt[32 + j] = round == 0 ? ks1 : s_kt[32 + j] + ks1;
        }
      }
      __syncthreads();
    }
    trace.mark(6);
    // merge fold M[o][dd] = sum_{v in head(dd)} Wm[o][v] KV[dd][v] on the matrix core: four 32 x 32 tiles (o block, dd
    // block) over the cloud's waves, operands straight from LDS (A = Wm rows, B = KV rows with the head mask applied on
    // the read; DIAG: only the dd block's own 32 columns exist), then the packed image of M and the key sums
    if (live) {
      float *kvo = p.kv + (size_t)b * ((size_t)D * D + D);
      for (int ti = wsub; ti < 4; ti += wpc2) {
        const int ob = ti >> 1, db = ti & 1;
        const float *ap = s_wm + (ob * 32 + j) * LD + h;
        const float *bp = KVl + (db * 32 + j) * LD + h;
        const int hd = (db * 32 + j) / dh;
        f32x16 m;
#pragma unroll
        for (int r = 0; r < 16; r++) m[r] = 0.f;
        const int s_lo = DIAG ? db * 16 : 0, s_hi = DIAG ? db * 16 + 16 : 32;
        if constexpr (kAPrec == 0) {
#pragma unroll 4
          for (int s2 = s_lo; s2 < s_hi; s2++) {
            const float bv = bp[2 * s2];
            m = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s2], (2 * s2 + h) / dh == hd ? bv : 0.f, m, 0, 0, 0);
          }
          const int dd = db * 32 + j;
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int o = ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int kb = dd >> 3, rem = dd & 7;
            kvo[(((size_t)kb * D + o) * 2 + (rem & 1)) * 4 + (rem >> 1)] = m[r];
          }
        } else {
          // the bf16 image wants, per (output row o, half h), the eight cin values 16 s + bf_kpos(h, .) as ONE 16-byte unit:
          // with the fold TRANSPOSED (KV rows as the A operand, Wm rows as B: the same products summed in the same order,
          // so the same bits) lane (o, h) holds dd = 8 g + 4 h + q in register 4 g + q -- registers [8 G, 8 G + 8) are
          // exactly the unit of step 2 db + G.  (Round 3 stored the untransposed tile element by element: 32 scattered
          // 2-byte stores per lane and tile, 0.5 ms of a 36864-cloud gallery launch.)
#pragma unroll 4
          for (int s2 = s_lo; s2 < s_hi; s2++) {
            const float bv = bp[2 * s2];
            m = __builtin_amdgcn_mfma_f32_32x32x2f32((2 * s2 + h) / dh == hd ? bv : 0.f, ap[2 * s2], m, 0, 0, 0);
          }
          bf16x8 *img = reinterpret_cast<bf16x8 *>(kvo);
#pragma unroll
          for (int G = 0; G < 2; G++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = m[8 * G + e];
            bf16x8 hi, lo;
            bf_split8(v, hi, lo, true);
            const size_t unit = (((size_t)(db * 2 + G) * (D >> 5) + ob) * 2) * 64 + h * 32 + j;
            img[unit] = hi;
            img[unit + 64] = lo;
          }
        }
      }
      for (int e = wsub * 64 + lane; e < D; e += 64 * wpc2) kvo[(size_t)D * D + e] = s_kt[e];
    }
    trace.mark(7);
    trace.next();
    __syncthreads();   // the next round overwrites the reduction areas
  }
}

#if PCR_ATTN_PREC != 0
// The same kernel shape for d = c2 = 32 (the SA1 self-attention), split-bf16 projection only: one K and one V block,
// one 32 x 32 KV tile per wave, one fold tile per cloud.
__global__ __launch_bounds__(64 * kKvsWaves) __attribute__((amdgpu_waves_per_eu(2, 4)))
void attn_kv_stream32_kernel(AttnArgs a) {
  constexpr int D = 32, LD = D + 1, KVS = D * LD + D;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  f32x4 *s_w = reinterpret_cast<f32x4 *>(smem);                   // bf image [4 steps][2 cb][hi, lo][64]: 1024 units
  f32x4 *s_p0 = reinterpret_cast<f32x4 *>(smem + 4096);           // [32] {w0x, w0y, w0z, b0}
  float *s_bkv = smem + 4096 + 128;                               // [64]
  float *s_wm = s_bkv + 64;                                       // [32][33] merge weights
  float *s_red = s_wm + D * LD;                                   // [CPG][KVS]
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(p.wkv_bf);
    for (int e = tid; e < 1024; e += 64 * kKvsWaves) s_w[e] = src[e];
    for (int e = tid; e < D * D; e += 64 * kKvsWaves) s_wm[(e >> 5) * LD + (e & 31)] = p.wmerge[e];
    if (tid < D) s_p0[tid] = f32x4{p.pos0_w[3 * tid], p.pos0_w[3 * tid + 1], p.pos0_w[3 * tid + 2], p.pos0_b[tid]};
    if (tid < 2 * D) s_bkv[tid] = p.bkv[tid];
  }
  __syncthreads();
  const int nblk = p.Sk >> 5;
  const int wpc = nblk < kKvsWaves ? nblk : kKvsWaves;
  int wpc2 = 1;
  while (wpc2 * 2 <= wpc) wpc2 *= 2;
  if (wpc2 < 2) wpc2 = 2;
  const int cpg = kKvsWaves / wpc2;
  const int cslot = wave / wpc2, wsub = wave - cslot * wpc2;
  const float inv_sk = 1.0f / (float)p.Sk;
  const float bias0 = s_bkv[j], bias1 = s_bkv[32 + j];
  const int dh = D / p.nhead;
  for (long c0 = (long)blockIdx.x * cpg; c0 < p.B; c0 += (long)gridDim.x * cpg) {
    const long b = c0 + cslot;
    const bool live = b < p.B;
    f32x16 kv;
#pragma unroll
    for (int r = 0; r < 16; r++) kv[r] = 0.f;
    float ks = 0.f;
    if (live) {
      const float *feat = p.feat_k + (size_t)b * D * p.Sk;
      const float *xyz = p.xyz_k + (size_t)b * p.Sk * 3;
      const __amdgpu_buffer_rsrc_t rfeat =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(feat), 0, D * p.Sk * 4, 0x00020000);
      for (int blk = wsub; blk < nblk; blk += wpc2) {
        asm volatile("" ::: "memory");
        const int t = blk * 32 + j;
        const float px = xyz[3 * t], py = xyz[3 * t + 1], pz = xyz[3 * t + 2];
        float xf[16];
        {
          const int vo = (4 * h * p.Sk + t) * 4;
#pragma unroll
          for (int e = 0; e < 16; e++) {
            const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);   // + 4 h: in the lane offset
            xf[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rfeat, vo, ch * p.Sk * 4, 0));
          }
        }
        bf16x8 ah[4], al[4];
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
          float hv[8];
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const f32x4 w = s_p0[16 * s2 + bf_kpos(0, e) + 4 * h];
            const float v = w[0] * px + w[1] * py + w[2] * pz + w[3];
            hv[e] = relu_i(v);
          }
          bf_split8(hv, ah[2 + s2], al[2 + s2], true);
        }
#pragma unroll
        for (int e = 0; e < 16; e++) asm volatile("" : "+v"(xf[e]));
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
          float xv[8];
#pragma unroll
          for (int e = 0; e < 8; e++) xv[e] = xf[8 * s2 + e];
          bf_split8(xv, ah[s2], al[s2], true);
        }
        f32x16 acc[2];
#pragma unroll
        for (int cb = 0; cb < 2; cb++)
#pragma unroll
          for (int r = 0; r < 16; r++) acc[cb][r] = 0.f;
        const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(s_w) + lane;
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++) {
          bf16x8 wh[2], wl[2];
#pragma unroll
          for (int cb = 0; cb < 2; cb++) {
            wh[cb] = wb[((s2 * 2 + cb) * 2) * 64];
            wl[cb] = wb[((s2 * 2 + cb) * 2 + 1) * 64];
          }
#pragma unroll
          for (int cb = 0; cb < 2; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s2], wh[cb], acc[cb], 0, 0, 0);
#pragma unroll
          for (int cb = 0; cb < 2; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s2], wh[cb], acc[cb], 0, 0, 0);
#pragma unroll
          for (int cb = 0; cb < 2; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s2], wl[cb], acc[cb], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
          acc[0][r] = elu1(acc[0][r] + bias0);
          acc[1][r] = (acc[1][r] + bias1) * inv_sk;
          ks += acc[0][r];
        }
#pragma unroll
        for (int r = 0; r < 16; r++) kv = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[0][r], acc[1][r], kv, 0, 0, 0);
      }
    }
    ks += __shfl_xor(ks, 32, 64);
    float *KVl = s_red + cslot * KVS, *s_kt = KVl + D * LD;
    for (int round = 0; round < wpc2; round++) {
      if (wsub == round) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          float *dst = KVl + ((r & 3) + 8 * (r >> 2) + 4 * h) * LD + j;
          *dst = round == 0 ? kv[r] : *dst + kv[r];
        }
        if (h == 0) s_kt[j] = round == 0 ? ks : s_kt[j] + ks;
      }
      __syncthreads();
    }
    if (live && wsub == 0) {
      float *kvo = p.kv + (size_t)b * ((size_t)D * D + D);
      const float *ap = s_wm + j * LD + h;
      const float *bp = KVl + j * LD + h;
      const int hd = j / dh;
      f32x16 m;
#pragma unroll
      for (int r = 0; r < 16; r++) m[r] = 0.f;
      // (transposed fold, whole 16-byte units per lane: see attn_kv_stream64_kernel)
#pragma unroll 4
      for (int s2 = 0; s2 < 16; s2++) {
        const float bv = bp[2 * s2];
        m = __builtin_amdgcn_mfma_f32_32x32x2f32((2 * s2 + h) / dh == hd ? bv : 0.f, ap[2 * s2], m, 0, 0, 0);
      }
      bf16x8 *img = reinterpret_cast<bf16x8 *>(kvo);
#pragma unroll
      for (int G = 0; G < 2; G++) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = m[8 * G + e];
        bf16x8 hi, lo;
        bf_split8(v, hi, lo, true);
        const size_t unit = (((size_t)G * (D >> 5)) * 2) * 64 + h * 32 + j;
        img[unit] = hi;
        img[unit + 64] = lo;
      }
      if (lane < D) kvo[(size_t)D * D + lane] = s_kt[lane];
    }
    __syncthreads();
  }
}
#endif

// second launch of the token-split form: one workgroup per cloud adds the splits' partials in order (fixed: the result
// does not depend on the schedule), applies the head mask and folds the merge projection
__global__ __launch_bounds__(kThreads) void attn_kv_fold_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  const int d = p.d, dh = d / p.nhead, ld = d + 1, nsplit = p.kv_splits, tid = threadIdx.x;
  const size_t b = blockIdx.x, per = (size_t)d * d + d;
  float *KVl = smem, *s_kt = smem + d * ld;
  const float *part = p.kv_part + b * nsplit * per;
  for (int e = tid; e < d * d + d; e += kThreads) {
    float v = part[e];
    for (int y = 1; y < nsplit; y++) v += part[(size_t)y * per + e];
    if (e < d * d) {
      const int dd = e / d, c = e - dd * d;
      KVl[dd * ld + c] = (dd / dh == c / dh) ? v : 0.f;
    } else {
      s_kt[e - d * d] = v;
    }
  }
  __syncthreads();
  attn_kv_fold_write(p, KVl, s_kt, b);
}

#if PCR_ATTN_PREC == 0
// d_model 256 / 512 (the 1.5M / 7M Point-Transformer configs, backbone_net.py:43-46,84-86): the per-cloud KV matrix
// no longer fits one workgroup's accumulators, so a cloud is split over d / 64 workgroups.  Workgroup (band g, cloud b)
// owns the rows dd in [64 g, 64 g + 64) of KV -- one head, since the head width is a multiple of 64 -- and therefore
// needs the K rows of its band and the V rows of its head: the host gathers exactly those rows of the fused K/V
// projection into one packed image per band (wkv_wide, 64 + dh couts), so the projection is one in-place dense call
// as in the narrow kernel.  With a whole head's V columns at hand the merge fold M[:, band] = Wm[:, head] KV_band^T
// is complete inside the workgroup (no cross-workgroup reduction) and runs on the matrix core as well.
//   NRW: cout-block rounds of the 64 + dh row projection (2 for dh = 128, 3 for dh = 256)
template <int NRW>
__global__ __launch_bounds__(kThreads) void attn_kv_wide_kernel(AttnArgs a) {
  constexpr int TB = 1, T = 32, RP = 33, BAND = 64, RPK = BAND + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  const int d = p.d, c2 = p.c2, dh = d / p.nhead;
  const int g = blockIdx.x, hd = (g * BAND) / dh;
  const int OPW = BAND + dh;                 // couts of this band's projection (multiple of 32)
  float *XH = smem;                          // [c2 + d][RP]: key features ; hidden -> rows [0,64) K band, [64,64+dh) V head
  float *KB = XH, *VB = XH + BAND * RP;
  float *P = XH + (c2 + d) * RP;
  float *s_w0 = P + 3 * RP, *s_b0 = s_w0 + 3 * d;
  float *s_ks = s_b0 + d;                    // [256] partial key sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const size_t b = blockIdx.y;
  for (int e = tid; e < 3 * d; e += kThreads) s_w0[e] = p.pos0_w[e];
  for (int e = tid; e < d; e += kThreads) s_b0[e] = p.pos0_b[e];
  const float *feat = p.feat_k + b * c2 * p.Sk;
  const float *xyz = p.xyz_k + b * p.Sk * 3;
  const float sk = (float)p.Sk;
  const float *wband = p.wkv_wide + (size_t)g * ((size_t)ceil8(c2 + d) * OPW);
  const float *bband = p.bkv_wide + (size_t)g * OPW;
  const int nj = dh >> 5, nT = 2 * nj;       // KV tiles (ib in {0,1}) x (jb < dh/32): 8 or 16, up to 4 per wave
  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
  const int krow = tid & (BAND - 1), kpart = tid >> 6;   // four partial sums per K row
  float ksum = 0.f;
  for (int t0 = 0; t0 < p.Sk; t0 += T) {
    const int valid = p.Sk - t0;
    load_tile(XH, RP, feat, c2, c2, p.Sk, t0, T);
    load_xyz3(P, RP, xyz, p.Sk, t0, T);
    __syncthreads();
    pos_hidden(XH + c2 * RP, RP, P, s_w0, s_b0, d, T);
    __syncthreads();
    tile_dense2<TB, NRW, 0, true>(XH, c2 + d, wband, OPW, true,
                                  [&](const f32x16 &acc, int cb, int tb, int l31, int h) {
      const int t = tb * 32 + l31;
      float *dst = XH + (cb * 32 + 4 * h) * RP + t;
      const bool live = t < valid;
      if (cb * 32 < BAND) {
#pragma unroll
        for (int r = 0; r < 16; r++) dst[((r & 3) + 8 * (r >> 2)) * RP] = live ? elu1(acc[r]) : 0.f;
      } else {
#pragma unroll
        for (int r = 0; r < 16; r++) dst[((r & 3) + 8 * (r >> 2)) * RP] = live ? acc[r] / sk : 0.f;
      }
    }, bband);
    __syncthreads();
    {
      const float *row = KB + krow * RP;
      for (int t = kpart; t < T; t += 4) ksum += row[t];
    }
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int item = wave + 4 * it;
      if (item < nT) {
        const int ib = item / nj, jb = item - ib * nj;
        const float *ap = KB + (ib * 32 + l31) * RP + h;
        const float *bp = VB + (jb * 32 + l31) * RP + h;
#pragma unroll 4
        for (int ks = 0; ks < T / 2; ks++)
          acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * ks], bp[2 * ks], acc[it], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // KV band, transposed: KVt [v (dh)][dd (64) + 1] = the B operand (k = v, token = dd) of the merge fold
  // (KVt spans dh * 65 floats from the start of the buffer and can reach past s_ks -- d_model 256 with ONE head and
  // c2 < 214 -- so the four key-sum partials are combined into a register before the first KVt write)
  float *KVt = smem;
  s_ks[tid] = ksum;
  __syncthreads();
  const float ks_total = tid < BAND ? s_ks[tid] + s_ks[64 + tid] + s_ks[128 + tid] + s_ks[192 + tid] : 0.f;
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; it++) {
    const int item = wave + 4 * it;
    if (item < nT) {
      const int ib = item / nj, jb = item - ib * nj;
      const int v = jb * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; r++) KVt[v * RPK + ib * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = acc[it][r];
    }
  }
  __syncthreads();
  float *kv = p.kv + b * ((size_t)d * d + d);
  if (tid < BAND) kv[(size_t)d * d + g * BAND + tid] = ks_total;
  // M[o][dd] = sum_{v < dh} Wm[o][hd dh + v] KV[dd][v]: dense over k = v with the k-blocks [hd dh / 8, +dh / 8) of the
  // packed merge weights; stored in the packed (d,d) layout the apply kernel reads as an A operand
  const float *wm = p.wmerge_packed + (size_t)(hd * dh / 8) * d * 8;
  tile_dense(KVt, dh, RPK, 2, wm, d, [&](float m, int o, int t) {
    const int dd = g * BAND + t;
    const int kb = dd >> 3, rem = dd & 7;
    kv[(((size_t)kb * d + o) * 2 + (rem & 1)) * 4 + (rem >> 1)] = m;
  });
}

#endif   // PCR_ATTN_PREC == 0 (wide kv kernel)

// One workgroup per (query cloud, tile of T query tokens), T = 128 / 64 / 32 for d = 32 / 64 / 128 (32 beyond).
// ONE LDS buffer U of max(c1 + d, 2d, cout, cfinal) rows, every dense phase in place (barrier between its
// k-loop and its epilogue), so a d = 64 tile is 33 KB and four workgroups share a CU:
//   rows [0,c1) query features x, rows [c1,c1+d) position hidden h  --Q-->  rows [c1,c1+d) = elu(.)+1
//   --scale by Sk/(Q.ksum)--> --M (kv image)--> message --LayerNorm--> [x ; msg] --FFN0--> 2d rows --FFN1-->
//   cout rows --LayerNorm--> (+ x, re-read from global: it was overwritten by FFN0) --cov_final--> store.
// GATE (pcr_live): the workgroups of a dead cloud leave at entry.
template <int TB, int NR, bool GATE = false>
__global__ __launch_bounds__(kThreads) void attn_apply_kernel(AttnArgs a) {
  if constexpr (GATE) {
    if (!live_cloud(a, blockIdx.y)) return;
  }
  constexpr int T = 32 * TB, RP = T + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  const int d = p.d, c1 = p.c1, cout = p.cout;
  const int catC = c1 + d, catP = ceil8(catC);
  int rowsU = catP > 2 * d ? catP : 2 * d;
  if (ceil32(cout) > rowsU) rowsU = ceil32(cout);
  if (ceil32(p.cfinal) > rowsU) rowsU = ceil32(p.cfinal);
  float *U = smem;
  float *P = U + rowsU * RP;
  float *zs = P + 3 * RP;
  float *red = zs + p.nhead * RP;  // [2 * (256/T)][T]
  // small constant vectors, staged once: reading them from global inside the per-element loops costs a
  // vector-memory instruction per use
  float *cst = red + 2 * (kThreads / T) * T;
  float *s_ksum = cst, *s_ln1g = cst + d, *s_ln1b = cst + 2 * d, *s_ln2g = cst + 3 * d, *s_ln2b = s_ln2g + cout;
  float *s_w0 = s_ln2b + cout, *s_b0 = s_w0 + 3 * d;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.y;
  const int t0 = blockIdx.x * T;
  const size_t bq_ = p.q_index ? (size_t)p.q_index[b] : b;    // which cloud supplies the query tokens
  const float *feat = p.feat_q + bq_ * c1 * p.Lq;
  const size_t kb_ = p.kv_index ? (size_t)p.kv_index[b] : b;
  const float *kv = p.kv + kb_ * ((size_t)d * d + d);
  const int dh = d / p.nhead;
  for (int e = tid; e < d; e += kThreads) {
    s_ksum[e] = kv[(size_t)d * d + e];
    s_ln1g[e] = p.ln1_g[e];
    s_ln1b[e] = p.ln1_b[e];
    if (p.q_pos) {
      s_w0[3 * e] = p.pos0_w[3 * e];
      s_w0[3 * e + 1] = p.pos0_w[3 * e + 1];
      s_w0[3 * e + 2] = p.pos0_w[3 * e + 2];
      s_b0[e] = p.pos0_b[e];
    }
  }
  for (int e = tid; e < cout; e += kThreads) {
    s_ln2g[e] = p.ln2_g[e];
    s_ln2b[e] = p.ln2_b[e];
  }
  const float *ksum = s_ksum;
  float *MSG = U + c1 * RP;   // rows [c1, c1+d): hidden -> Q -> message

  load_tile(U, RP, feat, c1, c1, p.Lq, t0, T);
  if (p.q_pos) {
    load_xyz3(P, RP, p.xyz_q + bq_ * p.Lq * 3, p.Lq, t0, T);
    __syncthreads();
    pos_hidden(MSG, RP, P, s_w0, s_b0, d, T);
    for (int e = tid; e < (catP - catC) * T; e += kThreads) U[(catC + e / T) * RP + e % T] = 0.f;
  } else {
    for (int e = tid; e < (catP - c1) * T; e += kThreads) U[(c1 + e / T) * RP + e % T] = 0.f;
  }
  __syncthreads();
  // Q = elu(Wq' [x ; h] + bq) + 1, written over h
  tile_dense2p<kAPrec, TB, NR>(U, p.q_pos ? catP : ceil8(c1), p.wq, d, true,
                               [&](float v, int o, int t) { MSG[o * RP + t] = elu1(v); }, p.bq);
  __syncthreads();
  for (int e = tid; e < p.nhead * T; e += kThreads) {
    const int hd = e / T, t = e - hd * T;
    float z = 0.f;
    for (int c = 0; c < dh; c++) z += MSG[(hd * dh + c) * RP + t] * ksum[hd * dh + c];
    zs[hd * RP + t] = (1.0f / (z + 1e-6f)) * (float)p.Sk;
  }
  __syncthreads();
  for (int hd = 0; hd < p.nhead; hd++)   // (head-major: no runtime division per element)
    for (int e = tid; e < dh * T; e += kThreads) {
      const int o = hd * dh + e / T, t = e % T;
      MSG[o * RP + t] *= zs[hd * RP + t];
    }
  __syncthreads();
  tile_dense2p<kAPrec, TB, NR>(MSG, d, kv, d, true, [&](float v, int o, int t) { MSG[o * RP + t] = v; });
  __syncthreads();
  tile_layernorm(MSG, d, RP, T, s_ln1g, s_ln1b, red);
  tile_dense2p<kAPrec, TB, NR>(U, catP, p.wmlp0, 2 * d, true, [&](float v, int o, int t) { U[o * RP + t] = fmaxf(v, 0.f); });
  __syncthreads();
  tile_dense2p<kAPrec, TB, NR>(U, 2 * d, p.wmlp2, ceil32(cout), true, [&](float v, int o, int t) { U[o * RP + t] = v; });
  __syncthreads();
  tile_layernorm(U, cout, RP, T, s_ln2g, s_ln2b, red);
  if (p.residual) {   // cout == c1: add the query features back (re-read: FFN0 has overwritten them)
    for (int e = tid; e < cout * T; e += kThreads) {
      const int c = e / T, t = e - c * T;
      if (t0 + t < p.Lq) U[c * RP + t] += feat[(size_t)c * p.Lq + t0 + t];
    }
    __syncthreads();
  }
  int cres = cout;
  if (p.cfinal) {  // trailing 1x1 conv with bias (cov_final); needs cout % 8 == 0
    const int cf = p.cfinal;
    tile_dense2p<kAPrec, TB, NR>(U, cout, p.wfinal, ceil32(cf), true, [&](float v, int o, int t) { U[o * RP + t] = v; },
                                 p.bfinal);   // bfinal is zero-padded to a multiple of 32 by the host
    __syncthreads();
    cres = cf;
  }
  float *out = p.out + b * cres * p.Lq;
  for (int e = tid; e < cres * T; e += kThreads) {
    const int c = e / T, t = e - c * T;
    if (t0 + t < p.Lq) out[(size_t)c * p.Lq + t0 + t] = U[c * RP + t];
  }
}

#if PCR_ATTN_PREC != 0
// ---- wave-autonomous apply kernel, d = c1 = cout = 64, split bf16, no trailing conv, whole 32-token blocks ----------
// (gallery / SSG matching: every apply launch; pt1024: the three self / cross attention launches of SA2 and the matching
// stages.)  A wave owns a 32-token block from the feature load to the output store -- NO workgroup barrier after the
// weights are staged.  Every dense phase is in the normal orientation D[cout][token] with the activations as the B
// operand held in registers, lane (t, h) = token t, k-group h:
//   * the bf16 weight images order the 16 channels of a step as 16 s + bf_kpos(h, j) -- the order in which a 32 x 32
//     accumulator tile hands its rows to a lane -- so registers [8 G, 8 G + 8) of cout block cb of one phase's
//     accumulators convert (bf_split8) into the B operand of step s = 2 cb + G of the NEXT phase: Q -> message -> FFN0 ->
//     FFN1 chain through registers, no LDS tile, no transposition;
//   * the input is loaded in the same order, so element i of the lane's 32 feature values is also element i of the
//     final accumulators (the residual add) and of the output store;
//   * LayerNorm over the 64 channels of a token = the lane's 32 registers + its partner lane (lane ^ 32): two
//     cross-lane adds per moment instead of two barrier-separated passes over an LDS tile; the per-head normaliser of
//     linear attention likewise;
//   * the per-cloud matrix M (bf16 image written by the kv kernel) is the A operand of the message phase, read straight
//     from global memory / L2 by each wave; the three weight images (128 KB) live in LDS, staged once by a persistent
//     workgroup of eight waves (two per SIMD).
constexpr int kApsWaves = 8;
// C1S: 16-channel steps of the query features (c1 = 64 or 32; 32: the FP_SA blocks, no residual); CF: trailing 64 -> 128
// conv (cov_final), its weight image read from global memory / L2 like M
// NOB: 32-channel blocks of the block's output (cout = 64, or 128: no residual, no trailing conv)
// (CF as an int: 32-channel blocks of the trailing conv's output, 0 = none -- 64 -> 128 and the first FP_SA block's 32 -> 64)
// ND: d_model / 32 (2: d = 64; 1: d = 32, the SA1 self-attention)
// POOL (round 6; the gallery's stage-2 launch): the block's output is not stored -- the wave keeps ALL blocks of a virtual
// cloud, reduces every block's 32 tokens per channel with a TRANSPOSING butterfly (five exchange steps; a lane keeps half
// of its registers per step, so the steps cost 16 + 8 + 4 + 2 + 1 registers, not 5 x 32) and writes the cloud's
// per-channel maximum and sum: p.pool_out (B, 2, 64) -- 512 bytes per cloud instead of 32 KB that pool_head would read back.
// GATE (pcr_live): the items are the blocks (POOL: the clouds) of the live clouds only, by their compact index; a workgroup
// with no item leaves before it stages anything.
template <bool QPOS, int C1S, int CF, int NOB = 2, int ND = 2, bool POOL = false, bool GATE = false>
__global__ __launch_bounds__(64 * kApsWaves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void attn_apply_stream64_kernel(AttnArgs a) {
  static_assert(!QPOS || C1S == 2 * ND, "q_pos needs c1 == d");
  static_assert(NOB <= 2 || (NOB == 4 && !CF), "cout = 128 has no trailing conv");
  static_assert(!POOL || (!CF && NOB == 2), "pooled output: cout = 64, no trailing conv");
  constexpr int D = 32 * ND, SD = 2 * ND;   // d_model, its 16-channel steps
  constexpr int SQ = C1S + (QPOS ? SD : 0), S0 = C1S + SD, NX = 8 * C1S;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  bf16x8 *s_wq = reinterpret_cast<bf16x8 *>(smem);   // [SQ][ND cb][hi, lo][64]
  bf16x8 *s_w0 = s_wq + SQ * ND * 128;               // [S0][2 ND][2][64]
  bf16x8 *s_w2 = s_w0 + S0 * ND * 256;               // [4 ND][NOB][2][64]
  float *s_c = reinterpret_cast<float *>(s_w2 + ND * NOB * 512);   // bq | ln1 g | ln1 b : 3 x 64 | ln2 g | ln2 b : 2 x 32 NOB | (bfinal 128)
  f32x4 *s_p0 = reinterpret_cast<f32x4 *>(s_c + 448);    // [64] {w0x, w0y, w0z, b0}
  float *s_ks = reinterpret_cast<float *>(s_p0 + 64);    // [waves][64] key sums of the wave's current cloud
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  LiveWalk lw{};
  if constexpr (GATE) {
    lw = live_walk(a);
    if ((long)blockIdx.x * kApsWaves >= lw.total * (POOL ? 1 : (p.Lq >> 5))) return;
  }
  {
    // (c1 not a multiple of 16: the padded image of mlp[0]; the packer pads wq's single step with zero columns itself)
    const f32x4 *wq = reinterpret_cast<const f32x4 *>(p.wq),
                *w0 = reinterpret_cast<const f32x4 *>((p.c1 & 15) ? p.wmlp0_bf_xpad : p.wmlp0),
                *w2 = reinterpret_cast<const f32x4 *>(p.wmlp2);
    f32x4 *dq = reinterpret_cast<f32x4 *>(s_wq), *d0 = reinterpret_cast<f32x4 *>(s_w0), *d2 = reinterpret_cast<f32x4 *>(s_w2);
    for (int e = tid; e < SQ * ND * 128; e += 64 * kApsWaves) dq[e] = wq[e];
    for (int e = tid; e < S0 * ND * 256; e += 64 * kApsWaves) d0[e] = w0[e];
    for (int e = tid; e < ND * NOB * 512; e += 64 * kApsWaves) d2[e] = w2[e];
    if (tid < D) {
      s_c[tid] = p.bq[tid];
      s_c[64 + tid] = p.ln1_g[tid];
      s_c[128 + tid] = p.ln1_b[tid];

      if (QPOS) s_p0[tid] = f32x4{p.pos0_w[3 * tid], p.pos0_w[3 * tid + 1], p.pos0_w[3 * tid + 2], p.pos0_b[tid]};
    }
    if (tid < 32 * NOB) {
      s_c[192 + tid] = p.ln2_g[tid];
      s_c[192 + 32 * NOB + tid] = p.ln2_b[tid];
    }
    if (CF && tid < 32 * CF) s_c[320 + tid] = p.bfinal[tid];
  }
  __syncthreads();
  const int nblk = p.Lq >> 5;
  const long nB = GATE ? lw.total : (long)p.B;
  const long nitem = nB * nblk;
  const int dh = D / p.nhead;
  const float skf = (float)p.Sk;
  float *ksw = s_ks + wave * 64;
  // constants of the lane's registers (cout = 32 cb + 8 g + 4 h + q): 16-byte reads at 32 cb + 8 g + 4 h
  auto cvec = [&](const float *base, int cb, int g) __attribute__((always_inline)) {
    return *reinterpret_cast<const f32x4 *>(base + 32 * cb + 8 * g + 4 * h);
  };
  auto to_ops = [&](const f32x16 &acc, int G, bf16x8 &oh, bf16x8 &ol) __attribute__((always_inline)) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = acc[8 * G + e];
    bf_split8(v, oh, ol, true);
  };
  // trace builds: waves 0 and 5 of the first workgroups stamp the shader clock
  AttnTrace trace;
  if constexpr (kTraceBuild)
    trace.begin((a.dbg & 256) && lane == 0 && (wave == 0 || wave == 5) && blockIdx.x < kATraceWgs,
                g_attn_trace, 2 * blockIdx.x + (wave ? 1 : 0));
  // item walk: (cloud, block) dealt block by block over the waves -- or, POOL, cloud by cloud (all blocks of a cloud on one
  // wave, in order: the running maximum / sum of the cloud live in two registers)
  const long nwav = (long)gridDim.x * kApsWaves, gw = (long)blockIdx.x * kApsWaves + wave;
  long pc = gw;
  int pblk = 0;
  float pmax = -INFINITY, psum = 0.f;
  for (long it = gw; POOL ? pc < nB : it < nitem; it += POOL ? 0 : nwav) {
    asm volatile("" ::: "memory");   // (weight reads stay inside the item loop)
    trace.mark(0);
    const long vb = POOL ? pc : it / nblk;   // (GATE: the cloud's compact index)
    const int blk = POOL ? pblk : (int)(it - vb * nblk);
    const long b = GATE ? lw.map(vb) : vb;
    const size_t bq_ = p.q_index ? (size_t)p.q_index[b] : (size_t)b;
    const size_t kb_ = p.kv_index ? (size_t)p.kv_index[b] : (size_t)b;
    const float *kvp = p.kv + kb_ * ((size_t)D * D + D);
    const int t = blk * 32 + j;
    const __amdgpu_buffer_rsrc_t rfeat = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.feat_q + bq_ * p.c1 * p.Lq), 0, p.c1 * p.Lq * 4, 0x00020000);   // (channels past c1 read as 0)
    const int vo = (4 * h * p.Lq + t) * 4;
    float xf[NX];
#pragma unroll
    for (int e = 0; e < NX; e++) {
      const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);   // + 4 h: in the lane offset
      xf[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rfeat, vo, ch * p.Lq * 4, 0));
    }
    if (lane < D) ksw[lane] = kvp[(size_t)D * D + lane];
    bf16x8 bh[4 * ND], bl[4 * ND];
    if constexpr (QPOS) {
      const float *xyz = p.xyz_q + (bq_ * p.Lq + t) * 3;
      const float px = xyz[0], py = xyz[1], pz = xyz[2];
#pragma unroll
      for (int s2 = 0; s2 < SD; s2++) {
        float hv[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const f32x4 w = s_p0[16 * s2 + bf_kpos(0, e) + 4 * h];
          const float v = w[0] * px + w[1] * py + w[2] * pz + w[3];
          hv[e] = relu_i(v);
        }
        bf_split8(hv, bh[C1S + s2], bl[C1S + s2], true);
      }
    }
#pragma unroll
    for (int e = 0; e < NX; e++) asm volatile("" : "+v"(xf[e]));   // (the loads land here: see attn_kv_stream64_kernel)
#pragma unroll
    for (int s2 = 0; s2 < C1S; s2++) {
      float xv[8];
#pragma unroll
      for (int e = 0; e < 8; e++) xv[e] = xf[8 * s2 + e];
      bf_split8(xv, bh[s2], bl[s2], true);
    }
    trace.mark(1);
    // ---- Q = elu(Wq [x ; h] + bq) + 1
    f32x16 q[ND];
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) q[cb][r] = 0.f;
    {
      const bf16x8 *wb = s_wq + lane;
#pragma unroll
      for (int s2 = 0; s2 < SQ; s2++) {
        bf16x8 wh[ND], wl[ND];
#pragma unroll
        for (int cb = 0; cb < ND; cb++) {
          wh[cb] = wb[((s2 * ND + cb) * 2) * 64];
          wl[cb] = wb[((s2 * ND + cb) * 2 + 1) * 64];
        }
#pragma unroll
        for (int cb = 0; cb < ND; cb++) q[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bh[s2], q[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < ND; cb++) q[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bl[s2], q[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < ND; cb++) q[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[cb], bh[s2], q[cb], 0, 0, 0);
      }
    }
    trace.mark(2);
    // the message-phase A operands (the cloud's matrix M): requested now, used after the normaliser
    bf16x8 mh[SD][ND], ml[SD][ND];
    {
      const bf16x8 *mb = reinterpret_cast<const bf16x8 *>(kvp) + lane;
#pragma unroll
      for (int s2 = 0; s2 < SD; s2++)
#pragma unroll
        for (int cb = 0; cb < ND; cb++) {
          mh[s2][cb] = mb[((s2 * ND + cb) * 2) * 64];
          ml[s2][cb] = mb[((s2 * ND + cb) * 2 + 1) * 64];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the wave's own key-sum strip: written above, read below)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // z[head][token] = Q_head . ksum_head; partial sums per 16-channel group (cb, G), then by head width
    float z16[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const f32x4 bqv = cvec(s_c, cb, g), ksv = cvec(ksw, cb, g);
        float zz = 0.f;
#pragma unroll
        for (int qq = 0; qq < 4; qq++) {
          const float v = elu1(q[cb][4 * g + qq] + bqv[qq]);
          q[cb][4 * g + qq] = v;
          zz += v * ksv[qq];
        }
        if ((g & 1) == 0) z16[cb][g >> 1] = zz;
        else z16[cb][g >> 1] += zz;
      }
    float zs[2][2];
    {
      float za = z16[0][0], zb = z16[0][1], zc = z16[1][0], zd = z16[1][1];
      if (dh >= 32) {
        za += zb; zb = za;
        zc += zd; zd = zc;
      }
      if (ND == 2 && dh >= 64) {
        za += zc; zb = za; zc = za; zd = za;
      }
      za += __shfl_xor(za, 32, 64);
      zb += __shfl_xor(zb, 32, 64);
      zc += __shfl_xor(zc, 32, 64);
      zd += __shfl_xor(zd, 32, 64);
      zs[0][0] = (1.0f / (za + 1e-6f)) * skf;
      zs[0][1] = (1.0f / (zb + 1e-6f)) * skf;
      zs[1][0] = (1.0f / (zc + 1e-6f)) * skf;
      zs[1][1] = (1.0f / (zd + 1e-6f)) * skf;
    }
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) q[cb][r] *= zs[cb][r >> 3];
    // ---- message = M Q'
    bf16x8 ch_[SD], cl_[SD];
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int G = 0; G < 2; G++) to_ops(q[cb], G, ch_[2 * cb + G], cl_[2 * cb + G]);
    f32x16 m[ND];
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) m[cb][r] = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < SD; s2++) {
#pragma unroll
      for (int cb = 0; cb < ND; cb++) m[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mh[s2][cb], ch_[s2], m[cb], 0, 0, 0);
#pragma unroll
      for (int cb = 0; cb < ND; cb++) m[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mh[s2][cb], cl_[s2], m[cb], 0, 0, 0);
#pragma unroll
      for (int cb = 0; cb < ND; cb++) m[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ml[s2][cb], ch_[s2], m[cb], 0, 0, 0);
    }
    // ---- LayerNorm over the 64 channels of a token (two passes, eps inside the sqrt: tile_layernorm's arithmetic)
    auto layernorm = [&](auto &v, auto nb_tag, const float *gam, const float *bet) __attribute__((always_inline)) {
      constexpr int NB = decltype(nb_tag)::value;
      float sm = 0.f;
#pragma unroll
      for (int cb = 0; cb < NB; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) sm += v[cb][r];
      sm += __shfl_xor(sm, 32, 64);
      const float mean = sm / (32.0f * NB);
      float vr = 0.f;
#pragma unroll
      for (int cb = 0; cb < NB; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float dlt = v[cb][r] - mean;
          vr += dlt * dlt;
        }
      vr += __shfl_xor(vr, 32, 64);
      const float inv = 1.0f / sqrtf(vr / (32.0f * NB) + 1e-5f);
#pragma unroll
      for (int cb = 0; cb < NB; cb++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const f32x4 gv = cvec(gam, cb, g), bv = cvec(bet, cb, g);
#pragma unroll
          for (int qq = 0; qq < 4; qq++) v[cb][4 * g + qq] = (v[cb][4 * g + qq] - mean) * inv * gv[qq] + bv[qq];
        }
    };
    trace.mark(3);
    layernorm(m, std::integral_constant<int, ND>{}, s_c + 64, s_c + 128);
    trace.mark(4);
    // ---- FFN0: relu(W0 [x ; msg]) (128 couts), operands: x re-converted from its f32 registers, msg from m
#pragma unroll
    for (int s2 = 0; s2 < C1S; s2++) {
      float xv[8];
#pragma unroll
      for (int e = 0; e < 8; e++) xv[e] = xf[8 * s2 + e];
      bf_split8(xv, bh[s2], bl[s2], true);
    }
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int G = 0; G < 2; G++) to_ops(m[cb], G, bh[C1S + 2 * cb + G], bl[C1S + 2 * cb + G]);
    f32x16 f[SD];
#pragma unroll
    for (int cb = 0; cb < SD; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) f[cb][r] = 0.f;
    {
      const bf16x8 *wb = s_w0 + lane;
#pragma unroll
      for (int s2 = 0; s2 < S0; s2++) {
        bf16x8 wh[SD], wl[SD];
#pragma unroll
        for (int cb = 0; cb < SD; cb++) {
          wh[cb] = wb[((s2 * SD + cb) * 2) * 64];
          wl[cb] = wb[((s2 * SD + cb) * 2 + 1) * 64];
        }
#pragma unroll
        for (int cb = 0; cb < SD; cb++) f[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bh[s2], f[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < SD; cb++) f[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bl[s2], f[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < SD; cb++) f[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[cb], bh[s2], f[cb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int cb = 0; cb < SD; cb++) {
#pragma unroll
      for (int r = 0; r < 16; r++) f[cb][r] = relu_i(f[cb][r]);
#pragma unroll
      for (int G = 0; G < 2; G++) to_ops(f[cb], G, bh[2 * cb + G], bl[2 * cb + G]);
    }
    trace.mark(5);
    // ---- FFN1 (64 couts), LayerNorm, residual, store
    f32x16 o[NOB];
#pragma unroll
    for (int cb = 0; cb < NOB; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) o[cb][r] = 0.f;
    {
      const bf16x8 *wb = s_w2 + lane;
#pragma unroll
      for (int s2 = 0; s2 < 4 * ND; s2++) {
        bf16x8 wh[NOB], wl[NOB];
#pragma unroll
        for (int cb = 0; cb < NOB; cb++) {
          wh[cb] = wb[((s2 * NOB + cb) * 2) * 64];
          wl[cb] = wb[((s2 * NOB + cb) * 2 + 1) * 64];
        }
#pragma unroll
        for (int cb = 0; cb < NOB; cb++) o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bh[s2], o[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NOB; cb++) o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bl[s2], o[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NOB; cb++) o[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[cb], bh[s2], o[cb], 0, 0, 0);
      }
    }
    trace.mark(6);
    layernorm(o, std::integral_constant<int, NOB>{}, s_c + 192, s_c + 192 + 32 * NOB);
    if constexpr (C1S == 2 * NOB) {   // cout == c1
      if (p.residual) {
#pragma unroll
        for (int cb = 0; cb < NOB; cb++)
#pragma unroll
          for (int r = 0; r < 16; r++) o[cb][r] += xf[16 * cb + r];
      }
    }
    if constexpr (POOL) {
      // lane (j, h) holds the block's token j in the 32 channels ch(e) = 16 (e >> 3) + bf_kpos(h, e & 7), e = 0 .. 31.  Step s
      // exchanges with lane j ^ (1 << s): the lane with bit s set keeps the upper half of its register list, its partner
      // the lower half (t = what I keep, u = what my partner keeps), so after five steps lane j holds the maximum and the
      // sum over the 32 tokens of ONE channel: e = bitreverse5(j).  (Sums: a fixed pairwise tree per block, blocks in order.)
      float vm[16], vs[16];
      {
        const bool up = (j & 1) != 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float lo_ = o[r >> 4][r & 15], hi_ = o[(r + 16) >> 4][(r + 16) & 15];
          const float tk = up ? hi_ : lo_, uk = up ? lo_ : hi_;
          const float pu = __uint_as_float(pcr_sort_partner<2, 1>(__float_as_uint(uk), lane));
          vm[r] = fmaxf(tk, pu);
          vs[r] = tk + pu;
        }
      }
#define PCR_POOL_STEP(N, J, BIT)                                                                      \
      {                                                                                               \
        const bool up = (j & BIT) != 0;                                                               \
        _Pragma("unroll") for (int r = 0; r < N; r++) {                                               \
          const float tm = up ? vm[r + N] : vm[r], um = up ? vm[r] : vm[r + N];                       \
          const float ts = up ? vs[r + N] : vs[r], us = up ? vs[r] : vs[r + N];                       \
          vm[r] = fmaxf(tm, __uint_as_float(pcr_sort_partner<2 * J, J>(__float_as_uint(um), lane)));  \
          vs[r] = ts + __uint_as_float(pcr_sort_partner<2 * J, J>(__float_as_uint(us), lane));        \
        }                                                                                             \
      }
      PCR_POOL_STEP(8, 2, 2)
      PCR_POOL_STEP(4, 4, 4)
      PCR_POOL_STEP(2, 8, 8)
      PCR_POOL_STEP(1, 16, 16)
#undef PCR_POOL_STEP
      pmax = fmaxf(pmax, vm[0]);
      psum += vs[0];
      if (++pblk == nblk) {
        const int e = ((j & 1) << 4) | ((j & 2) << 2) | (j & 4) | ((j & 8) >> 2) | ((j & 16) >> 4);
        const int ch = 16 * (e >> 3) + bf_kpos(h, e & 7);
        float *po = p.pool_out + (size_t)b * 128;
        po[ch] = pmax;
        po[64 + ch] = psum;
        pmax = -INFINITY;
        psum = 0.f;
        pblk = 0;
        pc += nwav;
      }
    } else if constexpr (!CF) {
      const __amdgpu_buffer_rsrc_t rout =
          __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)b * (32 * NOB) * p.Lq, 0, 32 * NOB * p.Lq * 4, 0x00020000);
#pragma unroll
      for (int e = 0; e < 16 * NOB; e++) {
        const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);
        const float v = o[e >> 4][e & 15];   // (a copy: __builtin_bit_cast of a vector ELEMENT reads element 0)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, vo, ch * p.Lq * 4, 0);
      }
    } else {
      // ---- cov_final (32 NOB -> 32 CF channels, bias), A operands from the global image
#pragma unroll
      for (int cb = 0; cb < NOB; cb++)
#pragma unroll
        for (int G = 0; G < 2; G++) to_ops(o[cb], G, bh[2 * cb + G], bl[2 * cb + G]);
      f32x16 fo[CF ? CF : 1];
#pragma unroll
      for (int cb = 0; cb < CF; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) fo[cb][r] = 0.f;
      const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(p.wfinal) + lane;
#pragma unroll
      for (int s2 = 0; s2 < 2 * NOB; s2++) {
        bf16x8 wh[CF ? CF : 1], wl[CF ? CF : 1];
#pragma unroll
        for (int cb = 0; cb < CF; cb++) {
          wh[cb] = wb[((s2 * CF + cb) * 2) * 64];
          wl[cb] = wb[((s2 * CF + cb) * 2 + 1) * 64];
        }
#pragma unroll
        for (int cb = 0; cb < CF; cb++) fo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bh[s2], fo[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < CF; cb++) fo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[cb], bl[s2], fo[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < CF; cb++) fo[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[cb], bh[s2], fo[cb], 0, 0, 0);
      }
      const __amdgpu_buffer_rsrc_t rout =
          __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)b * (32 * CF) * p.Lq, 0, 32 * CF * p.Lq * 4, 0x00020000);
#pragma unroll
      for (int cb = 0; cb < CF; cb++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const f32x4 bv = cvec(s_c + 320, cb, g);
#pragma unroll
          for (int qq = 0; qq < 4; qq++) {
            const int e = 16 * cb + 4 * g + qq;
            const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);
            const float v = fo[cb][4 * g + qq] + bv[qq];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, vo, ch * p.Lq * 4, 0);
          }
        }
    }
    __builtin_amdgcn_wave_barrier();   // (the key-sum strip is rewritten by the next item)
    trace.mark(7);
    trace.next();
  }
}

// ---- the same wave-autonomous form at d = c1 = cout = 128 (SA3's self-attention: q_pos, residual, no trailing conv) --------
// A wave owns a 32-token block from the feature load to the store and chains Q -> message -> FFN0 -> FFN1 through its
// registers exactly as attn_apply_stream64_kernel does (same operand orders, same LayerNorm / normaliser arithmetic).  What
// differs is where the weights come from: the three images are 512 KB (Wq 256 -> 128, FFN0 256 -> 256, FFN1 256 -> 128, bf16
// hi / lo), far beyond LDS.  They are streamed, in the order the phases consume them, as 16 chunks of 32 KB through a
// two-slot LDS ring that the waves of a persistent workgroup share: every wave runs the same phase on its own block, so one
// barrier per chunk is the only synchronisation, and the L2 weight traffic is divided by the waves per workgroup (the tile
// kernel re-reads all 512 KB per 32-token tile).  Chunk k + 1 is fetched into registers (eight 16-byte pieces per thread)
// while chunk k is on the matrix core and written to the other slot before the barrier; the stream is the same for every
// block, so the last chunk's fetch is the next block's first.  Each chunk is 48 MFMAs per wave (Q: four steps x four cout
// blocks, FFN0: two steps x eight, FFN1: four steps x four).
// Registers: FFN0's input [x ; msg] is 16 steps x 8 (hi / lo) and its accumulators 8 x 16 -- more than two waves per SIMD
// hold -- so the kernel runs ONE wave per SIMD with the whole 512-register file (four waves per workgroup, one workgroup
// per CU; tools/kres.py: 256 VGPRs + 210 AGPRs, no scratch) instead of chunking FFN0 by hidden channels.  x's operands
// from the Q phase are kept for FFN0 (the same steps), the f32 features are re-read for the residual under FFN1, and
// FFN1's operands are converted chunk by chunk.  The per-cloud matrix M (64 KB bf16 image) is read per wave from global
// memory / L2 one step ahead of its MFMAs.
// NH: heads (1, 2, 4), a template argument so the normaliser's head sums unroll.
// one 16-channel step (ls) of a ring chunk against NB cout blocks, four blocks at a time: 8 ds_read_b128 feed 12 MFMAs; the
// compiler barrier keeps the next group's reads from being hoisted over this group's (a chunk's reads all at once are
// 128 registers).  TRANS: the activations are the A operand (Y^T = X^T W^T: lane (cout, h) holds tokens 8 g + 4 h + q,
// attn_kv_stream128_kernel); the weight image serves both roles unchanged.
template <int NB, bool TRANS = false>
__device__ __forceinline__ void ap128_step(f32x16 (&acc)[NB], const bf16x8 *wb, int ls, const bf16x8 &bh, const bf16x8 &bl) {
  auto mm = [](const bf16x8 &w, const bf16x8 &x, const f32x16 &c) __attribute__((always_inline)) {
    return TRANS ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, w, c, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, x, c, 0, 0, 0);
  };
#pragma unroll
  for (int c0 = 0; c0 < NB; c0 += 4) {
    bf16x8 wh[4], wl[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) {
      wh[cb] = wb[((ls * NB + c0 + cb) * 2) * 64];
      wl[cb] = wb[((ls * NB + c0 + cb) * 2 + 1) * 64];
    }
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[c0 + cb] = mm(wh[cb], bh, acc[c0 + cb]);
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[c0 + cb] = mm(wh[cb], bl, acc[c0 + cb]);
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[c0 + cb] = mm(wl[cb], bh, acc[c0 + cb]);
    asm volatile("" ::: "memory");
  }
}
constexpr int kAp128Waves = 4, kAp128ChunkU = 2048, kAp128Chunks = 16;   // chunk: 2048 16-byte units
constexpr int kAp128Npc = kAp128ChunkU / (64 * kAp128Waves);             // 16-byte pieces per thread and chunk
// the weight ring of the d = 128 stream kernels: chunk kk of the image behind r is fetched into registers (buffer loads: one
// lane-offset register, the chunk offset scalar) ahead of its use, then committed to slot k & 1 with the one barrier per chunk
__device__ __forceinline__ void ring128_fetch(f32x4 (&stg)[kAp128Npc], __amdgpu_buffer_rsrc_t r, int kk, int tid) {
#pragma unroll
  for (int u = 0; u < kAp128Npc; u++)
    stg[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, tid * 16, (kk * kAp128ChunkU + u * 64 * kAp128Waves) * 16, 0));
  asm volatile("" ::: "memory");   // (issued here, ahead of the chunk's MFMAs; they land at the commit)
}
__device__ __forceinline__ void ring128_commit(f32x4 *s_ring, const f32x4 (&stg)[kAp128Npc], int k, int tid) {
  f32x4 *dst = s_ring + (k & 1) * kAp128ChunkU + tid;
#pragma unroll
  for (int u = 0; u < kAp128Npc; u++) dst[u * 64 * kAp128Waves] = stg[u];
  __syncthreads();
}
constexpr size_t kAp128Lds = (size_t)2 * kAp128ChunkU * 16 + (640 + 4 * 128 + kAp128Waves * 128) * sizeof(float);
template <int NH>
__global__ __launch_bounds__(64 * kAp128Waves) __attribute__((amdgpu_waves_per_eu(1, 1)))
void attn_apply_stream128_kernel(AttnArgs a) {
  constexpr int D = 128, ND = 4, SD = 8, GPH = 8 / NH;   // d_model, its 32-channel blocks, 16-channel steps; steps per head
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  f32x4 *s_ring = reinterpret_cast<f32x4 *>(smem);                    // [2 slots][2048 units]
  // (the constants lie past 64 KB, beyond a ds_read's 16-bit offset field: with the offset a compile-time constant every
  // read there got an address register of its own, hoisted out of the item loop -- 300 spilled registers.  Laundered, it
  // is one base register plus immediate offsets.)
  int coff = 2 * kAp128ChunkU * 4;
  asm volatile("" : "+s"(coff));
  float *s_c = smem + coff;                                           // bq | ln1 g | ln1 b | ln2 g | ln2 b : 5 x 128
  f32x4 *s_p0 = reinterpret_cast<f32x4 *>(s_c + 640);                 // [128] {w0x, w0y, w0z, b0}
  float *s_ks = s_c + 640 + 4 * 128;                                  // [waves][128] key sums of the wave's current cloud
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the weight stream: chunks 0-3 Wq (steps 4k .. 4k + 3), 4-11 FFN0 (steps 2 (k - 4) ..), 12-15 FFN1 (steps 4 (k - 12) ..);
  // buffer loads (64-bit addresses per chunk and piece were hoisted out of the item loop and spilled)
  const __amdgpu_buffer_rsrc_t rwq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq), 0, 4 * kAp128ChunkU * 16, 0x00020000),
                               rw0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wmlp0), 0, 8 * kAp128ChunkU * 16, 0x00020000),
                               rw2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wmlp2), 0, 4 * kAp128ChunkU * 16, 0x00020000);
  f32x4 stg[kAp128Npc];
  auto fetch = [&](int k) __attribute__((always_inline)) {
    k %= kAp128Chunks;
    ring128_fetch(stg, k < 4 ? rwq : (k < 12 ? rw0 : rw2), k < 4 ? k : (k < 12 ? k - 4 : k - 12), tid);
  };
  auto commit = [&](int k) __attribute__((always_inline)) { ring128_commit(s_ring, stg, k, tid); };
  for (int e = tid; e < D; e += 64 * kAp128Waves) {
    s_c[e] = p.bq[e];
    s_c[128 + e] = p.ln1_g[e];
    s_c[256 + e] = p.ln1_b[e];
    s_c[384 + e] = p.ln2_g[e];
    s_c[512 + e] = p.ln2_b[e];
    s_p0[e] = f32x4{p.pos0_w[3 * e], p.pos0_w[3 * e + 1], p.pos0_w[3 * e + 2], p.pos0_b[e]};
  }
  fetch(0);
  commit(0);
  const int nblk = p.Lq >> 5;
  const long nitem = (long)p.B * nblk;
  const float skf = (float)p.Sk;
  float *ksw = s_ks + wave * 128;
  auto cvec = [&](const float *base, int cb, int g) __attribute__((always_inline)) {
    return *reinterpret_cast<const f32x4 *>(base + 32 * cb + 8 * g + 4 * h);
  };
  auto to_ops = [&](const f32x16 &acc, int G, bf16x8 &oh, bf16x8 &ol) __attribute__((always_inline)) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = acc[8 * G + e];
    bf_split8(v, oh, ol, true);
  };
  // LayerNorm over the 128 channels of a token (two passes, eps inside the sqrt: tile_layernorm's arithmetic)
  auto layernorm = [&](f32x16 (&v)[ND], const float *gam, const float *bet) __attribute__((always_inline)) {
    float sm = 0.f;
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) sm += v[cb][r];
    sm += __shfl_xor(sm, 32, 64);
    const float mean = sm / (float)D;
    float vr = 0.f;
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float dlt = v[cb][r] - mean;
        vr += dlt * dlt;
      }
    vr += __shfl_xor(vr, 32, 64);
    const float inv = 1.0f / sqrtf(vr / (float)D + 1e-5f);
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const f32x4 gv = cvec(gam, cb, g), bv = cvec(bet, cb, g);
#pragma unroll
        for (int qq = 0; qq < 4; qq++) v[cb][4 * g + qq] = (v[cb][4 * g + qq] - mean) * inv * gv[qq] + bv[qq];
      }
  };
  // rounds of kAp128Waves items (cloud, block), one per wave; every wave of the workgroup takes part in every round (the
  // ring's barriers), a wave past the last item runs the last item again and stores nothing
  for (long it0 = (long)blockIdx.x * kAp128Waves; it0 < nitem; it0 += (long)gridDim.x * kAp128Waves) {
    const long item = it0 + wave;
    const bool live = item < nitem;
    const long it = live ? item : nitem - 1;
    const long b = it / nblk;
    const int blk = (int)(it - b * nblk);
    const size_t bq_ = p.q_index ? (size_t)p.q_index[b] : (size_t)b;
    const size_t kb_ = p.kv_index ? (size_t)p.kv_index[b] : (size_t)b;
    const float *kvp = p.kv + kb_ * ((size_t)D * D + D);
    const int t = blk * 32 + j;
    const __amdgpu_buffer_rsrc_t rfeat = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.feat_q + bq_ * D * p.Lq), 0, D * p.Lq * 4, 0x00020000);
    const int vo = (4 * h * p.Lq + t) * 4;
    // lane (t, h): element e of its 64 feature values is channel 16 (e >> 3) + bf_kpos(h, e & 7) -- B-operand order of the
    // eight x steps, and the order of the final accumulators (residual, store)
    auto load_x = [&](float (&xf)[64]) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 64; e++) {
        const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);   // + 4 h: in the lane offset
        xf[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rfeat, vo, ch * p.Lq * 4, 0));
      }
    };
    ksw[lane] = kvp[(size_t)D * D + lane];
    ksw[64 + lane] = kvp[(size_t)D * D + 64 + lane];
    // B operands: steps 0-7 x (kept through FFN0, whose input starts with the same x), 8-15 the position hidden layer
    // (Q) / the message (FFN0)
    bf16x8 bh[16], bl[16];
    {
      float xf[64];
      load_x(xf);
      const float *xyz = p.xyz_q + (bq_ * p.Lq + t) * 3;
      const float px = xyz[0], py = xyz[1], pz = xyz[2];
#pragma unroll
      for (int s2 = 0; s2 < SD; s2++) {
        float hv[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const f32x4 w = s_p0[16 * s2 + bf_kpos(0, e) + 4 * h];
          const float v = w[0] * px + w[1] * py + w[2] * pz + w[3];
          hv[e] = relu_i(v);
        }
        bf_split8(hv, bh[SD + s2], bl[SD + s2], true);
      }
#pragma unroll
      for (int e = 0; e < 64; e++) asm volatile("" : "+v"(xf[e]));   // (the loads land here: see attn_kv_stream64_kernel)
#pragma unroll
      for (int s2 = 0; s2 < SD; s2++) {
        float xv[8];
#pragma unroll
        for (int e = 0; e < 8; e++) xv[e] = xf[8 * s2 + e];
        bf_split8(xv, bh[s2], bl[s2], true);
      }
    }
    // ---- Q = elu(Wq [x ; h] + bq) + 1: chunks 0-3 (the bias seeds the accumulators, as in the tile kernel)
    f32x16 q[ND];
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const f32x4 bqv = cvec(s_c, cb, g);
#pragma unroll
        for (int qq = 0; qq < 4; qq++) q[cb][4 * g + qq] = bqv[qq];
      }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      fetch(k + 1);
      const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(s_ring + (k & 1) * kAp128ChunkU) + lane;
#pragma unroll
      for (int ls = 0; ls < 4; ls++) ap128_step<ND>(q, wb, ls, bh[4 * k + ls], bl[4 * k + ls]);
      commit(k + 1);
    }
    // z[head][token] = Q_head . ksum_head: partial sums per 16-channel group gi = 2 cb + G, then per head (GPH groups), then
    // over the partner lane.  (The key-sum strip was written before the ring's barriers.)
    float zg[SD];
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const f32x4 ksv = cvec(ksw, cb, g);
        float zz = 0.f;
#pragma unroll
        for (int qq = 0; qq < 4; qq++) {
          const float v = elu1(q[cb][4 * g + qq]);
          q[cb][4 * g + qq] = v;
          zz += v * ksv[qq];
        }
        if ((g & 1) == 0) zg[2 * cb + (g >> 1)] = zz;
        else zg[2 * cb + (g >> 1)] += zz;
      }
    float zs[NH];
#pragma unroll
    for (int hd = 0; hd < NH; hd++) {
      float z = zg[hd * GPH];
#pragma unroll
      for (int gi = 1; gi < GPH; gi++) z += zg[hd * GPH + gi];
      z += __shfl_xor(z, 32, 64);
      zs[hd] = (1.0f / (z + 1e-6f)) * skf;
    }
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) q[cb][r] *= zs[(2 * cb + (r >> 3)) / GPH];
    // ---- message = M Q' (M: the cloud's bf16 image [8 steps][4 cout blocks][hi, lo][64], read from global memory / L2
    // one step ahead of its MFMAs), written over the hidden layer's operands
    {
      bf16x8 ch_[SD], cl_[SD];
#pragma unroll
      for (int cb = 0; cb < ND; cb++)
#pragma unroll
        for (int G = 0; G < 2; G++) to_ops(q[cb], G, ch_[2 * cb + G], cl_[2 * cb + G]);
#pragma unroll
      for (int cb = 0; cb < ND; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) q[cb][r] = 0.f;   // (q becomes the message accumulator)
      const bf16x8 *mb = reinterpret_cast<const bf16x8 *>(kvp) + lane;
      bf16x8 mh[2][ND], ml[2][ND];
#pragma unroll
      for (int cb = 0; cb < ND; cb++) {
        mh[0][cb] = mb[(cb * 2) * 64];
        ml[0][cb] = mb[(cb * 2 + 1) * 64];
      }
#pragma unroll
      for (int s2 = 0; s2 < SD; s2++) {
        const int c = s2 & 1;
        if (s2 + 1 < SD) {
#pragma unroll
          for (int cb = 0; cb < ND; cb++) {
            mh[c ^ 1][cb] = mb[(((s2 + 1) * ND + cb) * 2) * 64];
            ml[c ^ 1][cb] = mb[(((s2 + 1) * ND + cb) * 2 + 1) * 64];
          }
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int cb = 0; cb < ND; cb++) q[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mh[c][cb], ch_[s2], q[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < ND; cb++) q[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mh[c][cb], cl_[s2], q[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < ND; cb++) q[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ml[c][cb], ch_[s2], q[cb], 0, 0, 0);
      }
    }
    layernorm(q, s_c + 128, s_c + 256);
    // ---- FFN0: relu(W0 [x ; msg]) (256 couts): chunks 4-11
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int G = 0; G < 2; G++) to_ops(q[cb], G, bh[SD + 2 * cb + G], bl[SD + 2 * cb + G]);
    f32x16 f[2 * ND];
#pragma unroll
    for (int cb = 0; cb < 2 * ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) f[cb][r] = 0.f;
#pragma unroll
    for (int k = 4; k < 12; k++) {
      fetch(k + 1);
      const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(s_ring + (k & 1) * kAp128ChunkU) + lane;
#pragma unroll
      for (int ls = 0; ls < 2; ls++) ap128_step<2 * ND>(f, wb, ls, bh[2 * (k - 4) + ls], bl[2 * (k - 4) + ls]);
      commit(k + 1);
    }
    // the residual's features, re-read (L2) under FFN1
    float xf[64];
    load_x(xf);
    // ---- FFN1 (128 couts): chunks 12-15 (the last one's fetch is the next block's chunk 0); chunk k takes the hidden
    // channels of FFN0 blocks 2 (k - 12), 2 (k - 12) + 1, converted when it starts
    f32x16 o[ND];
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) o[cb][r] = 0.f;
#pragma unroll
    for (int k = 12; k < 16; k++) {
      fetch(k + 1);
      bf16x8 oh[4], ol[4];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        f32x16 &fc = f[2 * (k - 12) + i];
#pragma unroll
        for (int r = 0; r < 16; r++) fc[r] = relu_i(fc[r]);
#pragma unroll
        for (int G = 0; G < 2; G++) to_ops(fc, G, oh[2 * i + G], ol[2 * i + G]);
      }
      const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(s_ring + (k & 1) * kAp128ChunkU) + lane;
#pragma unroll
      for (int ls = 0; ls < 4; ls++) ap128_step<ND>(o, wb, ls, oh[ls], ol[ls]);
      commit(k + 1);
    }
    layernorm(o, s_c + 384, s_c + 512);
#pragma unroll
    for (int cb = 0; cb < ND; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) o[cb][r] += xf[16 * cb + r];
    if (live) {
      const __amdgpu_buffer_rsrc_t rout =
          __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)b * D * p.Lq, 0, D * p.Lq * 4, 0x00020000);
#pragma unroll
      for (int e = 0; e < 16 * ND; e++) {
        const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);
        const float v = o[e >> 4][e & 15];   // (a copy: __builtin_bit_cast of a vector ELEMENT reads element 0)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, vo, ch * p.Lq * 4, 0);
      }
    }
  }
}

// ---- the kv half at d = c2 = 128 (SA3's self-attention, key sets of >= 256 tokens): attn_kv_stream64_kernel's form with
// attn_apply_stream128_kernel's weight ring.  A wave owns a 32-token block from the feature load to its KV MFMAs: lane
// (t, h) holds the 128 feature and 128 position-hidden channels of token t in the K order of the bf16 image (16 steps,
// 128 registers as hi / lo operands), the fused K / V projection runs TRANSPOSED (Y^T = [x ; h]^T W^T, all eight cout blocks
// at once: 128 accumulator registers) so that after elu + 1 / the 1 / Sk scale its accumulators are the operands of
// KV += K V^T as they stand (f32, same-head 32 x 32 tiles only, accumulated transposed as in the ONEW form: lane = dd,
// register r <-> v).  The 256 KB image wkv_bf streams as 8 chunks of 32 KB (two steps x eight cout blocks, 48 MFMAs per
// wave) through the two-slot ring; the stream is the same for every block, so the last chunk's fetch is the next block's
// first.  The next block's features are requested right after the last chunk's barrier (vector loads retire in order:
// before it, the ring's wait would sit out their HBM round trip) and land under the KV MFMAs.
// A cloud takes wpc = 1 / 2 / 4 waves of a workgroup (attn_kv128_wpc: Sk only); with wpc > 1 its waves add their KV tiles and
// key sums through LDS in wave order, then every wave holds the same sums and folds its share of the output blocks.  The
// merge fold M[o][dd] = sum_{v in head(dd)} Wm[o][v] KV[dd][v] takes the KV tile registers as the A operand and the f32
// merge rows from L2 as B (lane (o, h) then holds the 16-byte units of the bf16 image of M), then the key sums follow:
// the image attn_kv_fold_mfma writes in this unit.  One wave per SIMD (four per workgroup, one workgroup per CU).
// NH: heads (2, 4); nhead = 1 needs 16 KV tiles (256 registers) and stays on the tile kernel.
__host__ __device__ constexpr int attn_kv128_wpc(int nblk) { return nblk >= 32 ? 4 : (nblk >= 16 ? 2 : 1); }
constexpr size_t kKv128Lds0 = (size_t)2 * kAp128ChunkU * 16 + 128 * 16 + 256 * 4;   // ring + position MLP + biases
template <int NH>
__global__ __launch_bounds__(64 * kAp128Waves) __attribute__((amdgpu_waves_per_eu(1, 1)))
void attn_kv_stream128_kernel(AttnArgs a) {
  constexpr int D = 128, SD = 8, TPH = 4 / NH, NKV = NH * TPH * TPH;   // steps of x / of h; 32-blocks per head; KV tiles
  constexpr int KVU = NKV * 16 + 4;                                     // reduction floats per lane: KV tiles + key sums
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const pcr_attn_params &p = a.p;
  f32x4 *s_ring = reinterpret_cast<f32x4 *>(smem);                    // [2 slots][2048 units]
  int coff = 2 * kAp128ChunkU * 4;                                     // (past 64 KB: laundered, see the apply kernel)
  asm volatile("" : "+s"(coff));
  f32x4 *s_p0 = reinterpret_cast<f32x4 *>(smem + coff);                // [128] {w0x, w0y, w0z, b0}
  float *s_bkv = smem + coff + 4 * D;                                  // [256] K / V biases
  float *s_red = s_bkv + 2 * D;                                        // [clouds per round][KVU][64] (wpc > 1)
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wkv_bf), 0, 8 * kAp128ChunkU * 16, 0x00020000);
  f32x4 stg[kAp128Npc];
  auto fetch = [&](int k) __attribute__((always_inline)) { ring128_fetch(stg, rw, k & 7, tid); };
  auto commit = [&](int k) __attribute__((always_inline)) { ring128_commit(s_ring, stg, k, tid); };
  for (int e = tid; e < D; e += 64 * kAp128Waves) s_p0[e] = f32x4{p.pos0_w[3 * e], p.pos0_w[3 * e + 1], p.pos0_w[3 * e + 2], p.pos0_b[e]};
  for (int e = tid; e < 2 * D; e += 64 * kAp128Waves) s_bkv[e] = p.bkv[e];
  fetch(0);
  commit(0);
  const int Sk = p.Sk, nblk = Sk >> 5;
  const int wpc = a.wpc, cpg = kAp128Waves / wpc;
  const int cslot = wave / wpc, wsub = wave - cslot * wpc;
  const int nper = (nblk + wpc - 1) / wpc;                            // block rounds per cloud: the same for every wave
  const long cstep = (long)gridDim.x * cpg;
  const float inv_sk = 1.0f / (float)Sk;
  // features (element e: channel 16 (e >> 3) + bf_kpos(h, e & 7)) and position of token t of block blk of cloud b
  float xf[64], pxyz[3];
  auto issue = [&](long bq, int blk) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t rfeat =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.feat_k + (size_t)bq * D * Sk), 0, D * Sk * 4, 0x00020000);
    const int t = blk * 32 + j, vo = (4 * h * Sk + t) * 4;
#pragma unroll
    for (int e = 0; e < 64; e++) {
      const int ch = 16 * (e >> 3) + bf_kpos(0, e & 7);   // + 4 h: in the lane offset
      xf[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rfeat, vo, ch * Sk * 4, 0));
    }
    const __amdgpu_buffer_rsrc_t rxyz =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.xyz_k + (size_t)bq * Sk * 3), 0, Sk * 12, 0x00020000);
#pragma unroll
    for (int c = 0; c < 3; c++) pxyz[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rxyz, t * 12, c * 4, 0));
    asm volatile("" ::: "memory");
  };
  if ((long)blockIdx.x * cpg + cslot < p.B && wsub < nblk) issue((long)blockIdx.x * cpg + cslot, wsub);
  // rounds of cpg clouds per workgroup; every wave takes part in every ring barrier (a wave without a block in a round
  // fetches and commits and skips the MFMAs)
  for (long c0 = (long)blockIdx.x * cpg; c0 < p.B; c0 += cstep) {
    const long b = c0 + cslot;
    const bool live = b < p.B;
    f32x16 kv[NKV];
#pragma unroll
    for (int i = 0; i < NKV; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) kv[i][r] = 0.f;
    float ks[4] = {0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < nper; it++) {
      const int blk = wsub + it * wpc;
      const bool has = live && blk < nblk;
      const bool last = it + 1 == nper;
      const long bn = last ? b + cstep : b;                           // this wave's next block
      const int blkn = last ? wsub : blk + wpc;
      const bool hasn = bn < p.B && blkn < nblk;
      // A operands: steps 0-7 the features, converted here; steps 8-15 the position-hidden channels 16 s2 + bf_kpos(h, .),
      // computed by the chunk that takes them (all sixteen steps at once are 128 registers: spilled)
      bf16x8 bh[SD], bl[SD];
      if (has) {
#pragma unroll
        for (int s2 = 0; s2 < SD; s2++) {
          float xv[8];
#pragma unroll
          for (int e = 0; e < 8; e++) xv[e] = xf[8 * s2 + e];
          bf_split8(xv, bh[s2], bl[s2], true);
        }
      }
      f32x16 acc[8];
#pragma unroll
      for (int cb = 0; cb < 8; cb++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[cb][r] = 0.f;   // (the bias joins in the epilogue)
#pragma unroll
      for (int k = 0; k < 8; k++) {
        fetch(k + 1);
        if (has) {
          const bf16x8 *wb = reinterpret_cast<const bf16x8 *>(s_ring + (k & 1) * kAp128ChunkU) + lane;
#pragma unroll
          for (int ls = 0; ls < 2; ls++) {
            if (k < 4) {
              ap128_step<8, true>(acc, wb, ls, bh[2 * k + ls], bl[2 * k + ls]);
            } else {
              const int s2 = 2 * k + ls - SD;
              float hv[8];
#pragma unroll
              for (int e = 0; e < 8; e++) {
                const f32x4 w = s_p0[16 * s2 + bf_kpos(0, e) + 4 * h];
                const float v = w[0] * pxyz[0] + w[1] * pxyz[1] + w[2] * pxyz[2] + w[3];
                hv[e] = relu_i(v);
              }
              bf16x8 hh, hl;
              bf_split8(hv, hh, hl, true);
              ap128_step<8, true>(acc, wb, ls, hh, hl);
            }
          }
        }
        commit(k + 1);
      }
      if (hasn) issue(bn, blkn);
      else {
#pragma unroll
        for (int e = 0; e < 64; e++) xf[e] = 0.f;   // (defined on both paths: not live through the chunks)
        pxyz[0] = pxyz[1] = pxyz[2] = 0.f;
      }
      if (has) {
        float bias[8];   // (from LDS here: eight registers through the chunks were what spilled)
#pragma unroll
        for (int cb = 0; cb < 8; cb++) bias[cb] = s_bkv[cb * 32 + j];
#pragma unroll
        for (int r = 0; r < 16; r++) {
#pragma unroll
          for (int cb = 0; cb < 4; cb++) {
            acc[cb][r] = elu1(acc[cb][r] + bias[cb]);
            ks[cb] += acc[cb][r];
            acc[4 + cb][r] = (acc[4 + cb][r] + bias[4 + cb]) * inv_sk;
          }
        }
        // KV^T tile (v block jb, dd block ib): lane (dd, h), register r <-> v = 32 jb + 8 g + 4 h + q
#pragma unroll
        for (int i = 0; i < NKV; i++) {
          const int hd = i / (TPH * TPH), ib = hd * TPH + (i % (TPH * TPH)) / TPH, jb = hd * TPH + i % TPH;
#pragma unroll
          for (int r = 0; r < 16; r++) kv[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[4 + jb][r], acc[ib][r], kv[i], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int cb = 0; cb < 4; cb++) ks[cb] += __shfl_xor(ks[cb], 32, 64);
    if (wpc > 1) {
      // the cloud's waves add their tiles and key sums in wave order (lane-major: conflict-free, no layout change), then
      // all of them read the sums back
      int ln = lane;
      asm volatile("" : "+v"(ln));   // (the lane offsets of the cold phases are computed where used: hoisted, they spilled)
      float *red = s_red + (size_t)cslot * KVU * 64 + ln;
      for (int round = 0; round < wpc; round++) {
        if (wsub == round) {
#pragma unroll
          for (int i = 0; i < NKV; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
              float *dst = red + (i * 16 + r) * 64;
              *dst = round == 0 ? kv[i][r] : *dst + kv[i][r];
            }
#pragma unroll
          for (int cb = 0; cb < 4; cb++) {
            float *dst = red + (NKV * 16 + cb) * 64;
            *dst = round == 0 ? ks[cb] : *dst + ks[cb];
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < NKV; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) kv[i][r] = red[(i * 16 + r) * 64];
#pragma unroll
      for (int cb = 0; cb < 4; cb++) ks[cb] = red[(NKV * 16 + cb) * 64];
      // (the next round writes these areas after at least eight ring barriers)
    }
    if (live) {
      // (buffer loads / stores throughout: 64-bit lane addresses were what spilled)
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int j = ln & 31, h = ln >> 5;
      const __amdgpu_buffer_rsrc_t rkv =
          __builtin_amdgcn_make_buffer_rsrc(p.kv + (size_t)b * ((size_t)D * D + D), 0, (D * D + D) * 4, 0x00020000);
      const __amdgpu_buffer_rsrc_t rwm = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wmerge), 0, D * D * 4, 0x00020000);
      for (int ob = wsub; ob < 4; ob += wpc) {
        const int wrow = ((ob * 32 + j) * D + 4 * h) * 4;
#pragma unroll
        for (int hd = 0; hd < NH; hd++) {
          f32x4 w[TPH][4];   // Wm[o][32 jb + 8 g + 4 h + q] of the head's v blocks
#pragma unroll
          for (int jj = 0; jj < TPH; jj++)
#pragma unroll
            for (int g = 0; g < 4; g++)
              w[jj][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rwm, wrow, ((hd * TPH + jj) * 32 + 8 * g) * 4, 0));
#pragma unroll
          for (int dl = 0; dl < TPH; dl++) {
            const int db = hd * TPH + dl;
            f32x16 m;
#pragma unroll
            for (int r = 0; r < 16; r++) m[r] = 0.f;
#pragma unroll
            for (int jj = 0; jj < TPH; jj++) {
              const int i = hd * TPH * TPH + dl * TPH + jj;
#pragma unroll
              for (int r = 0; r < 16; r++) m = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[i][r], w[jj][r >> 2][r & 3], m, 0, 0, 0);
            }
#pragma unroll
            for (int G = 0; G < 2; G++) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = m[8 * G + e];
              bf16x8 hi, lo;
              bf_split8(v, hi, lo, true);
              const int unit = (((db * 2 + G) * (D >> 5) + ob) * 2) * 64 + h * 32 + j;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi), rkv, unit * 16, 0, 0);
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo), rkv, (unit + 64) * 16, 0, 0);
            }
          }
        }
      }
      if (wsub == 0 && h == 0) {
#pragma unroll
        for (int cb = 0; cb < 4; cb++)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ks[cb]), rkv, (D * D + cb * 32 + j) * 4, 0, 0);
      }
    }
  }
}
#endif

}  // namespace

static int attn_check(const pcr_attn_params &p) {
  if (p.B < 0 || p.Lq < 1 || p.Sk < 1 || p.c1 < 1 || p.c2 < 1 || p.cout < 1 || p.nhead < 1) return 1;
  if (p.d < 32 || p.d > 512 || (p.d & 31) || p.d % p.nhead) return 1;  // d_model in {32,64,96,128} or wide (below)
  if (p.d > 128 && ((p.d & 63) || ((p.d / p.nhead) & 63) || p.d / p.nhead > 256)) return 1;   // wide: heads of 64 n <= 256
  if ((p.c2 & 7) || p.cout > 512 || p.cfinal > 512) return 1;
  if (!p.feat_q || !p.feat_k || !p.xyz_k || !p.kv || !p.pos0_w || !p.pos0_b || !p.wq || !p.bq || !p.wkv ||
      !p.bkv || !p.wmerge || !p.wmlp0 || !p.wmlp2 || !p.ln1_g || !p.ln1_b || !p.ln2_g || !p.ln2_b)
    return 1;
  if (p.q_pos && (!p.xyz_q || p.c1 != p.c2 || p.c1 != p.d)) return 1;
  if (p.residual && p.cout != p.c1) return 1;
  if (p.cfinal && (!p.wfinal || !p.bfinal || (p.cout & 7))) return 1;
  return 0;
}

static void attn_dump_trace(const char *path, const char *tag, int wgs, int B, int Sk) {
  wave_trace_dump<AttnTrace>(path, HIP_SYMBOL(g_attn_trace), 2 * wgs, "kernel %s wgs %d B %d Sk %d\n", tag, wgs, B,
                             Sk);
}

// ---- the dispatch, compiled once per arithmetic unit.  attn_plan_kv / attn_plan_apply are the single statement of what a
// unit decides for a launch -- kernel family, template arguments, everything shape-derived the launch needs -- and touch
// neither the device nor the chip's size; one launcher per family turns a plan into the launch.  The f32 unit also holds the
// order of the units (attn_bf), the gate, the exported queries and the C-ABI entry points.

// tuning builds' knobs (0 / null in production builds: pcr_common.h), gathered once per process and unit.  One more,
// PCR_ATTN_KV_FULL (attn_kv_stream64_kernel runs the full form whatever the weights hold), is read per launch: attn_unit.
struct AttnTune {
  int no_onew;         // PCR_ATTN_NO_ONEW: short key sets keep several waves per cloud
  int no_kv128;        // PCR_ATTN_NO_KV128: the d = 128 stream kv shapes back to the tile kernel
  int kv128_wpc;       // PCR_ATTN_KV128_WPC: 1 / 2 / 4 waves per cloud of attn_kv_stream128_kernel whatever Sk says
  int no_stream128;    // PCR_ATTN_NO_STREAM128: the d = 128 stream apply shapes back to the tile kernel
  const char *trace;   // PCR_ATTN_TRACE: file the d = 64 stream kernels' stamps are appended to
};
static const AttnTune &attn_tune() {
  static const AttnTune once = {pcr_tune_int("PCR_ATTN_NO_ONEW"), pcr_tune_int("PCR_ATTN_NO_KV128"), pcr_tune_int("PCR_ATTN_KV128_WPC"),
                                pcr_tune_int("PCR_ATTN_NO_STREAM128"), pcr_tune_str("PCR_ATTN_TRACE")};
  return once;
}

// What one launch does.  arith / family / targ / gated / splits / fold / wpc / lds are pcr_attn_launch_form's encoding
// (pcr.h); the rest is what the launchers read besides the parameter block.
struct AttnPlan {
  int arith = -1;               // PCR_PREC_* the launch notes: set as soon as the unit knows it (a later refusal still notes it)
  int family = 0;               // PCR_ATTN_*
  int ntarg = 0, targ[6] = {};  // the kernel's template arguments in the kernel's order, defaults filled in, GATE left out
  bool gated = false;           // the gated twin (GATE = true, attn_kv_kernel_o3_live) is taken
  bool trace = false;           // the kernel stamps the shader clock (AttnArgs.dbg = 256)
  int threads = 0;              // per workgroup
  size_t lds = 0;               // dynamic LDS of the main kernel
  // the grid without the chip: (gx, gy) as it stands, or persistent -- `work` workgroups of work, at most per_cu per CU
  bool persistent = false;
  unsigned gx = 1, gy = 1;
  long work = 0;
  int per_cu = 0;
  // kv side
  int splits = 1;               // effective token split (AttnArgs.p.kv_splits of the narrow families)
  bool fold = false;            // attn_kv_fold_kernel follows, one workgroup per cloud, fold_lds bytes
  size_t fold_lds = 0;
  int wpc = 0;                  // attn_kv_stream128_kernel: waves per cloud (AttnArgs.wpc)
};

// the plan's last step: the form, refused where a gated launch meets a family (or instantiation) without a gated twin
static int attn_plan_form(AttnPlan *pl, int family, std::initializer_list<int> targ, bool twin, bool gated) {
  pl->family = family;
  pl->ntarg = 0;
  for (int v : targ) pl->targ[pl->ntarg++] = v;
  if (gated && !twin) return PCR_ERR_INVALID;
  pl->gated = gated;
  return PCR_OK;
}
// a persistent grid: `items` units of work, per_wg of them a workgroup round
static void attn_plan_persistent(AttnPlan *pl, long items, int per_wg, int per_cu, int threads, size_t lds) {
  pl->persistent = true;
  pl->work = (items + per_wg - 1) / per_wg;
  pl->per_cu = per_cu;
  pl->threads = threads;
  pl->lds = lds;
}
static void attn_plan_grid(AttnPlan *pl, unsigned gx, unsigned gy, size_t lds) {
  pl->gx = gx;
  pl->gy = gy;
  pl->threads = kThreads;
  pl->lds = lds;
}
// waves a cloud of nblk 32-token blocks takes in the stream kv kernels: the largest power of two within min(nblk, cap),
// at least minw (the kernels' comments)
static int attn_waves_per_cloud(int nblk, int cap, int minw) {
  int w = 1;
  while (w * 2 <= (nblk < cap ? nblk : cap)) w *= 2;
  return w < minw ? minw : w;
}

// the blocks a gated launch covers: the matching stages' (d = c1 = c2 = cout = 64, whole launches).  Shape only.  Every
// kernel the plans choose for them has a gated twin (tests/test_attn_ref_cpu.py enumerates them), so attn_plan_form's
// refusal is never met behind this predicate.
static bool attn_live_shape(const pcr_attn_params &p) {
  return p.d == 64 && p.c1 == 64 && p.c2 == 64 && p.cout == 64 && p.kv_splits <= 1;
}

// The kv launch of one unit (wq / wkv / ... are images of THIS unit's kind).  d_model <= 128: one workgroup per key-side
// cloud and token split (tile families) or persistent wave-autonomous workgroups (stream families); wider: d / 64
// workgroups per cloud (f32 unit only).
static int attn_plan_kv(const pcr_attn_params &p, bool gated, const AttnTune &t, AttnPlan *pl) {
  constexpr bool kBfUnit = kAPrec != 0;
  const int d = p.d;
  if (d > 128) {
    if (kBfUnit || !p.wkv_wide || !p.bkv_wide || !p.wmerge_packed || p.B > 65535) return PCR_ERR_INVALID;
    pl->arith = PCR_PREC_F32;
    const int dh = d / p.nhead;
    size_t lds = ((size_t)(p.c2 + d + 3) * 33 + 4 * d + kThreads) * sizeof(float);
    const size_t lds2 = (size_t)dh * 65 * sizeof(float);
    if (lds2 > lds) lds = lds2;
    if (lds > (size_t)kMaxDynLds) return PCR_ERR_INVALID;
    attn_plan_grid(pl, d / 64, p.B, lds);
    return attn_plan_form(pl, PCR_ATTN_KV_WIDE, {64 + dh <= 256 ? 2 : 3}, false, gated);
  }
  if (p.c2 < d) return PCR_ERR_INVALID;   // the in-place K/V projection needs 2d <= c2 + d rows
  // RULE: the tile kernel's LDS and the token split are judged first, whichever family then takes the launch -- a block the
  // tile kernel could not hold, or a split without its workspace, is refused even where a stream form would run it
  const int tb = d <= 64 ? 2 : 1, RP = 32 * tb + 1;
  size_t lds = (size_t)(p.c2 + d + 3) * RP + 4 * d;
  const size_t lds2 = (size_t)d * (d + 1) + d;
  if (lds2 > lds) lds = lds2;
  lds = (lds + kThreads) * sizeof(float);
  if (lds > (size_t)kMaxDynLds) return PCR_ERR_INVALID;
  const int ntile = (p.Sk + 32 * tb - 1) / (32 * tb);
  int ns = p.kv_splits > 1 ? p.kv_splits : 1;
  if (ns > 1 && (!p.kv_part || ns > 64)) return PCR_ERR_INVALID;
  if (ns > ntile) ns = ntile;                 // (kv_part is sized for the requested count: fewer splits use its head)
  pl->splits = ns;
  // the stream families take whole clouds of whole 32-token blocks (shape-only choices; an explicit token split keeps the
  // tile kernel); bfk: this unit projects in split bf16 from the wkv_bf image
  const bool whole = ns == 1 && (p.Sk & 31) == 0, bfk = kBfUnit && p.wkv_bf != nullptr;
  const int nblk = p.Sk >> 5;
  if (whole && d == 64 && (p.c2 == 64 || (p.c2 == 128 && bfk && p.Sk >= 128)) && 64 % p.nhead == 0) {
    // c2 = 128 (XS = 8): not a matching-stage block, no gated twin.  ONEW: short key sets, one wave per cloud (the bf16
    // unit's image only).  At most four waves per cloud.
    const bool wide = p.c2 == 128, onew = bfk && !wide && nblk <= 4 && !t.no_onew;
    pl->arith = bfk ? PCR_PREC_BF16X3 : PCR_PREC_F32;   // (the projection; the KV accumulation and the fold are f32)
    const int cpg = kKvsWaves / (onew ? 1 : attn_waves_per_cloud(nblk, 4, wide ? 4 : 2));
    const size_t wu = bfk ? (size_t)((wide ? 8 : 4) + 4) * 512 : 4096;
    const size_t lds_s = (wu * 4 + 256 + 128 + 64 * 65 + (onew ? (size_t)0 : (size_t)cpg * (64 * 65 + 64))) * sizeof(float);
    attn_plan_persistent(pl, p.B, cpg, 1, 64 * kKvsWaves, lds_s);
    pl->trace = bfk && !wide && t.trace != nullptr;
    return attn_plan_form(pl, PCR_ATTN_KV_STREAM64, {p.nhead >= 2, bfk, wide ? 8 : 4, onew}, !wide, gated);
  }
#if PCR_ATTN_PREC != 0
  if (whole && d == 32 && p.c2 == 32 && p.wkv_bf && 32 % p.nhead == 0) {
    pl->arith = PCR_PREC_BF16X3;
    const int cpg = kKvsWaves / attn_waves_per_cloud(nblk, kKvsWaves, 2);
    const size_t lds_s = (size_t)(4096 + 128 + 64 + 32 * 33 + cpg * (32 * 33 + 32)) * sizeof(float);
    attn_plan_persistent(pl, p.B, cpg, 2, 64 * kKvsWaves, lds_s);        // (small footprint: two workgroups per CU)
    return attn_plan_form(pl, PCR_ATTN_KV_STREAM32, {}, false, gated);
  }
  if (whole && d == 128 && p.c2 == 128 && p.wkv_bf && p.Sk >= 256 && (p.nhead == 2 || p.nhead == 4) && !t.no_kv128) {
    // SA3's self-attention (d_model 128): the wave-autonomous form with the weights streamed through an LDS ring (the
    // split-projection rule below: key sets of >= 256 tokens); one workgroup of four waves per CU
    pl->arith = PCR_PREC_BF16X3;   // (the projection; the KV accumulation and the fold are f32)
    pl->wpc = (t.kv128_wpc == 1 || t.kv128_wpc == 2 || t.kv128_wpc == 4) ? t.kv128_wpc : attn_kv128_wpc(nblk);
    const int cpg = kAp128Waves / pl->wpc;
    const size_t lds_s = kKv128Lds0 + (pl->wpc > 1 ? (size_t)cpg * (16 * (16 / p.nhead) + 4) * 64 * sizeof(float) : 0);
    attn_plan_persistent(pl, p.B, cpg, 1, 64 * kAp128Waves, lds_s);
    return attn_plan_form(pl, PCR_ATTN_KV_STREAM128, {p.nhead}, false, gated);
  }
#endif
  // the tile families project in f32 in both units (only the form of M differs)
  attn_plan_grid(pl, p.B, ns, lds);
  pl->fold = ns > 1;
  pl->fold_lds = ((size_t)d * (d + 1) + d) * sizeof(float);
  int rc;
  if (d == 32) rc = attn_plan_form(pl, PCR_ATTN_KV_TILE, {2, 1, 2, 1}, false, gated);            // 2d = 64: two cout blocks
  else if (d == 64) rc = attn_plan_form(pl, PCR_ATTN_KV_TILE_O3, {2, 1, 1, 1}, ns == 1, gated);   // four, one per wave
  else if (d == 128)
    // eight cout blocks, two rounds.  NOT the three-workgroups-per-CU form: this shape's fold buffer (d (d + 1) floats =
    // 66 KB) allows two workgroups per CU whatever the registers say, and held to a third of the register file the body
    // spilled 93 registers inside its tile loop for nothing (round 5, tools/kres.py)
    // (BFP, split-bf16 projection for key sets of >= 256 tokens -- a shape-only rule: the KV state is a mean over the key
    // tokens, so the projection's rounding averages out with their number; at Sk = 32 (the Point-Transformer @128) the
    // guard's sweep of tests/test_gpu_precision.py went from 4.5e-5 to 5.2e-5 with it, for 0.014 ms)
    rc = attn_plan_form(pl, PCR_ATTN_KV_TILE_O2, {1, 2, 1, 4, bfk && p.Sk >= 256}, false, gated);
  else rc = attn_plan_form(pl, PCR_ATTN_KV_TILE, {1, 2, 0, 4}, false, gated);                     // d = 96: generic shape
  if (rc == PCR_OK) pl->arith = PCR_PREC_F32;
  return rc;
}

// the d = 64 wave-autonomous apply form (attn_apply_stream64_kernel), shapes: (c1 = 64 | 32 | < 16 with the padded
// mlp[0] image) x (cout = 64 [+ cov_final 128] | cout = 128 | cout = 32 + cov_final 64)
static bool aps64_shape(const pcr_attn_params &p) {
  const bool aps_in = p.c1 == 64 || ((p.c1 == 32 || (p.c1 < 16 && p.wmlp0_bf_xpad)) && !p.q_pos && !p.residual);
  const bool aps_out = (p.cout == 64 && (p.cfinal == 0 || p.cfinal == 128) && p.c1 >= 32) ||
                       (p.cout == 128 && !p.cfinal && !p.residual && p.c1 == 64) ||
                       (p.cout == 32 && p.cfinal == 64 && !p.residual && p.c1 < 16);
  return p.d == 64 && aps_in && aps_out && (p.Lq & 31) == 0 && (p.nhead == 1 || p.nhead == 2 || p.nhead == 4);
}

// The apply launch of one unit: 32 tb-token tiles per workgroup (tile family) or persistent wave-autonomous workgroups over
// 32-token blocks (stream families, bf16 unit only).
static int attn_plan_apply(const pcr_attn_params &p, bool gated, const AttnTune &t, AttnPlan *pl) {
  (void)t;
  // (round 6, measured and dropped: 64-token tiles for d = 128 -- half the weight traffic from L2, half the waves per CU:
  // pt1024's attn_apply[d=128] 0.455 -> 0.518 ms, profiles/r06_inproc_ab.txt)
  const int tb = p.d <= 32 ? 4 : (p.d <= 64 ? 2 : 1), T = 32 * tb, RP = T + 1;
  const int catP = ceil8(p.c1 + p.d);
  int rowsU = catP > 2 * p.d ? catP : 2 * p.d;
  if (ceil32(p.cout) > rowsU) rowsU = ceil32(p.cout);
  if (ceil32(p.cfinal) > rowsU) rowsU = ceil32(p.cfinal);
  const size_t lds = ((size_t)(rowsU + 3 + p.nhead) * RP + 2 * (kThreads / T) * T + 7 * p.d + 2 * p.cout) * sizeof(float);
  // RULE: the tile kernel's LDS is judged first, whichever family then takes the launch
  if (lds > (size_t)kMaxDynLds) return PCR_ERR_INVALID;
  pl->arith = kAPrec != 0 ? PCR_PREC_BF16X3 : PCR_PREC_F32;   // (the bf unit is split bf16 whatever was requested)
#if PCR_ATTN_PREC != 0
  const long nitem = (long)p.B * (p.Lq >> 5);   // (the stream shapes: whole 32-token blocks)
  if (p.d == 128 && p.c1 == 128 && p.cout == 128 && !p.cfinal && p.q_pos && p.residual && (p.Lq & 31) == 0 && p.Lq >= 256 &&
      (p.nhead == 1 || p.nhead == 2 || p.nhead == 4) && !t.no_stream128) {
    // SA3's self-attention (d_model 128): the wave-autonomous form with the weights streamed through an LDS ring
    // (shape-only choice); one workgroup of four waves per CU.  Query sets of >= 256 tokens only, the kv kernel's
    // split-projection rule: at Lq = 32 (the Point-Transformer @128) its other rounding took one case of
    // tests/test_gpu_precision.py's margin sweep from under 5e-5 to 5.4e-5
    attn_plan_persistent(pl, nitem, kAp128Waves, 1, 64 * kAp128Waves, kAp128Lds);
    return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM128, {p.nhead}, false, gated);
  }
  const int aps_c1s = (p.c1 + 15) >> 4, aps_nd = p.d >> 5;
  const size_t aps_lds = (size_t)((aps_c1s + (p.q_pos ? 2 * aps_nd : 0)) * aps_nd * 128 + (aps_c1s + 2 * aps_nd) * aps_nd * 256 +
                                  aps_nd * (p.cout >> 5) * 512) * 16 +
                         (size_t)(448 + 256 + 64 * kApsWaves) * sizeof(float);
  if (p.d == 32 && p.c1 == 32 && p.cout == 32 && !p.cfinal && (p.Lq & 31) == 0 && (p.nhead == 1 || p.nhead == 2)) {
    // the SA1 self-attention (d_model 32): the d = 64 kernel with one 32-channel block
    attn_plan_persistent(pl, nitem, kApsWaves, 1, 64 * kApsWaves, aps_lds);
    return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM64, {p.q_pos != 0, 2, 0, 1, 1, 0}, false, gated);
  }
  if (aps64_shape(p) && aps_lds <= (size_t)kMaxDynLds) {
    pl->trace = t.trace != nullptr;
    const int cf = p.cfinal ? 4 : 0;
    if (p.pool_out) {
      // pooled output (pcr_attn_apply_pool_ok said yes): whole clouds per wave
      attn_plan_persistent(pl, p.B, kApsWaves, 1, 64 * kApsWaves, aps_lds);
      return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM64, {0, 4, 0, 2, 2, 1}, true, gated);
    }
    attn_plan_persistent(pl, nitem, kApsWaves, 1, 64 * kApsWaves, aps_lds);
    if (p.cout == 128) return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM64, {p.q_pos != 0, 4, 0, 4, 2, 0}, false, gated);
    if (p.c1 < 16) return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM64, {0, 1, 2, 1, 2, 0}, false, gated);
    if (p.c1 == 32) return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM64, {0, 2, cf, 2, 2, 0}, false, gated);
    return attn_plan_form(pl, PCR_ATTN_APPLY_STREAM64, {p.q_pos != 0, 4, cf, 2, 2, 0}, true, gated);   // the matching stages'
  }
#endif
  attn_plan_grid(pl, (p.Lq + T - 1) / T, p.B, lds);
  const bool wide = 2 * p.d > 128 || p.cout > 128 || p.cfinal > 128;   // some layer has > 4 cout blocks
  if (tb == 4) return attn_plan_form(pl, PCR_ATTN_APPLY_TILE, {4, wide ? 2 : 1}, false, gated);
  if (tb == 2) return attn_plan_form(pl, PCR_ATTN_APPLY_TILE, {2, wide ? 2 : 1}, true, gated);
  // cout blocks of the widest layer: up to 8 -> two rounds per wave, up to 16 -> four, up to 32 (d_model 512) -> eight
  int widest = 2 * p.d > p.cout ? 2 * p.d : p.cout;
  if (p.cfinal > widest) widest = p.cfinal;
  if (kAPrec != 0 && widest > 256) return PCR_ERR_INVALID;   // (the bf16 unit holds two rounds only)
  return attn_plan_form(pl, PCR_ATTN_APPLY_TILE, {1, widest > 512 ? 8 : (widest > 256 ? 4 : 2)}, false, gated);
}

// ---- one launcher per family: every kernel instantiation is named here and nowhere else, its gated twin beside it -----------
static dim3 attn_grid(const AttnPlan &pl) {
  if (!pl.persistent) return dim3(pl.gx, pl.gy);
  const long cap = (long)pl.per_cu * pcr_cu_count();
  return dim3((unsigned)(pl.work < cap ? pl.work : cap));
}
// KERN, or its gated twin when the plan says so
template <auto KERN, auto KERN_LIVE>
static inline int attn_launch_g(const AttnPlan &pl, dim3 grid, hipStream_t st, const AttnArgs &a) {
  return pl.gated ? pcr_launch_lds<KERN_LIVE>(grid, dim3(pl.threads), pl.lds, st, a)
                  : pcr_launch_lds<KERN>(grid, dim3(pl.threads), pl.lds, st, a);
}

// attn_kv_kernel<TB, NR, WSEL, NTW>
static int attn_launch_kv_tile(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  if (pl.targ[0] == 2) return pcr_launch_lds<attn_kv_kernel<2, 1, 2, 1>>(g, blk, pl.lds, st, a);
  return pcr_launch_lds<attn_kv_kernel<1, 2, 0, 4>>(g, blk, pl.lds, st, a);
}
// attn_kv_kernel_o3<TB, NR, WSEL, NTW> / attn_kv_kernel_o3_live
static int attn_launch_kv_tile_o3(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  return attn_launch_g<attn_kv_kernel_o3<2, 1, 1, 1>, attn_kv_kernel_o3_live<2, 1, 1, 1>>(pl, attn_grid(pl), st, a);
}
// attn_kv_kernel_o2<TB, NR, WSEL, NTW, BFP>
static int attn_launch_kv_tile_o2(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  if (pl.targ[4]) return pcr_launch_lds<attn_kv_kernel_o2<1, 2, 1, 4, true>>(g, blk, pl.lds, st, a);
  return pcr_launch_lds<attn_kv_kernel_o2<1, 2, 1, 4>>(g, blk, pl.lds, st, a);
}
// attn_kv_stream64_kernel<DIAG, BF, XS, ONEW, GATE>
template <bool DIAG>
static int attn_launch_kv_stream64(const AttnPlan &pl, const AttnArgs &a, const AttnTune &t, hipStream_t st) {
  const dim3 g = attn_grid(pl);
  int rc = PCR_ERR_INVALID;
  if (!pl.targ[1])
    rc = attn_launch_g<attn_kv_stream64_kernel<DIAG, false>, attn_kv_stream64_kernel<DIAG, false, 4, false, true>>(pl, g, st, a);
#if PCR_ATTN_PREC != 0
  else if (pl.targ[2] == 8) rc = pcr_launch_lds<attn_kv_stream64_kernel<DIAG, true, 8>>(g, dim3(pl.threads), pl.lds, st, a);
  else if (pl.targ[3])
    rc = attn_launch_g<attn_kv_stream64_kernel<DIAG, true, 4, true>, attn_kv_stream64_kernel<DIAG, true, 4, true, true>>(pl, g, st, a);
  else rc = attn_launch_g<attn_kv_stream64_kernel<DIAG, true>, attn_kv_stream64_kernel<DIAG, true, 4, false, true>>(pl, g, st, a);
#endif
  if (pl.trace) attn_dump_trace(t.trace, "kv64", (int)g.x, (int)a.p.B, a.p.Sk);
  return rc;
}
#if PCR_ATTN_PREC != 0
static int attn_launch_kv_stream32(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  return pcr_launch_lds<attn_kv_stream32_kernel>(attn_grid(pl), dim3(pl.threads), pl.lds, st, a);
}
// attn_kv_stream128_kernel<NH>
static int attn_launch_kv_stream128(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  if (pl.targ[0] == 2) return pcr_launch_lds<attn_kv_stream128_kernel<2>>(g, blk, pl.lds, st, a);
  return pcr_launch_lds<attn_kv_stream128_kernel<4>>(g, blk, pl.lds, st, a);
}
#else
// attn_kv_wide_kernel<NRW>
static int attn_launch_kv_wide(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  if (pl.targ[0] == 2) return pcr_launch_lds<attn_kv_wide_kernel<2>>(g, blk, pl.lds, st, a);
  return pcr_launch_lds<attn_kv_wide_kernel<3>>(g, blk, pl.lds, st, a);
}
#endif

static int attn_launch_kv(const AttnPlan &pl, AttnArgs &a, const AttnTune &t, hipStream_t st) {
  int rc = PCR_ERR_INVALID;
  if (pl.family != PCR_ATTN_KV_WIDE) a.p.kv_splits = pl.splits;
  switch (pl.family) {
    case PCR_ATTN_KV_TILE: rc = attn_launch_kv_tile(pl, a, st); break;
    case PCR_ATTN_KV_TILE_O3: rc = attn_launch_kv_tile_o3(pl, a, st); break;
    case PCR_ATTN_KV_TILE_O2: rc = attn_launch_kv_tile_o2(pl, a, st); break;
    case PCR_ATTN_KV_STREAM64:
      return pl.targ[0] ? attn_launch_kv_stream64<true>(pl, a, t, st) : attn_launch_kv_stream64<false>(pl, a, t, st);
#if PCR_ATTN_PREC != 0
    case PCR_ATTN_KV_STREAM32: return attn_launch_kv_stream32(pl, a, st);
    case PCR_ATTN_KV_STREAM128: return attn_launch_kv_stream128(pl, a, st);
#else
    case PCR_ATTN_KV_WIDE: return attn_launch_kv_wide(pl, a, st);
#endif
    default: return PCR_ERR_INVALID;
  }
  if (rc != PCR_OK || !pl.fold) return rc;
  return pcr_launch_lds<attn_kv_fold_kernel>(dim3(a.p.B), dim3(pl.threads), pl.fold_lds, st, a);
}

// attn_apply_kernel<TB, NR, GATE>
static int attn_launch_apply_tile(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  switch (pl.targ[0] * 10 + pl.targ[1]) {
    case 41: return pcr_launch_lds<attn_apply_kernel<4, 1>>(g, blk, pl.lds, st, a);
    case 42: return pcr_launch_lds<attn_apply_kernel<4, 2>>(g, blk, pl.lds, st, a);
    case 21: return attn_launch_g<attn_apply_kernel<2, 1>, attn_apply_kernel<2, 1, true>>(pl, g, st, a);
    case 22: return attn_launch_g<attn_apply_kernel<2, 2>, attn_apply_kernel<2, 2, true>>(pl, g, st, a);
    case 12: return pcr_launch_lds<attn_apply_kernel<1, 2>>(g, blk, pl.lds, st, a);
#if PCR_ATTN_PREC == 0
    case 14: return pcr_launch_lds<attn_apply_kernel<1, 4>>(g, blk, pl.lds, st, a);
    case 18: return pcr_launch_lds<attn_apply_kernel<1, 8>>(g, blk, pl.lds, st, a);
#endif
    default: return PCR_ERR_INVALID;
  }
}
#if PCR_ATTN_PREC != 0
// attn_apply_stream64_kernel<QPOS, C1S, CF, NOB, ND, POOL, GATE>
template <bool QPOS>
static int attn_launch_apply_stream64(const AttnPlan &pl, const AttnArgs &a, const AttnTune &t, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  const int c1s = pl.targ[1], cf = pl.targ[2], nob = pl.targ[3], nd = pl.targ[4];
  int rc = PCR_ERR_INVALID;
  if (nd == 1) rc = pcr_launch_lds<attn_apply_stream64_kernel<QPOS, 2, 0, 1, 1>>(g, blk, pl.lds, st, a);
  else if (nob == 4) rc = pcr_launch_lds<attn_apply_stream64_kernel<QPOS, 4, 0, 4>>(g, blk, pl.lds, st, a);
  else if (c1s == 4 && cf && !pl.targ[5])
    rc = attn_launch_g<attn_apply_stream64_kernel<QPOS, 4, 4>, attn_apply_stream64_kernel<QPOS, 4, 4, 2, 2, false, true>>(pl, g, st, a);
  else if (c1s == 4 && !pl.targ[5])
    rc = attn_launch_g<attn_apply_stream64_kernel<QPOS, 4, 0>, attn_apply_stream64_kernel<QPOS, 4, 0, 2, 2, false, true>>(pl, g, st, a);
  else if constexpr (!QPOS) {
    if (pl.targ[5])   // (the pooled form stamps with a trace file set, but has never dumped)
      return attn_launch_g<attn_apply_stream64_kernel<false, 4, 0, 2, 2, true>, attn_apply_stream64_kernel<false, 4, 0, 2, 2, true, true>>(pl, g, st, a);
    if (c1s == 1) rc = pcr_launch_lds<attn_apply_stream64_kernel<false, 1, 2, 1>>(g, blk, pl.lds, st, a);
    else if (cf) rc = pcr_launch_lds<attn_apply_stream64_kernel<false, 2, 4>>(g, blk, pl.lds, st, a);
    else rc = pcr_launch_lds<attn_apply_stream64_kernel<false, 2, 0>>(g, blk, pl.lds, st, a);
  }
  if (pl.trace) attn_dump_trace(t.trace, "apply64", (int)g.x, (int)a.p.B, a.p.Lq);
  return rc;
}
// attn_apply_stream128_kernel<NH>
static int attn_launch_apply_stream128(const AttnPlan &pl, const AttnArgs &a, hipStream_t st) {
  const dim3 g = attn_grid(pl), blk(pl.threads);
  if (pl.targ[0] == 1) return pcr_launch_lds<attn_apply_stream128_kernel<1>>(g, blk, pl.lds, st, a);
  if (pl.targ[0] == 2) return pcr_launch_lds<attn_apply_stream128_kernel<2>>(g, blk, pl.lds, st, a);
  return pcr_launch_lds<attn_apply_stream128_kernel<4>>(g, blk, pl.lds, st, a);
}
#endif

static int attn_launch_apply(const AttnPlan &pl, const AttnArgs &a, const AttnTune &t, hipStream_t st) {
  (void)t;
  switch (pl.family) {
    case PCR_ATTN_APPLY_TILE: return attn_launch_apply_tile(pl, a, st);
#if PCR_ATTN_PREC != 0
    case PCR_ATTN_APPLY_STREAM64:
      return pl.targ[0] ? attn_launch_apply_stream64<true>(pl, a, t, st) : attn_launch_apply_stream64<false>(pl, a, t, st);
    case PCR_ATTN_APPLY_STREAM128: return attn_launch_apply_stream128(pl, a, st);
#endif
    default: return PCR_ERR_INVALID;
  }
}

// One unit: its plan, and the launch when one is asked for (pcr_attn_launch_form asks for none and leaves the device and
// pcr_last_launch_arith alone).  live, when given, has passed attn_entry's checks.
static int attn_unit(const pcr_attn_params &p, const pcr_live *live, bool apply, AttnPlan *pl, bool launch, pcr_stream_t stream) {
  const AttnTune &t = attn_tune();
  *pl = AttnPlan();
  const int rc = apply ? attn_plan_apply(p, live != nullptr, t, pl) : attn_plan_kv(p, live != nullptr, t, pl);
  if (!launch) return rc;
  if (pl->arith >= 0) pcr_note_arith(pl->arith);
  if (rc != PCR_OK) return rc;
  AttnArgs a;
  a.p = p;
  // PCR_ATTN_KV_FULL (tuning builds; for the skip test and the A/B, not for users) is read at every launch, not once per
  // process like AttnTune: a test flips it between two launches of one process
  a.dbg = (pl->trace ? 256 : 0) | (pcr_tune_int("PCR_ATTN_KV_FULL") ? 512 : 0);
  a.wpc = pl->wpc;
  // gated launches (pcr_live): the caller's count, period and offset travel in AttnArgs
  a.live_count = live ? live->count : nullptr;
  a.live_period = live ? live->period : 0;
  a.live_offset = live ? live->offset : 0;
  return apply ? attn_launch_apply(*pl, a, t, pcr_s(stream)) : attn_launch_kv(*pl, a, t, pcr_s(stream));
}

#if PCR_ATTN_PREC == 1
// (the caller -- attn_kernels.hip -- has validated the parameters and swapped the bf16 images into wq / wkv / ...)
int pcr_attn_kv_bf3(const pcr_attn_params *pp, const pcr_live *live, AttnPlan *pl, bool launch, pcr_stream_t stream) {
  return attn_unit(*pp, live, false, pl, launch, stream);
}
int pcr_attn_apply_bf3(const pcr_attn_params *pp, const pcr_live *live, AttnPlan *pl, bool launch, pcr_stream_t stream) {
  return attn_unit(*pp, live, true, pl, launch, stream);
}
#else
int pcr_attn_kv_bf3(const pcr_attn_params *pp, const pcr_live *live, AttnPlan *pl, bool launch, pcr_stream_t stream);      // attn_kernels_bf3.hip
int pcr_attn_apply_bf3(const pcr_attn_params *pp, const pcr_live *live, AttnPlan *pl, bool launch, pcr_stream_t stream);

// precision != f32, d_model <= 128 and bf16 images given: the same parameters with the images swapped in
static bool attn_bf(const pcr_attn_params &p, pcr_attn_params &q) {
  const int widest = 2 * p.d > p.cout ? (2 * p.d > p.cfinal ? 2 * p.d : p.cfinal) : (p.cout > p.cfinal ? p.cout : p.cfinal);
  if (p.precision == 0 || p.d > 128 || widest > 256 || !p.wq_bf || !p.wmlp0_bf || !p.wmlp2_bf ||
      (p.cfinal && !p.wfinal_bf))
    return false;
  q = p;      // (wkv stays the f32 image: the kv kernel's projection is f32 in both units, only its output M changes form)
  q.wq = p.wq_bf; q.wmlp0 = p.wmlp0_bf; q.wmlp2 = p.wmlp2_bf; q.wfinal = p.wfinal_bf;
  return true;
}

// Suggested token split of a kv launch: a function of the launch SHAPE only (never of the batch size), so that a pair's
// logits do not depend on how many other pairs share its launch (tests/test_gpu_fullsize.py holds the bench batch to the
// logits of the same pairs run in small groups, bit for bit).  Measured on pt1024 (1024 clouds): 1 / 2 / 3 / 4 splits
// run the d = 64, Sk = 1024 launches in 0.495 / 0.484 / 0.476 / 0.492 ms -- a grid that fills the chip is bound by its
// per-tile work, so the split costs nothing there -- while a few clouds (gallery queries, small batches) gain the
// parallelism they lack.  d = 128 stays whole: its partial matrices are as large as its inputs (0.73 -> 0.85 ms at two).
PCR_EXPORT int pcr_attn_kv_splits(int B, int Sk, int d) {
  (void)B;
  if (Sk < 1 || d > 64) return 1;
  if ((d == 64 || d == 32) && (Sk & 31) == 0) return 1;   // the wave-autonomous kernels' shapes (attn_kv_stream64 / 32): whole clouds
  const int ntile = (Sk + 63) / 64;
  return ntile >= 16 ? 4 : (ntile >= 8 ? 2 : 1);
}

static bool attn_pool_ok(const pcr_attn_params &p) {
  pcr_attn_params q;
  return aps64_shape(p) && p.c1 == 64 && p.cout == 64 && !p.cfinal && !p.q_pos && attn_bf(p, q);
}

// Both launches and the form query: what is refused whichever unit would run it, the gate (checked HERE and nowhere else:
// never a silent un-gated launch), then the unit -- the bf16 unit where attn_bf says so, else this one.
static int attn_entry(const pcr_attn_params *pp, const pcr_live *live, bool apply, AttnPlan *pl, bool launch, pcr_stream_t stream) {
  if (!pp || attn_check(*pp)) return PCR_ERR_INVALID;
  if (apply && ((!pp->out && !pp->pool_out) || (pp->pool_out && !attn_pool_ok(*pp)))) return PCR_ERR_INVALID;
  if (live && !attn_live_shape(*pp)) return PCR_ERR_INVALID;
  if (launch && pp->B == 0) return PCR_OK;   // (the query reports the plan of an empty launch)
  if (apply && pp->B > 65535) return PCR_ERR_INVALID;
  if (live && (!live->count || live->period < 1 || live->offset < 0)) return PCR_ERR_INVALID;
  pcr_attn_params q;
  if (attn_bf(*pp, q)) return apply ? pcr_attn_apply_bf3(&q, live, pl, launch, stream) : pcr_attn_kv_bf3(&q, live, pl, launch, stream);
  return attn_unit(*pp, live, apply, pl, launch, stream);
}

PCR_EXPORT int pcr_attn_kv_f32(const pcr_attn_params *pp, pcr_stream_t stream) {
  AttnPlan pl;
  return attn_entry(pp, nullptr, false, &pl, true, stream);
}
PCR_EXPORT int pcr_attn_kv_live_f32(const pcr_attn_params *pp, const pcr_live *live, pcr_stream_t stream) {
  AttnPlan pl;
  return attn_entry(pp, live, false, &pl, true, stream);
}
PCR_EXPORT int pcr_attn_apply_f32(const pcr_attn_params *pp, pcr_stream_t stream) {
  AttnPlan pl;
  return attn_entry(pp, nullptr, true, &pl, true, stream);
}
PCR_EXPORT int pcr_attn_apply_live_f32(const pcr_attn_params *pp, const pcr_live *live, pcr_stream_t stream) {
  AttnPlan pl;
  return attn_entry(pp, live, true, &pl, true, stream);
}
PCR_EXPORT int pcr_attn_live_ok(const pcr_attn_params *pp) {
  return (pp && !attn_check(*pp) && attn_live_shape(*pp)) ? 1 : 0;
}
PCR_EXPORT int pcr_attn_apply_pool_ok(const pcr_attn_params *pp) {
  return (pp && !attn_check(*pp) && attn_pool_ok(*pp)) ? 1 : 0;
}

PCR_EXPORT int pcr_attn_launch_form(const pcr_attn_params *pp, const pcr_live *live, int apply, int *form) {
  if (!form) return PCR_ERR_INVALID;
  AttnPlan pl;
  const int rc = attn_entry(pp, live, apply != 0, &pl, false, nullptr);
  if (rc != PCR_OK) return rc;
  for (int i = 0; i < PCR_ATTN_FORM_INTS; i++) form[i] = 0;
  form[0] = pl.arith;
  form[1] = pl.family;
  form[2] = pl.gated;
  form[3] = pl.ntarg;
  for (int i = 0; i < pl.ntarg; i++) form[4 + i] = pl.targ[i];
  if (!apply) {
    form[10] = pl.splits;
    form[11] = pl.fold;
    form[12] = pl.wpc;
  }
  form[13] = (int)pl.lds;
  return PCR_OK;
}
#endif

