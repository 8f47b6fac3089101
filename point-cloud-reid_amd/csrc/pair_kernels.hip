// Pair head over per-object embedding tables (pcr.h, section A10): the `concat` matching head of a gallery.
//   z = relu(GN1(u[i] + v[j]));  y = GN2(W2 z) + [e_i | e_j];  logit = w_out . relu(y) + b_out
// One workgroup of n/32 waves walks tiles of 32 pairs.  Wave w owns the output channels [32 w, 32 w + 32) of W2 and keeps
// its slice of the packed image in registers for the whole launch (n/2 VGPRs per lane: 128 at n = 256); the 32 pairs of a
// tile are the 32 columns of v_mfma_f32_32x32x2_f32.  A GroupNorm group of <= 32 channels never leaves a wave's slice, so
// the second GroupNorm, the residual and the output dot product are done on the accumulators.
// A column's arithmetic is a function of that column alone -- the same instructions in the same order wherever the pair
// stands in the list, whatever P and *count are -- which is the batch-independence rule of the header.
#include "pcr_common.h"

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 32;    // pairs per tile: the columns of one MFMA
constexpr int kPitch = 33;   // floats per channel row of the tile in LDS

struct PairArgs {
  pcr_pair_head_params p;
  const int *count;          // NULL: every pair is live
  int period, offset;
  float dead_value;
};

enum { kLive = 0, kDead = 1, kBad = 2 };

template <int NW, int GS>
__global__ __launch_bounds__(64 * NW) void pair_head_kernel(PairArgs a) {
  constexpr int n = 32 * NW, F = n / 2, QN = n / 4, KB = n / 8, kT = 64 * NW;
  constexpr int NG = GS == 4 ? 4 : GS / 2;       // accumulator registers of a lane that belong to one group
  constexpr bool kCross = GS >= 8;               // the group's other half sits in lane ^ 32
  __shared__ float Z[n * kPitch];
  __shared__ __attribute__((aligned(16))) float s_g2[n], s_b2[n], s_wo[n];
  __shared__ float s_part[NW * kTile];
  __shared__ int s_i[kTile], s_j[kTile], s_st[kTile];
  const pcr_pair_head_params &p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const long P = p.P;
  int c = 0;
  if (a.count) {
    c = __builtin_amdgcn_readfirstlane(*a.count);
    c = (c < 0 ? 0 : c) - a.offset;
    c = c < 0 ? 0 : (c > a.period ? a.period : c);
  }
  const bool plain_gate = a.count && (long)a.period >= P;     // then pair p is live iff p < c, and whole tiles are dead
  for (int e = tid; e < n; e += kT) {
    s_g2[e] = p.gn2_g[e];
    s_b2[e] = p.gn2_b[e];
    s_wo[e] = p.w_out[e];
  }
  // the wave's slice of W2: k-block kb, f32x4 at [kb][cout][h], element qq = W2[cout][8 kb + 2 qq + h]
  f32x4 wreg[KB];
  {
    const f32x4 *wv = reinterpret_cast<const f32x4 *>(p.w2p) + (size_t)(wave * 32 + l31) * 2 + h;
#pragma unroll
    for (int kb = 0; kb < KB; kb++) wreg[kb] = wv[(size_t)kb * n * 2];
  }
  // first phase: thread -> (pair tid / QN of every eight, channels 4 cq .. 4 cq + 3)
  const int cq = tid % QN, tq = tid / QN;
  const f32x4 g1 = *reinterpret_cast<const f32x4 *>(p.gn1_g + 4 * cq), b1 = *reinterpret_cast<const f32x4 *>(p.gn1_b + 4 * cq);
  const float b_out = p.b_out[0];
  const long ntiles = (P + kTile - 1) / kTile;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * kTile;
    if (plain_gate && p0 >= (long)c) {           // workgroup-uniform: nothing of the tile is read
      if (tid < kTile && p0 + tid < P) p.logits[p0 + tid] = a.dead_value;
      continue;
    }
    if (tid < kTile) {
      const long pr = p0 + tid;
      int st = kDead, i = 0, j = 0;
      if (pr < P && (!a.count || (int)(pr % a.period) < c)) {
        const int2 ij = reinterpret_cast<const int2 *>(p.pairs)[pr];
        i = ij.x;
        j = ij.y;
        st = (i >= 0 && i < p.M && j >= 0 && j < p.M) ? kLive : kBad;
      }
      s_i[tid] = i;
      s_j[tid] = j;
      s_st[tid] = st;
    }
    __syncthreads();
    // ---- z = relu(GN1(u[i] + v[j])) into Z[channel][pair]
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int t = s * 8 + tq;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (s_st[t] == kLive) {
        const f32x4 u4 = *reinterpret_cast<const f32x4 *>(p.u + (size_t)s_i[t] * n + 4 * cq);
        const f32x4 v4 = *reinterpret_cast<const f32x4 *>(p.v + (size_t)s_j[t] * n + 4 * cq);
        x = u4 + v4;
      }
      float sum = (x[0] + x[1]) + (x[2] + x[3]);
      if (GS >= 8) sum += __shfl_xor(sum, 1, 64);
      if (GS >= 16) sum += __shfl_xor(sum, 2, 64);
      if (GS >= 32) sum += __shfl_xor(sum, 4, 64);
      const float mean = sum / (float)GS;
      const f32x4 d = x - mean;
      float var = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      if (GS >= 8) var += __shfl_xor(var, 1, 64);
      if (GS >= 16) var += __shfl_xor(var, 2, 64);
      if (GS >= 32) var += __shfl_xor(var, 4, 64);
      const float rstd = 1.0f / sqrtf(var / (float)GS + 1e-5f);
#pragma unroll
      for (int k = 0; k < 4; k++) Z[(4 * cq + k) * kPitch + t] = fmaxf(d[k] * rstd * g1[k] + b1[k], 0.f);
    }
    __syncthreads();
    // ---- W2 z: the wave's 32 output channels of the tile's 32 pairs
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    {
      const float *bp = Z + h * kPitch + l31;
#pragma unroll
      for (int kb = 0; kb < KB; kb++) {
        float xq[4];
#pragma unroll
        for (int qq = 0; qq < 4; qq++) xq[qq] = bp[(kb * 8 + 2 * qq) * kPitch];
#pragma unroll
        for (int qq = 0; qq < 4; qq++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[kb][qq], xq[qq], acc, 0, 0, 0);
      }
    }
    // ---- y = GN2(.) + [e_i | e_j], the lane's share of w_out . relu(y).  Register r of the lane is channel
    // 32 wave + 8 (r / 4) + 4 h + r % 4 of pair l31.
    {
      const bool live = s_st[l31] == kLive;
      const int oi = s_i[l31], oj = s_j[l31];
      float part = 0.f;
#pragma unroll
      for (int q = 0; q < 16 / NG; q++) {
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < NG; r++) sum += acc[q * NG + r];
        if (kCross) sum += __shfl_xor(sum, 32, 64);
        const float mean = sum / (float)GS;
        float var = 0.f;
#pragma unroll
        for (int r = 0; r < NG; r++) {
          const float dd = acc[q * NG + r] - mean;
          var += dd * dd;
        }
        if (kCross) var += __shfl_xor(var, 32, 64);
        const float rstd = 1.0f / sqrtf(var / (float)GS + 1e-5f);
#pragma unroll
        for (int r4 = 0; r4 < NG; r4 += 4) {
          const int r0 = q * NG + r4;
          const int ch = 32 * wave + 8 * (r0 >> 2) + 4 * h;
          f32x4 res = {0.f, 0.f, 0.f, 0.f};
          if (live)
            res = *reinterpret_cast<const f32x4 *>(ch < F ? p.emb + (size_t)oi * F + ch : p.emb + (size_t)oj * F + (ch - F));
          const f32x4 gg = *reinterpret_cast<const f32x4 *>(s_g2 + ch), bb = *reinterpret_cast<const f32x4 *>(s_b2 + ch);
          const f32x4 ww = *reinterpret_cast<const f32x4 *>(s_wo + ch);
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const float y = (acc[r0 + k] - mean) * rstd * gg[k] + bb[k] + res[k];
            part += fmaxf(y, 0.f) * ww[k];
          }
        }
      }
      part += __shfl_xor(part, 32, 64);
      if (h == 0) s_part[wave * kTile + l31] = part;
    }
    __syncthreads();
    if (tid < kTile && p0 + tid < P) {
      float s = s_part[tid];
#pragma unroll
      for (int w = 1; w < NW; w++) s += s_part[w * kTile + tid];
      s += b_out;
      const int st = s_st[tid];
      p.logits[p0 + tid] = st == kLive ? s : (st == kDead ? a.dead_value : __builtin_nanf(""));
    }
  }
}

template <int NW>
int pair_head_launch_gs(int gs, dim3 grid, hipStream_t st, const PairArgs &a) {
  switch (gs) {
    case 4: return pcr_launch<pair_head_kernel<NW, 4>>(grid, dim3(64 * NW), 0, st, a);
    case 8: return pcr_launch<pair_head_kernel<NW, 8>>(grid, dim3(64 * NW), 0, st, a);
    case 16: return pcr_launch<pair_head_kernel<NW, 16>>(grid, dim3(64 * NW), 0, st, a);
    case 32: return pcr_launch<pair_head_kernel<NW, 32>>(grid, dim3(64 * NW), 0, st, a);
  }
  return PCR_ERR_INVALID;
}
}  // namespace

PCR_EXPORT int pcr_pair_head_ok(int F, int groups) {
  if (F != 32 && F != 64 && F != 128) return 0;
  if (groups < 1 || (2 * F) % groups) return 0;
  const int gs = 2 * F / groups;
  return gs == 4 || gs == 8 || gs == 16 || gs == 32;
}

PCR_EXPORT int pcr_pair_head_f32(const pcr_pair_head_params *pp, const pcr_live *live, const float *dead_value,
                                 pcr_stream_t stream) {
  if (!pp) return PCR_ERR_INVALID;
  const pcr_pair_head_params &p = *pp;
  if (!pcr_pair_head_ok(p.F, p.groups) || p.n != 2 * p.F || p.M < 0 || p.P < 0) return PCR_ERR_INVALID;
  if (live && (!live->count || live->period < 1 || live->offset < 0)) return PCR_ERR_INVALID;
  if (p.P == 0) return PCR_OK;
  if (!p.pairs || !p.w2p || !p.gn1_g || !p.gn1_b || !p.gn2_g || !p.gn2_b || !p.w_out || !p.b_out || !p.logits)
    return PCR_ERR_INVALID;
  if (p.M > 0 && (!p.emb || !p.u || !p.v)) return PCR_ERR_INVALID;
  // 16-byte rows and images, 8-byte index pairs
  const size_t a16 = reinterpret_cast<size_t>(p.emb) | reinterpret_cast<size_t>(p.u) | reinterpret_cast<size_t>(p.v) |
                     reinterpret_cast<size_t>(p.w2p) | reinterpret_cast<size_t>(p.gn1_g) | reinterpret_cast<size_t>(p.gn1_b);
  if ((a16 & 15) || (reinterpret_cast<size_t>(p.pairs) & 7)) return PCR_ERR_INVALID;
  pcr_note_arith(PCR_PREC_F32);
  const PairArgs a{p, live ? live->count : nullptr, live ? live->period : 1, live ? live->offset : 0,
                   dead_value ? *dead_value : 0.f};
  const long ntiles = (p.P + kTile - 1) / kTile;
  const long cap = 4L * pcr_cu_count();
  const dim3 grid((unsigned)(ntiles < cap ? ntiles : cap));
  const int gs = p.n / p.groups;
  switch (p.F) {
    case 32: return pair_head_launch_gs<2>(gs, grid, pcr_s(stream), a);
    case 64: return pair_head_launch_gs<4>(gs, grid, pcr_s(stream), a);
    case 128: return pair_head_launch_gs<8>(gs, grid, pcr_s(stream), a);
  }
  return PCR_ERR_INVALID;
}
