// The auxiliary training losses of ReIDNet that have a hot path (include/pcr.h, section C2): the pairwise KL term
// (get_kl_loss, ReIDNet.py:467-482) and the triplet term (get_triplet_loss, :538-582) as a draw, a tiled distance
// matrix, a hinge selection and the distance backward.
//
// f32 vector work, no matrix core.  Every sum has ONE order, fixed by the launch shape: per-thread strides in index order,
// a shuffle tree inside the wave, the waves in order.  The only atomics are integer ones (LDS counters, the sticky info
// word), so every output is the same bits on every run.  tests/aux_ref.py restates all of it in float64 and numpy.
#include "pcr_common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr uint32_t kStreamTriplet = 3u;
constexpr float kEps = PCR_PAIR_DIST_EPS;

// ---- fixed-order block reductions: lane 0 of a shfl_down tree, then the waves left to right ----
template <class T>
__device__ __forceinline__ T wave_sum_down(T v) {
  for (int o = kWave / 2; o; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;          // (lane 0 holds the sum)
}

template <class T>
__device__ __forceinline__ T block_sum(T v, T *red) {
  v = wave_sum_down(v);
  __syncthreads();   // (red may still be read from a previous call)
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = red[0];
  for (int w = 1; w < kWaves; ++w) s += red[w];
  return s;
}

// ---- kl ----
// Online log-sum-exp state of a row: m the running maximum, s = sum exp(x - m), and for the target row
// a = sum exp(x - m) * w with w = h2 - h1.
__device__ __forceinline__ void lse_push(float &m, float &s, float &a, float x, float w) {
  if (x > m) {
    const float e = expf(m - x);       // (m = -inf: 0)
    s = s * e + 1.f;
    a = a * e + w;
    m = x;
  } else {
    const float e = expf(x - m);
    s += e;
    a += e * w;
  }
}

__device__ __forceinline__ void lse_merge(float &m, float &s, float &a, float mb, float sb, float ab) {
  const float mm = fmaxf(m, mb);
  const float ea = m == -INFINITY ? 0.f : expf(m - mm), eb = mb == -INFINITY ? 0.f : expf(mb - mm);
  s = s * ea + sb * eb;
  a = a * ea + ab * eb;
  m = mm;
}

// One workgroup per pair: ONE pass over the two rows.
__global__ __launch_bounds__(kThreads) void kl_pairs_fwd_kernel(const float *__restrict__ h, float *__restrict__ lse,
                                                                float *__restrict__ cross, float *__restrict__ kl, int B,
                                                                int D) {
  __shared__ float red[kWaves][6];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1);
  const float *x1 = h + (size_t)i * D, *x2 = h + ((size_t)B + i) * D;
  float m1 = -INFINITY, s1 = 0.f, a1 = 0.f, m2 = -INFINITY, s2 = 0.f, a2 = 0.f;
  for (int j = tid; j < D; j += kThreads) {
    const float u = x1[j], v = x2[j];
    lse_push(m1, s1, a1, u, 0.f);
    lse_push(m2, s2, a2, v, v - u);
  }
  for (int o = kWave / 2; o; o >>= 1) {
    const float mb1 = __shfl_down(m1, o, kWave), sb1 = __shfl_down(s1, o, kWave);
    const float mb2 = __shfl_down(m2, o, kWave), sb2 = __shfl_down(s2, o, kWave), ab2 = __shfl_down(a2, o, kWave);
    lse_merge(m1, s1, a1, mb1, sb1, 0.f);
    lse_merge(m2, s2, a2, mb2, sb2, ab2);
  }
  if (lane == 0) {
    float *r = red[tid >> 6];
    r[0] = m1, r[1] = s1, r[2] = m2, r[3] = s2, r[4] = a2;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      lse_merge(m1, s1, a1, red[w][0], red[w][1], 0.f);
      lse_merge(m2, s2, a2, red[w][2], red[w][3], red[w][4]);
    }
    const float l1 = m1 + logf(s1), l2 = m2 + logf(s2), c = a2 / s2;
    lse[i] = l1;
    lse[(size_t)B + i] = l2;
    cross[i] = c;
    kl[i] = (c - (l2 - l1)) / (float)D;
  }
}

// One workgroup: the group counts and the two group means, pairs in index order, binary64 sums.
__global__ __launch_bounds__(kThreads) void kl_pairs_fin_kernel(const float *__restrict__ kl, const int *__restrict__ match,
                                                                float *__restrict__ loss, int *__restrict__ counts,
                                                                int *__restrict__ info, int B) {
  __shared__ double redd[kWaves];
  __shared__ int redi[kWaves];
  double s0 = 0.0, s1 = 0.0;
  int n1 = 0;
  for (int i = threadIdx.x; i < B; i += kThreads) {
    if (match[i]) s1 += (double)kl[i], ++n1;
    else s0 -= (double)kl[i];
  }
  s0 = block_sum(s0, redd);
  s1 = block_sum(s1, redd);
  n1 = block_sum(n1, redi);
  if (threadIdx.x == 0) {
    const int n0 = B - n1;
    loss[0] = (float)((n0 ? s0 / n0 : 0.0) + (n1 ? s1 / n1 : 0.0));
    counts[0] = n0, counts[1] = n1;
    if (!n0 || !n1) atomicOr(info, PCR_AUX_INFO_KL_EMPTY);
  }
}

constexpr int kKlChunk = 4 * kThreads;

__global__ __launch_bounds__(kThreads) void kl_pairs_bwd_kernel(const float *__restrict__ h, const int *__restrict__ match,
                                                                const float *__restrict__ lse, const float *__restrict__ cross,
                                                                const int *__restrict__ counts, const float *__restrict__ gout,
                                                                float *__restrict__ dh, int B, int D, int nchunk) {
  const int i = blockIdx.x / nchunk, c = blockIdx.x - i * nchunk;
  const bool mt = match[i] != 0;
  const int n = counts[mt ? 1 : 0];                  // (>= 1: pair i is in its own group)
  const float w = (mt ? gout[0] : -gout[0]) / ((float)n * (float)D);
  const float l1 = lse[i], l2 = lse[(size_t)B + i], s = cross[i];
  const size_t o1 = (size_t)i * D, o2 = ((size_t)B + i) * D;
  const int j1 = min(D, (c + 1) * kKlChunk);
  for (int j = c * kKlChunk + threadIdx.x; j < j1; j += kThreads) {
    const float u = h[o1 + j], v = h[o2 + j];
    const float p1 = expf(u - l1), p2 = expf(v - l2);
    dh[o1 + j] = w * (p1 - p2);
    dh[o2 + j] = w * p2 * ((v - u) - s);
  }
}

// ---- triplet: the draw ----
// One wave per pair; the pool lives in LDS.
__global__ __launch_bounds__(kWave) void triplet_draw_kernel(const int *__restrict__ ids, const int *__restrict__ match,
                                                             const uint32_t *__restrict__ rnd,
                                                             const unsigned long long *__restrict__ seed, int *__restrict__ neg,
                                                             int *__restrict__ info, int B, int T) {
  extern __shared__ int pool[];
  const int i = blockIdx.x, lane = threadIdx.x, R = 2 * B;
  int *out = neg + (size_t)i * T;
  int P = 0;
  if (match[i]) {
    const int m = ids[i];
    for (int r0 = 0; r0 < R; r0 += kWave) {
      const int r = r0 + lane;
      const bool f = r < R && ids[r] != m;
      const unsigned long long b = __ballot(f);
      if (f) pool[P + __popcll(b & ((1ull << lane) - 1ull))] = r;
      P += __popcll(b);
    }
    if (P == 0 && lane == 0) atomicOr(info, PCR_AUX_INFO_TRIPLET_POOL);
  }
  __syncthreads();
  if (P == 0) {                                      // a non-matching pair, or no row with another id
    for (int t = lane; t < T; t += kWave) out[t] = -1;
    return;
  }
  const uint32_t hh = pcr_word_prefix(seed ? seed[0] : 0ull, kStreamTriplet, (uint32_t)i);
  const uint32_t *w = rnd ? rnd + (size_t)i * T : nullptr;
  if (P < T) {                                       // with replacement
    for (int t = lane; t < T; t += kWave) out[t] = pool[pcr_pick(w ? w[t] : pcr_mix32(hh ^ (uint32_t)t), (uint32_t)P)];
  } else if (lane == 0) {                            // T steps of a Fisher-Yates shuffle of the pool
    for (int t = 0; t < T; ++t) {
      const int j = t + (int)pcr_pick(w ? w[t] : pcr_mix32(hh ^ (uint32_t)t), (uint32_t)(P - t));
      const int a = pool[t], b = pool[j];
      pool[t] = b, pool[j] = a;
      out[t] = b;
    }
  }
}

// ---- triplet: the distance matrix ----
constexpr int kTile = 32, kPitch = kTile + 1;

// A 32 x 32 tile of dist per workgroup, 2 x 2 entries per thread, D in chunks of 32 through LDS; every entry is ONE
// accumulator that walks d = 0 .. D - 1.
__global__ __launch_bounds__(kThreads) void pair_dist_kernel(const float *__restrict__ a, const float *__restrict__ h,
                                                             float *__restrict__ dist, int B, int R, int D) {
  __shared__ float ta[kTile * kPitch], th[kTile * kPitch];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * kTile, r0 = blockIdx.x * kTile;
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int d0 = 0; d0 < D; d0 += kTile) {
    const int dl = min(kTile, D - d0);
    for (int q = tid; q < kTile * kTile; q += kThreads) {
      const int row = q >> 5, col = q & 31;
      const bool in = col < dl;
      ta[row * kPitch + col] = (in && i0 + row < B) ? a[(size_t)(i0 + row) * D + d0 + col] : 0.f;
      th[row * kPitch + col] = (in && r0 + row < R) ? h[(size_t)(r0 + row) * D + d0 + col] : 0.f;
    }
    __syncthreads();
    for (int d = 0; d < dl; ++d) {
      const float a0 = ta[ty * kPitch + d], a1 = ta[(ty + 16) * kPitch + d];
      const float h0 = th[tx * kPitch + d], h1 = th[(tx + 16) * kPitch + d];
      // (a - h) + eps in this order: where a row meets its anchor the difference is exactly eps
      const float e00 = (a0 - h0) + kEps, e01 = (a0 - h1) + kEps, e10 = (a1 - h0) + kEps, e11 = (a1 - h1) + kEps;
      acc[0][0] += e00 * e00, acc[0][1] += e01 * e01, acc[1][0] += e10 * e10, acc[1][1] += e11 * e11;
    }
    __syncthreads();
  }
  for (int p = 0; p < 2; ++p)
    for (int q = 0; q < 2; ++q) {
      const int i = i0 + ty + 16 * p, r = r0 + tx + 16 * q;
      if (i < B && r < R) dist[(size_t)i * R + r] = sqrtf(acc[p][q]);
    }
}

// ---- triplet: hinge, coefficients ----
__global__ __launch_bounds__(kThreads) void triplet_select_kernel(const float *__restrict__ dist, const int *__restrict__ neg,
                                                                  const int *__restrict__ match, const float *__restrict__ hyper,
                                                                  float *__restrict__ E, float *__restrict__ pair_loss, int B,
                                                                  int T) {
  extern __shared__ int cnt[];
  __shared__ float redf[kWaves];
  __shared__ int redi[kWaves];
  const int i = blockIdx.x, tid = threadIdx.x, R = 2 * B;
  for (int r = tid; r < R; r += kThreads) cnt[r] = 0;
  __syncthreads();
  const int *ng = neg + (size_t)i * T;
  const float *di = dist + (size_t)i * R;
  const bool valid = match[i] != 0 && ng[0] >= 0;
  const float margin = hyper[0], dap = di[B + i];
  float v = 0.f;
  int k = 0;
  if (valid)
    for (int t = tid; t < T; t += kThreads) {
      const int r = ng[t];
      if (r < 0 || r >= R) continue;                 // (never a row outside dist, whatever neg holds)
      const float x = dap - di[r] + margin;
      if (x > 0.f) {
        v += x;
        ++k;
        atomicAdd(&cnt[r], 1);
      }
    }
  v = block_sum(v, redf);
  k = block_sum(k, redi);                            // (its barriers order the LDS counters too)
  float *Ei = E + (size_t)i * R;
  for (int r = tid; r < R; r += kThreads) {
    const int c = cnt[r];
    const float d = di[r];
    float e = (c && d > 0.f) ? (float)c / d : 0.f;
    if (r == B + i && k && dap > 0.f) e -= (float)k / dap;
    Ei[r] = e;
  }
  if (tid == 0) pair_loss[i] = v;
}

__global__ __launch_bounds__(kThreads) void triplet_fin_kernel(const float *__restrict__ pair_loss, const int *__restrict__ neg,
                                                               const int *__restrict__ match, const float *__restrict__ hyper,
                                                               float *__restrict__ loss, int *__restrict__ count,
                                                               int *__restrict__ info, int B, int T) {
  __shared__ double redd[kWaves];
  __shared__ int redi[kWaves];
  double s = 0.0;
  int nv = 0;
  for (int i = threadIdx.x; i < B; i += kThreads)
    if (match[i] != 0 && neg[(size_t)i * T] >= 0) s += (double)pair_loss[i], ++nv;
  s = block_sum(s, redd);
  nv = block_sum(nv, redi);
  if (threadIdx.x == 0) {
    const int n = nv * T;
    loss[0] = n ? (float)((double)hyper[1] * s / n) : 0.f;
    count[0] = n;
    if (!n) atomicOr(info, PCR_AUX_INFO_TRIPLET_NONE);
  }
}

// ---- triplet: the distance backward ----
// blockIdx.y < B: the anchor row i = blockIdx.y of da; otherwise the row r = blockIdx.y - B of dh.  A workgroup owns
// kKlChunk columns of its row and adds the other side's rows in index order; the coefficients come through LDS 256 at a
// time, and a zero coefficient (all but T + 1 of an anchor's) is skipped by the whole workgroup.
__global__ __launch_bounds__(kThreads) void pair_dist_bwd_kernel(const float *__restrict__ a, const float *__restrict__ h,
                                                                 const float *__restrict__ E, const float *__restrict__ gout,
                                                                 const float *__restrict__ hyper, const int *__restrict__ count,
                                                                 float *__restrict__ da, float *__restrict__ dh, int B, int R,
                                                                 int D) {
  __shared__ float coef[kThreads];
  const int tid = threadIdx.x, row = blockIdx.y;
  const bool anchor = row < B;
  const int self = anchor ? row : row - B, n = anchor ? R : B;
  const float *own = (anchor ? a : h) + (size_t)self * D, *other = anchor ? h : a;
  const int cnt = count[0];
  const float g = cnt > 0 ? gout[0] * hyper[1] / (float)cnt : 0.f;
  const int d0 = blockIdx.x * kKlChunk + tid;
  float x[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < 4; ++q) {
    const int d = d0 + q * kThreads;
    x[q] = d < D ? own[d] : 0.f;
  }
  for (int base = 0; base < n; base += kThreads) {
    const int u = base + tid;
    coef[tid] = u < n ? (anchor ? E[(size_t)self * R + u] : E[(size_t)u * R + self]) : 0.f;
    __syncthreads();
    const int lim = min(kThreads, n - base);
    for (int j = 0; j < lim; ++j) {
      const float c = coef[j];
      if (c == 0.f) continue;
      const float *o = other + (size_t)(base + j) * D;
      for (int q = 0; q < 4; ++q) {
        const int d = d0 + q * kThreads;
        if (d < D) {
          const float e = anchor ? (x[q] - o[d]) + kEps : (o[d] - x[q]) + kEps;      // a - h + eps either way
          acc[q] += c * e;
        }
      }
    }
    __syncthreads();
  }
  float *out = (anchor ? da : dh) + (size_t)self * D;
  for (int q = 0; q < 4; ++q) {
    const int d = d0 + q * kThreads;
    if (d < D) out[d] = anchor ? -g * acc[q] : g * acc[q];
  }
}

}  // namespace

PCR_EXPORT int pcr_kl_pairs_fwd_f32(const float *h, const int *match, float *lse, float *cross, float *kl, float *loss,
                                    int *counts, int *info, int B, int D, pcr_stream_t stream) {
  if (B < 1 || D < 1 || !h || !match || !lse || !cross || !kl || !loss || !counts || !info) return PCR_ERR_INVALID;
  const int st = pcr_launch<kl_pairs_fwd_kernel>(dim3(B), dim3(kThreads), 0, pcr_s(stream), h, lse, cross, kl, B, D);
  if (st != PCR_OK) return st;
  return pcr_launch<kl_pairs_fin_kernel>(dim3(1), dim3(kThreads), 0, pcr_s(stream), kl, match, loss, counts, info, B);
}

PCR_EXPORT int pcr_kl_pairs_bwd_f32(const float *h, const int *match, const float *lse, const float *cross, const int *counts,
                                    const float *gout, float *dh, int B, int D, pcr_stream_t stream) {
  if (B < 1 || D < 1 || !h || !match || !lse || !cross || !counts || !gout || !dh) return PCR_ERR_INVALID;
  const long long nchunk = ((long long)D + kKlChunk - 1) / kKlChunk;
  if (nchunk * B > 0x7fffffffLL) return PCR_ERR_INVALID;
  return pcr_launch<kl_pairs_bwd_kernel>(dim3((unsigned)(nchunk * B)), dim3(kThreads), 0, pcr_s(stream), h, match, lse, cross,
                                         counts, gout, dh, B, D, (int)nchunk);
}

PCR_EXPORT int pcr_triplet_ok(int B, int T) {
  return B >= 1 && T >= 1 && 2 * (long long)B <= PCR_TRIPLET_MAX_ROWS && (long long)B * T <= 0x7fffffffLL;
}

PCR_EXPORT int pcr_triplet_draw_i32(const int *ids, const int *match, const int *rand, const long long *seed, int *neg,
                                    int *info, int B, int T, pcr_stream_t stream) {
  if (!pcr_triplet_ok(B, T) || !ids || !match || !neg || !info) return PCR_ERR_INVALID;
  return pcr_launch<triplet_draw_kernel>(dim3(B), dim3(kWave), 2 * (size_t)B * sizeof(int), pcr_s(stream), ids, match,
                                         reinterpret_cast<const uint32_t *>(rand),
                                         reinterpret_cast<const unsigned long long *>(seed), neg, info, B, T);
}

PCR_EXPORT int pcr_pair_dist_f32(const float *a, const float *h, float *dist, int B, int R, int D, pcr_stream_t stream) {
  if (B < 1 || R < 1 || D < 1 || !a || !h || !dist) return PCR_ERR_INVALID;
  const int gy = (B + kTile - 1) / kTile;
  if (gy > 65535) return PCR_ERR_INVALID;
  return pcr_launch<pair_dist_kernel>(dim3((R + kTile - 1) / kTile, gy), dim3(kThreads), 0, pcr_s(stream), a, h, dist, B, R, D);
}

PCR_EXPORT int pcr_triplet_select_f32(const float *dist, const int *neg, const int *match, const float *hyper, float *E,
                                      float *pair_loss, float *loss, int *count, int *info, int B, int T,
                                      pcr_stream_t stream) {
  if (!pcr_triplet_ok(B, T) || !dist || !neg || !match || !hyper || !E || !pair_loss || !loss || !count || !info)
    return PCR_ERR_INVALID;
  const int st = pcr_launch<triplet_select_kernel>(dim3(B), dim3(kThreads), 2 * (size_t)B * sizeof(int), pcr_s(stream), dist,
                                                   neg, match, hyper, E, pair_loss, B, T);
  if (st != PCR_OK) return st;
  return pcr_launch<triplet_fin_kernel>(dim3(1), dim3(kThreads), 0, pcr_s(stream), pair_loss, neg, match, hyper, loss, count,
                                        info, B, T);
}

PCR_EXPORT int pcr_pair_dist_bwd_f32(const float *a, const float *h, const float *E, const float *gout, const float *hyper,
                                     const int *count, float *da, float *dh, int B, int R, int D, pcr_stream_t stream) {
  if (B < 1 || R < 1 || D < 1 || !a || !h || !E || !gout || !hyper || !count || !da || !dh) return PCR_ERR_INVALID;
  if ((long long)B + R > 65535) return PCR_ERR_INVALID;
  return pcr_launch<pair_dist_bwd_kernel>(dim3((D + kKlChunk - 1) / kKlChunk, B + R), dim3(kThreads), 0, pcr_s(stream), a, h, E,
                                          gout, hyper, count, da, dh, B, R, D);
}
