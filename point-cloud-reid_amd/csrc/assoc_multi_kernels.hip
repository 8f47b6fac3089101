// Association with any set of decisions per side (include/pcr.h, section A3, "Any set of decisions"): the (T + dd*D,
// D + td*T) cost matrix by the margin or the softmax rule, the cheapest-decision reduction, and the decode of the solved
// assignment into per-object decisions and the born / kill masks.  Fixed-shape launches without a host read.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the margin matrix is compared bit for bit with
// pcr_assoc_cost_f32's and with the CPU restatement (tests/decisions_ref.py).
#include "pcr_common.h"

#include <climits>

namespace {

constexpr int kDecodeThreads = 1024;                               // one column (or row) of the matrix per thread
constexpr int kDecodeWaves = kDecodeThreads / kWave;
static_assert(PCR_LSA_MAX <= kDecodeThreads, "the decode keeps one row and one column per thread");

// decision i of object o (n objects, nd decisions); under reduce the cheapest one, ties to the lowest index
__device__ __forceinline__ float decision_value(const float *__restrict__ dec, int n, int nd, int i, int o, int reduce,
                                                int *__restrict__ choice) {
  if (!reduce) return dec ? dec[(size_t)i * n + o] : 0.f;
  float best = dec ? dec[o] : 0.f;
  int bi = 0;
  for (int k = 1; k < nd; ++k) {
    const float x = dec ? dec[(size_t)k * n + o] : 0.f;
    if (x < best) best = x, bi = k;
  }
  if (choice) choice[o] = bi;
  return best;
}

// margin: everything but the listed pairs -- fill and the decision diagonals (dd, td: the caller's counts; de, te: the
// diagonal blocks per side, which reduce makes one)
__global__ __launch_bounds__(256) void multi_fill_kernel(const float *__restrict__ det_dec, const float *__restrict__ trk_dec,
                                                         float fill, float *__restrict__ cost, int *__restrict__ det_choice,
                                                         int *__restrict__ trk_choice, int T, int D, int dd, int td, int de,
                                                         int te, int reduce) {
  const int C = D + te * T, r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float x = fill;
  if (r < T) {
    if (c >= D) {
      const int q = c - D, j = q / T, t = q - j * T;
      if (t == r) x = decision_value(trk_dec, T, td, j, t, reduce, trk_choice);
    }
  } else if (c < D) {
    const int q = r - T, i = q / D, d = q - i * D;
    if (d == c) x = decision_value(det_dec, D, dd, i, d, reduce, det_choice);
  }
  cost[(size_t)r * C + c] = x;
}

// margin: listed pair k -> (t, d) of the top-left block and (d, t) of every bottom-right block
__global__ __launch_bounds__(256) void multi_pairs_kernel(const float *__restrict__ logits, const int *__restrict__ pairs,
                                                          const int *__restrict__ count, const float *__restrict__ dist,
                                                          float dist_max, float dist_penalty, float *__restrict__ cost,
                                                          int T, int D, int de, int te, int cap) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cap || k >= count[0]) return;
  const int t = pairs[2 * (size_t)k], d = pairs[2 * (size_t)k + 1];
  if (t < 0 || t >= T || d < 0 || d >= D) return;
  float x = -logits[k];
  if (dist && dist[(size_t)t * D + d] > dist_max) x = x + dist_penalty;
  const size_t C = (size_t)D + (size_t)te * T;
  cost[(size_t)t * C + d] = x;
  for (int i = 0; i < de; ++i)
    for (int j = 0; j < te; ++j) cost[((size_t)T + (size_t)i * D + d) * C + D + (size_t)j * T + t] = x;
}

// ---- softmax ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smx_clear_kernel(float *__restrict__ score, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) score[e] = -__builtin_inff();
}

__global__ __launch_bounds__(256) void smx_scatter_kernel(const float *__restrict__ logits, const int *__restrict__ pairs,
                                                          const int *__restrict__ count, float *__restrict__ score, int T,
                                                          int D, int cap) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cap || k >= count[0]) return;
  const int t = pairs[2 * (size_t)k], d = pairs[2 * (size_t)k + 1];
  if (t < 0 || t >= T || d < 0 || d >= D) return;
  score[(size_t)t * D + d] = logits[k];
}

// One wave per track (blocks 0 .. T-1) and per detection (blocks T .. T+D-1): the maximum and the sum of exp(x - max) of
// its set, in pcr.h's order.  stats = rmax (T), rsum (T), cmax (D), csum (D).
__global__ __launch_bounds__(kWave) void smx_stats_kernel(const float *__restrict__ score, const float *__restrict__ det_dec,
                                                          const float *__restrict__ trk_dec, double *__restrict__ stats,
                                                          int T, int D, int dd, int td) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool row = b < T;
  const int o = row ? b : b - T;
  const int n = row ? D : T, nd = row ? td : dd, no = row ? T : D;
  const float *dec = row ? trk_dec : det_dec;
  const float ninf = -__builtin_inff();
  auto elem = [&](int e) -> float {
    if (e < n) return row ? score[(size_t)o * D + e] : score[(size_t)e * D + o];
    return dec ? dec[(size_t)(e - n) * no + o] : 0.f;
  };
  float m = ninf;
  for (int e = lane; e < n + nd; e += kWave) {
    const float x = elem(e);
    if (x > m) m = x;                                    // (a NaN never enters m; it reaches the sum below)
  }
#pragma unroll
  for (int off = kWave / 2; off; off >>= 1) {
    const float om = __shfl_xor(m, off, kWave);
    if (om > m) m = om;
  }
  double s = 0.0;
  for (int e = lane; e < n + nd; e += kWave) {
    const float x = elem(e);
    if (x != ninf) s = s + exp((double)x - (double)m);
  }
#pragma unroll
  for (int off = kWave / 2; off; off >>= 1) s = s + __shfl_xor(s, off, kWave);
  if (lane == 0) {
    double *mx = row ? stats : stats + 2 * (size_t)T, *sm = row ? stats + T : stats + 2 * (size_t)T + D;
    mx[o] = (double)m;
    sm[o] = s;
  }
}

__global__ __launch_bounds__(256) void smx_fill_kernel(const float *__restrict__ score, const float *__restrict__ det_dec,
                                                       const float *__restrict__ trk_dec,
                                                       const double *__restrict__ stats, float fill,
                                                       float *__restrict__ cost, int T, int D, int dd, int td) {
  const int C = D + td * T, r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double *rmax = stats, *rsum = stats + T, *cmax = stats + 2 * (size_t)T, *csum = stats + 2 * (size_t)T + D;
  float x = fill;
  if (r < T && c >= D) {
    const int q = c - D, j = q / T, t = q - j * T;
    if (t == r) {
      const float v = trk_dec ? trk_dec[(size_t)j * T + t] : 0.f;
      x = -(float)(exp((double)v - rmax[t]) / rsum[t]);
    }
  } else if (r >= T && c < D) {
    const int q = r - T, i = q / D, d = q - i * D;
    if (d == c) {
      const float v = det_dec ? det_dec[(size_t)i * D + d] : 0.f;
      x = -(float)(exp((double)v - cmax[d]) / csum[d]);
    }
  } else {                                                // a pair: the top-left block, or its transpose
    const int t = r < T ? r : (c - D) % T, d = r < T ? c : (r - T) % D;
    const float s = score[(size_t)t * D + d];
    if (s != -__builtin_inff()) {
      const double pr = exp((double)s - rmax[t]) / rsum[t], pc = exp((double)s - cmax[d]) / csum[d];
      x = -(float)((pr > pc || pr != pr) ? pr : pc);
    }
  }
  cost[(size_t)r * C + c] = x;
}

// ---- decode -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool cand_better(float av, int ai, float bv, int bi) {
  return av < bv || (av == bv && ai < bi);
}

// the least (value, index) over the workgroup, ties to the lowest index; i == INT_MAX: nobody had a candidate.  Two
// barriers; every thread gets the result.
__device__ __forceinline__ void block_argmin(float &v, int &i, float *sv, int *si) {
#pragma unroll
  for (int off = kWave / 2; off; off >>= 1) {
    const float ov = __shfl_xor(v, off, kWave);
    const int oi = __shfl_xor(i, off, kWave);
    if (cand_better(ov, oi, v, i)) v = ov, i = oi;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) sv[threadIdx.x >> 6] = v, si[threadIdx.x >> 6] = i;
  __syncthreads();
  v = sv[0], i = si[0];
  for (int w = 1; w < kDecodeWaves; ++w)
    if (cand_better(sv[w], si[w], v, i)) v = sv[w], i = si[w];
  __syncthreads();
}

__global__ __launch_bounds__(kDecodeThreads) void assoc_decode_kernel(pcr_assoc_decode p) {
  __shared__ int c4r[PCR_LSA_MAX], r4c[PCR_LSA_MAX];
  __shared__ float sv[kDecodeWaves];
  __shared__ int si[kDecodeWaves], cnt[4];
  const int tid = threadIdx.x, T = p.T, D = p.D;
  const int de = p.reduce ? (p.dd > 0) : p.dd, te = p.reduce ? (p.td > 0) : p.td;
  const int R = T + de * D, C = D + te * T;
  const float fill = p.fill, inf = __builtin_inff();
  const int sinfo = p.solver_info ? p.solver_info[0] : 0;
  const float *__restrict__ cost = p.cost;
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();

  // void and drop, seen from the rows and from the columns
  for (int r = tid; r < R; r += kDecodeThreads) {
    int c = sinfo ? -1 : p.col4row[r];
    if (c < 0 || c >= C) c = -1;
    if (c >= 0) {
      const bool is_void = cost[(size_t)r * C + c] == fill;
      if (is_void) atomicAdd(&cnt[1], 1);
      if (is_void || (te > 0 && r >= T && c >= D)) c = -1;
    }
    c4r[r] = c;
  }
  for (int c = tid; c < C; c += kDecodeThreads) {
    int r = sinfo ? -1 : p.row4col[c];
    if (r < 0 || r >= R) r = -1;
    if (r >= 0 && (cost[(size_t)r * C + c] == fill || (te > 0 && r >= T && c >= D))) r = -1;
    r4c[c] = r;
  }
  __syncthreads();

  if (te > 0 && !sinfo) {
    for (int t = 0; t < T; ++t) {                         // (c4r[t] is written in its own turn only: the test is uniform)
      if (c4r[t] >= 0) continue;
      float v = inf;
      int i = INT_MAX;
      if (tid < C && r4c[tid] < 0) v = cost[(size_t)t * C + tid], i = tid;
      block_argmin(v, i, sv, si);
      if (i != INT_MAX && v != fill && tid == 0) c4r[t] = i, r4c[i] = t, cnt[2] += 1;
      __syncthreads();
    }
    for (int d = 0; d < D; ++d) {
      if (r4c[d] >= 0) continue;
      float v = inf;
      int i = INT_MAX;
      if (tid < R && c4r[tid] < 0) v = cost[(size_t)tid * C + d], i = tid;
      block_argmin(v, i, sv, si);
      if (i != INT_MAX && v != fill && tid == 0) r4c[d] = i, c4r[i] = d, cnt[3] += 1;
      __syncthreads();
    }
  }

  for (int t = tid; t < T; t += kDecodeThreads) {
    const int c = c4r[t];
    int dec = 1 + p.td, to = -1;
    if (c >= 0 && c < D) dec = 0, to = c;
    else if (c >= D) dec = 1 + (p.reduce ? p.trk_choice[t] : (c - D) / T);
    p.track_to_det[t] = to;
    p.track_decision[t] = dec;
    p.kill[t] = (p.kill_dec >= 0 && dec == 1 + p.kill_dec) ? 1 : 0;
  }
  for (int d = tid; d < D; d += kDecodeThreads) {
    const int r = r4c[d];
    int dec = 1 + p.dd, to = -1;
    if (r >= 0 && r < T) dec = 0, to = r;
    else if (r >= T) dec = 1 + (p.reduce ? p.det_choice[d] : (r - T) / D);
    p.det_to_track[d] = to;
    p.det_decision[d] = dec;
    p.born[d] = (p.born_dec >= 0 && dec == 1 + p.born_dec) ? 1 : 0;
  }
  if (tid == 0) {
    p.info[0] = sinfo;
    p.info[1] = cnt[1], p.info[2] = cnt[2], p.info[3] = cnt[3];
  }
}

struct MultiShape {
  int de, te, R, C;
};

MultiShape multi_shape(int T, int D, int dd, int td, int reduce) {
  MultiShape s;
  s.de = reduce ? (dd > 0) : dd, s.te = reduce ? (td > 0) : td;
  s.R = T + s.de * D, s.C = D + s.te * T;
  return s;
}

}  // namespace

PCR_EXPORT int pcr_assoc_multi_ok(int T, int D, int dd, int td, int cap) {
  if (T < 0 || D < 0 || T > PCR_LSA_MAX || D > PCR_LSA_MAX) return 0;
  if (dd < 0 || dd > PCR_ASSOC_MAX_DECISIONS || td < 0 || td > PCR_ASSOC_MAX_DECISIONS) return 0;
  if (T + dd * D > PCR_LSA_MAX || D + td * T > PCR_LSA_MAX) return 0;
  if (cap < 0 || cap > T * D) return 0;
  return 1;
}

PCR_EXPORT int pcr_assoc_multi_ws_bytes(int T, int D, int dd, int td) {
  if (!pcr_assoc_multi_ok(T, D, dd, td, 0)) return 0;
  return (int)(2 * sizeof(double) * ((size_t)T + D) + sizeof(float) * (size_t)T * D);      // <= 32 KiB + 4 MiB
}

PCR_EXPORT int pcr_assoc_cost_multi_f32(const pcr_assoc_multi *p, pcr_stream_t stream) {
  if (!p || !pcr_assoc_multi_ok(p->T, p->D, p->dd, p->td, p->cap)) return PCR_ERR_INVALID;
  if ((p->kind != PCR_COST_MARGIN && p->kind != PCR_COST_SOFTMAX) || (p->reduce != 0 && p->reduce != 1)) return PCR_ERR_INVALID;
  if (p->kind == PCR_COST_SOFTMAX && (p->dist || p->reduce)) return PCR_ERR_INVALID;
  const int T = p->T, D = p->D, cap = p->cap;
  const MultiShape s = multi_shape(T, D, p->dd, p->td, p->reduce);
  if (s.R == 0 || s.C == 0) return PCR_OK;
  const bool listed = T > 0 && D > 0 && cap > 0;
  if (!p->cost || (listed && (!p->logits || !p->pairs || !p->count))) return PCR_ERR_INVALID;
  if (p->reduce && ((p->dd > 0 && D > 0 && !p->det_choice) || (p->td > 0 && T > 0 && !p->trk_choice))) return PCR_ERR_INVALID;
  hipStream_t st = pcr_s(stream);
  const dim3 grid((s.C + 255) / 256, s.R);
  if (p->kind == PCR_COST_MARGIN) {
    int rc = pcr_launch<multi_fill_kernel>(grid, dim3(256), 0, st, p->det_dec, p->trk_dec, p->fill, p->cost, p->det_choice,
                                           p->trk_choice, T, D, p->dd, p->td, s.de, s.te, p->reduce);
    if (rc != PCR_OK || !listed) return rc;
    return pcr_launch<multi_pairs_kernel>(dim3((cap + 255) / 256), dim3(256), 0, st, p->logits, p->pairs, p->count, p->dist,
                                          p->dist_max, p->dist_penalty, p->cost, T, D, s.de, s.te, cap);
  }
  if (!p->ws) return PCR_ERR_INVALID;
  double *stats = static_cast<double *>(p->ws);            // rmax (T), rsum (T), cmax (D), csum (D), then the score image
  float *score = reinterpret_cast<float *>(stats + 2 * ((size_t)T + D));
  int rc = PCR_OK;
  if (T > 0 && D > 0) rc = pcr_launch<smx_clear_kernel>(dim3((T * D + 255) / 256), dim3(256), 0, st, score, T * D);
  if (rc == PCR_OK && listed)
    rc = pcr_launch<smx_scatter_kernel>(dim3((cap + 255) / 256), dim3(256), 0, st, p->logits, p->pairs, p->count, score, T, D,
                                        cap);
  if (rc == PCR_OK)
    rc = pcr_launch<smx_stats_kernel>(dim3(T + D), dim3(kWave), 0, st, score, p->det_dec, p->trk_dec, stats, T, D, p->dd,
                                      p->td);
  if (rc != PCR_OK) return rc;
  return pcr_launch<smx_fill_kernel>(grid, dim3(256), 0, st, score, p->det_dec, p->trk_dec, stats, p->fill, p->cost, T, D,
                                     p->dd, p->td);
}

PCR_EXPORT int pcr_assoc_decode_i32(const pcr_assoc_decode *p, pcr_stream_t stream) {
  if (!p || !pcr_assoc_multi_ok(p->T, p->D, p->dd, p->td, 0)) return PCR_ERR_INVALID;
  if (p->reduce != 0 && p->reduce != 1) return PCR_ERR_INVALID;
  if (p->born_dec >= p->dd || p->kill_dec >= p->td) return PCR_ERR_INVALID;
  const int T = p->T, D = p->D;
  if (T + D == 0) return PCR_OK;
  const MultiShape s = multi_shape(T, D, p->dd, p->td, p->reduce);
  if (!p->info || (s.R > 0 && !p->col4row) || (s.C > 0 && !p->row4col) || (s.R > 0 && s.C > 0 && !p->cost)) return PCR_ERR_INVALID;
  if (T > 0 && (!p->track_to_det || !p->track_decision || !p->kill)) return PCR_ERR_INVALID;
  if (D > 0 && (!p->det_to_track || !p->det_decision || !p->born)) return PCR_ERR_INVALID;
  if (p->reduce && ((p->dd > 0 && D > 0 && !p->det_choice) || (p->td > 0 && T > 0 && !p->trk_choice))) return PCR_ERR_INVALID;
  return pcr_launch<assoc_decode_kernel>(dim3(1), dim3(kDecodeThreads), 0, pcr_s(stream), *p);
}
