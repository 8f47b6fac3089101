// Track / detection association (include/pcr.h, section A3): the class-gated pair list, the augmented cost matrix and
// the rectangular linear sum assignment, each a fixed-shape launch without a host read.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the solver's values are defined operation by operation in
// pcr.h and compared bit for bit with the CPU restatement (tests/assoc_ref.py).
#include "pcr_common.h"

namespace {

constexpr int kPairThreads = 1024;                                  // 16 waves share the label chunks
constexpr int kPairChunks = PCR_ASSOC_MAX_OBJECTS / kWave;          // 64-object chunks per side
constexpr int kPairClasses = PCR_ASSOC_MAX_CLASSES;
constexpr int kPairSlotsPerBlock = kPairThreads * 8;

// the class of object i if it takes part, -1 otherwise
__device__ __forceinline__ int pair_class(const int *__restrict__ labels, const int *__restrict__ lengths, int i, int n,
                                          int ncls, int min_points) {
  if (i >= n) return -1;
  const int x = labels[i];
  if (x < 0 || x >= ncls) return -1;
  if (lengths && lengths[i] < min_points) return -1;
  return x;
}

// Every workgroup sorts the T tracks and the D detections by class (stable: a count per 64-object chunk and class from
// ballots, an exclusive scan over the chunks, the rank inside a chunk from the ballot again) and then fills its share
// of the cap output slots: slot k -> its class by the pair bases, then (k - base) / nd and % nd name the track and the
// detection of that rank.  The sort is redundant across workgroups (<= 8192 labels) and costs less than a second launch.
__global__ __launch_bounds__(kPairThreads) void assoc_pairs_kernel(const int *__restrict__ tl, const int *__restrict__ dl,
                                                                   const int *__restrict__ tlen,
                                                                   const int *__restrict__ dlen, int *__restrict__ pairs,
                                                                   int *__restrict__ count, int T, int D, int ncls,
                                                                   int min_points, int cap) {
  __shared__ int cnt[2][kPairChunks][kPairClasses];
  __shared__ int ntot[2][kPairClasses], cbase[2][kPairClasses], pbase[kPairClasses + 1];
  __shared__ int list[2][PCR_ASSOC_MAX_OBJECTS];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  constexpr int nw = kPairThreads / kWave;
  const int n[2] = {T, D};
  const int *const lab[2] = {tl, dl};
  const int *const len[2] = {tlen, dlen};

#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int nch = (n[s] + kWave - 1) / kWave;
    for (int c = wave; c < nch; c += nw) {
      const int x = pair_class(lab[s], len[s], c * kWave + lane, n[s], ncls, min_points);
      int mine = 0;
      for (int cls = 0; cls < ncls; ++cls) {
        const int k = __popcll(__ballot(x == cls));
        if (lane == cls) mine = k;
      }
      if (lane < kPairClasses) cnt[s][c][lane] = mine;
    }
  }
  __syncthreads();
  if (tid < 2 * kPairClasses) {
    const int s = tid / kPairClasses, cls = tid % kPairClasses;
    const int nch = (n[s] + kWave - 1) / kWave;
    int run = 0;
    if (cls < ncls)
      for (int c = 0; c < nch; ++c) {
        const int t = cnt[s][c][cls];
        cnt[s][c][cls] = run;
        run += t;
      }
    ntot[s][cls] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int b0 = 0, b1 = 0, pb = 0;
    for (int cls = 0; cls < kPairClasses; ++cls) {
      cbase[0][cls] = b0, cbase[1][cls] = b1, pbase[cls] = pb;
      b0 += ntot[0][cls], b1 += ntot[1][cls];
      pb += ntot[0][cls] * ntot[1][cls];                 // <= 4096 * 4096 in all
    }
    pbase[kPairClasses] = pb;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int nch = (n[s] + kWave - 1) / kWave;
    for (int c = wave; c < nch; c += nw) {
      const int i = c * kWave + lane;
      const int x = pair_class(lab[s], len[s], i, n[s], ncls, min_points);
      int rank = 0;
      for (int cls = 0; cls < ncls; ++cls) {
        const unsigned long long bal = __ballot(x == cls);
        const int r = (int)pcr_lanes_below(bal);
        if (x == cls) rank = r;
      }
      if (x >= 0) list[s][cbase[s][x] + cnt[s][c][x] + rank] = i;
    }
  }
  __syncthreads();

  const int total = pbase[kPairClasses];
  if (blockIdx.x == 0 && tid == 0) count[0] = total;
  const int listed = min(total, cap);
  for (int k = blockIdx.x * kPairThreads + tid; k < cap; k += gridDim.x * kPairThreads) {
    int t = 0, d = 0;
    if (k < listed) {
      int lo = 0, hi = ncls - 1;                          // the largest class whose pair base is <= k: it is not empty
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pbase[mid] <= k) lo = mid;
        else hi = mid - 1;
      }
      const int q = k - pbase[lo], nd = ntot[1][lo];
      const int tr = q / nd;
      t = list[0][cbase[0][lo] + tr];
      d = list[1][cbase[1][lo] + (q - tr * nd)];
    }
    pairs[2 * (size_t)k] = t;
    pairs[2 * (size_t)k + 1] = d;
  }
}

// everything but the listed pairs: fill and the two decision diagonals
__global__ __launch_bounds__(256) void assoc_cost_fill_kernel(const float *__restrict__ track_miss,
                                                              const float *__restrict__ det_new, float fill,
                                                              float *__restrict__ cost, int T, int D) {
  const int N = T + D, r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float x = fill;
  if (r < T) {
    if (c - D == r) x = track_miss ? track_miss[r] : 0.f;
  } else if (c == r - T) {
    x = det_new ? det_new[c] : 0.f;
  }
  cost[(size_t)r * N + c] = x;
}

// listed pair k -> (t, d) of the top-left block and (d, t) of the bottom-right one
__global__ __launch_bounds__(256) void assoc_cost_pairs_kernel(const float *__restrict__ logits,
                                                               const int *__restrict__ pairs,
                                                               const int *__restrict__ count,
                                                               const float *__restrict__ dist, float dist_max,
                                                               float dist_penalty, float *__restrict__ cost, int T, int D,
                                                               int cap) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cap || k >= count[0]) return;
  const int t = pairs[2 * (size_t)k], d = pairs[2 * (size_t)k + 1];
  if (t < 0 || t >= T || d < 0 || d >= D) return;
  float x = -logits[k];
  if (dist && dist[(size_t)t * D + d] > dist_max) x = x + dist_penalty;
  const size_t N = (size_t)T + D;
  cost[(size_t)t * N + d] = x;
  cost[((size_t)T + d) * N + D + t] = x;
}

// ---- linear sum assignment ----------------------------------------------------------------------------------------
// How a search step reads entry (i, jj) of the SOLVED problem (nr <= nc rows i, columns jj).  Each reader keeps one
// address space: LDS for the staged matrix, global for the other two.
struct LsaLdsRows {                                       // the staged (nr, nc) copy
  const float *cl;
  int nc;
  __device__ __forceinline__ float operator()(int i, int jj) const { return cl[i * nc + jj]; }
};
struct LsaGlobalRows {                                    // the caller's (R, C) matrix, transposed on the way if tr
  const float *cb;
  int C;
  bool tr;
  __device__ __forceinline__ float operator()(int i, int jj) const {
    return tr ? cb[(size_t)jj * C + i] : cb[(size_t)i * C + jj];
  }
};
struct LsaGatherRows {                                    // a block of the caller's matrix through its two LDS index lists
  const float *cb;
  const int *ri, *ci;                                     // original indices of the solved problem's rows / columns
  int C;
  bool tr;
  __device__ __forceinline__ float operator()(int i, int jj) const {
    const int a = ri[i], b = ci[jj];
    return tr ? cb[(size_t)b * C + a] : cb[(size_t)a * C + b];
  }
};

// The ONE copy of the solver: search, dual update and augmentation over the solved problem (nr <= nc), by one wave.
// NK = columns per lane (column j = k * 64 + lane): v and r4c come back in registers, u and c4r (nr each) in LDS.
// status is what the pre-scan found; the return value is the problem's info.  The rules are pcr.h's, in its words.
template <int NK, class Rows>
__device__ __forceinline__ int lsa_solve(const Rows &entry, float *u, int *c4r, int nr, int nc, int lane, int status,
                                         float (&v)[NK], int (&r4c)[NK]) {
  const float inf = __builtin_inff();
  float sh[NK];
  int pr[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) v[k] = 0.f, r4c[k] = -1, sh[k] = inf, pr[k] = -1;
  for (int i = lane; i < nr; i += kWave) u[i] = 0.f, c4r[i] = -1;
  wave_sync();

  for (int cur = 0; cur < nr && status == 0; ++cur) {
#pragma unroll
    for (int k = 0; k < NK; ++k) sh[k] = inf, pr[k] = -1;
    uint32_t done = 0;
    float minv = 0.f;
    int i = cur, sink = -1;
    for (int step = 0; step < nc; ++step) {
      const float ui = u[i];
      float cv[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        cv[k] = 0.f;
        if (k * kWave < nc) cv[k] = entry(i, min(k * kWave + lane, nc - 1));
      }
      float lmin = inf;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (k * kWave + lane < nc && !((done >> k) & 1u)) {
          const float a = cv[k] - ui;
          const float d = a - v[k];
          const float r = d + minv;
          if (r < sh[k]) sh[k] = r, pr[k] = i;
          lmin = sh[k] < lmin ? sh[k] : lmin;
        }
      }
      const float gmin = wave_reduce<true>(lmin, WaveMin());   // (no NaN among the operands)
      int j = -1, ri = -1;
      float mv = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (j < 0 && k * kWave < nc) {
          const unsigned long long bal = __ballot(k * kWave + lane < nc && !((done >> k) & 1u) && sh[k] == gmin);
          if (bal) {
            const int owner = __builtin_amdgcn_readfirstlane(__ffsll((long long)bal) - 1);
            j = k * kWave + owner;
            mv = wave_readlane(sh[k], owner);
            ri = __builtin_amdgcn_readlane(r4c[k], owner);
            if (lane == owner) done |= 1u << k;
          }
        }
      }
      if (j < 0) break;                                   // no candidate compares equal to the minimum: overflow
      minv = mv;
      if (ri < 0) {
        sink = j;
        break;
      }
      i = ri;
    }
    if (sink < 0) {
      status = 2;
      break;
    }

    if (lane == 0) u[cur] = u[cur] + minv;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if ((done >> k) & 1u) {
        const float d = minv - sh[k];
        if (r4c[k] >= 0) u[r4c[k]] = u[r4c[k]] + d;       // every done column but the sink has a row, each its own
        v[k] = v[k] - d;
      }
    }
    wave_sync();

    int j = sink;
    for (int s = 0; s <= cur; ++s) {
      const int owner = j & (kWave - 1), slot = j >> 6;
      int i2 = -1;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (k == slot) {
          i2 = __builtin_amdgcn_readlane(pr[k], owner);
          if (lane == owner) r4c[k] = i2;
        }
      }
      if (i2 < 0) {
        status = 2;
        break;
      }
      const int jn = __builtin_amdgcn_readfirstlane(c4r[i2]);
      wave_sync();
      if (lane == 0) c4r[i2] = j;
      wave_sync();
      if (i2 == cur) break;
      j = jn;
      if (j < 0) {
        status = 2;
        break;
      }
    }
  }
  wave_sync();
  return status;
}

// One wave per problem; STAGED: the matrix is copied to LDS (as the solved problem's rows) and read from there.
template <int NK, bool STAGED>
__global__ __launch_bounds__(kWave) void lsa_kernel(const float *__restrict__ cost, int *__restrict__ col4row_o,
                                                    int *__restrict__ row4col_o, float *__restrict__ u_o,
                                                    float *__restrict__ v_o, int *__restrict__ info, int R, int C) {
  extern __shared__ float lsa_lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool tr = R > C;
  const int nr = tr ? C : R, nc = tr ? R : C;             // the solved problem: nr <= nc
  float *u = lsa_lds;
  int *c4r = reinterpret_cast<int *>(lsa_lds + nr);
  float *cl = lsa_lds + 2 * nr;                           // (nr, nc) when STAGED
  const float *cb = cost + (size_t)b * R * C;

  bool bad = false;
  for (int e = lane; e < R * C; e += kWave) {
    const float x = cb[e];
    bad |= (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u;
    if constexpr (STAGED) {
      if (tr) {
        const int r0 = e / C;
        cl[(e - r0 * C) * nc + r0] = x;
      } else {
        cl[e] = x;
      }
    }
  }
  int status = __ballot(bad) ? 1 : 0;

  float v[NK];
  int r4c[NK];
  if constexpr (STAGED) status = lsa_solve<NK>(LsaLdsRows{cl, nc}, u, c4r, nr, nc, lane, status, v, r4c);
  else status = lsa_solve<NK>(LsaGlobalRows{cb, C, tr}, u, c4r, nr, nc, lane, status, v, r4c);

  // the transposed problem's rows are the caller's columns
  int *rows_o = tr ? row4col_o + (size_t)b * C : col4row_o + (size_t)b * R;
  int *cols_o = tr ? col4row_o + (size_t)b * R : row4col_o + (size_t)b * C;
  float *ur_o = tr ? (v_o ? v_o + (size_t)b * C : nullptr) : (u_o ? u_o + (size_t)b * R : nullptr);
  float *vc_o = tr ? (u_o ? u_o + (size_t)b * R : nullptr) : (v_o ? v_o + (size_t)b * C : nullptr);
  const bool ok = status == 0;
  for (int i = lane; i < nr; i += kWave) {
    rows_o[i] = ok ? c4r[i] : -1;
    if (ur_o) ur_o[i] = ok ? u[i] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int j = k * kWave + lane;
    if (j < nc) {
      cols_o[j] = ok ? r4c[k] : -1;
      if (vc_o) vc_o[j] = ok ? v[k] : 0.f;
    }
  }
  if (lane == 0) info[b] = status;
}

// One wave per BLOCK of one (R, C) problem (pcr.h, "the block rule"): compact the block's rows and columns into two LDS
// index lists (ascending: a ballot over 64 ids, the rank from mbcnt), gather the sub-matrix through them -- into LDS when
// it fits beside the lists (lds_words is what the launch asked for), with the pre-scan folded in -- solve it with
// lsa_solve and scatter the results through the lists.  Wave 0 also writes the rows and columns outside every block.
template <int NK>
__global__ __launch_bounds__(kWave) void lsa_blocks_kernel(const float *__restrict__ cost, const int *__restrict__ row_block,
                                                           const int *__restrict__ col_block, int *__restrict__ col4row_o,
                                                           int *__restrict__ row4col_o, float *__restrict__ u_o,
                                                           float *__restrict__ v_o, int *__restrict__ info, int R, int C,
                                                           int G, int lds_words) {
  extern __shared__ float lsa_lds[];
  const int g = blockIdx.x, lane = threadIdx.x;
  int *lists = reinterpret_cast<int *>(lsa_lds);          // [0, R): the block's rows, [R, R + C): its columns
  int n[2] = {0, 0};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int len = s ? C : R;
    const int *ids = s ? col_block : row_block;
    int *list = lists + (s ? R : 0), *idx_o = s ? row4col_o : col4row_o;
    float *dual_o = s ? v_o : u_o;
    for (int c0 = 0; c0 < len; c0 += kWave) {
      const int i = c0 + lane;
      const int id = i < len ? ids[i] : g - 1;            // past the end: neither this block nor outside every block
      const unsigned long long bal = __ballot(i < len && id == g);
      if (i < len && id == g) list[n[s] + (int)pcr_lanes_below(bal)] = i;
      n[s] += __popcll(bal);
      if (g == 0 && i < len && (id < 0 || id >= G)) {
        idx_o[i] = -1;
        if (dual_o) dual_o[i] = 0.f;
      }
    }
  }
  wave_sync();

  const bool tr = n[0] > n[1];
  const int nr = tr ? n[1] : n[0], nc = tr ? n[0] : n[1];  // the solved problem: nr <= nc
  const int *ri = lists + (tr ? R : 0), *ci = lists + (tr ? 0 : R);
  float *u = lsa_lds + R + C;
  int *c4r = reinterpret_cast<int *>(u + nr);
  float *cl = u + 2 * nr;                                 // (nr, nc) when it fits
  const bool staged = R + C + 2 * nr + nr * nc <= lds_words;

  bool bad = false;
  for (int e = lane; e < nr * nc; e += kWave) {
    const int i = e / nc, a = ri[i], b = ci[e - i * nc];
    const float x = tr ? cost[(size_t)b * C + a] : cost[(size_t)a * C + b];
    bad |= (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u;
    if (staged) cl[e] = x;
  }
  int status = __ballot(bad) ? 1 : 0;

  float v[NK];
  int r4c[NK];
  if (staged) status = lsa_solve<NK>(LsaLdsRows{cl, nc}, u, c4r, nr, nc, lane, status, v, r4c);
  else status = lsa_solve<NK>(LsaGatherRows{cost, ri, ci, C, tr}, u, c4r, nr, nc, lane, status, v, r4c);

  int *rows_o = tr ? row4col_o : col4row_o, *cols_o = tr ? col4row_o : row4col_o;
  float *ur_o = tr ? v_o : u_o, *vc_o = tr ? u_o : v_o;
  const bool ok = status == 0;
  for (int i = lane; i < nr; i += kWave) {
    const int j = c4r[i];
    rows_o[ri[i]] = ok && j >= 0 ? ci[j] : -1;
    if (ur_o) ur_o[ri[i]] = ok ? u[i] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int j = k * kWave + lane;
    if (j < nc) {
      cols_o[ci[j]] = ok && r4c[k] >= 0 ? ri[r4c[k]] : -1;
      if (vc_o) vc_o[ci[j]] = ok ? v[k] : 0.f;
    }
  }
  if (lane == 0) info[g] = status;
}

// row / column -> block id of the (T + de*D, D + te*T) layout: an object's label in [0, ncls), the rest block ncls otherwise
__global__ __launch_bounds__(256) void assoc_blocks_kernel(const int *__restrict__ tl, const int *__restrict__ dl,
                                                           int *__restrict__ row_block, int *__restrict__ col_block, int T,
                                                           int D, int R, int C, int ncls) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R) {
    const int x = i < T ? tl[i] : dl[(i - T) % D];
    row_block[i] = x >= 0 && x < ncls ? x : ncls;
  }
  if (i < C) {
    const int x = i < D ? dl[i] : tl[(i - D) % T];
    col_block[i] = x >= 0 && x < ncls ? x : ncls;
  }
}

template <int NK>
int lsa_launch(const float *cost, int *col4row, int *row4col, float *u, float *v, int *info, int B, int R, int C,
               hipStream_t st) {
  const size_t nr = (size_t)(R < C ? R : C), words = 2 * nr + (size_t)R * C;
  if (words * sizeof(float) <= (size_t)kMaxDynLds)
    return pcr_launch_lds<lsa_kernel<NK, true>>(dim3(B), dim3(kWave), words * sizeof(float), st, cost, col4row, row4col, u,
                                                v, info, R, C);
  return pcr_launch_lds<lsa_kernel<NK, false>>(dim3(B), dim3(kWave), 2 * nr * sizeof(float), st, cost, col4row, row4col, u,
                                               v, info, R, C);
}

template <int NK>
int lsa_blocks_launch(const float *cost, const int *row_block, const int *col_block, int *col4row, int *row4col, float *u,
                      float *v, int *info, int R, int C, int G, hipStream_t st) {
  // block sizes are device data: the LDS a largest block (all of R x C) could use, capped
  const size_t nr = (size_t)(R < C ? R : C), want = (size_t)R + C + 2 * nr + (size_t)R * C;
  const size_t words = want * sizeof(float) <= (size_t)kMaxDynLds ? want : (size_t)kMaxDynLds / sizeof(float);
  return pcr_launch_lds<lsa_blocks_kernel<NK>>(dim3(G), dim3(kWave), words * sizeof(float), st, cost, row_block, col_block,
                                               col4row, row4col, u, v, info, R, C, G, (int)words);
}

}  // namespace

PCR_EXPORT int pcr_assoc_pairs_ok(int T, int D, int num_classes, int cap) {
  if (T < 0 || T > PCR_ASSOC_MAX_OBJECTS || D < 0 || D > PCR_ASSOC_MAX_OBJECTS) return 0;
  if (num_classes < 1 || num_classes > PCR_ASSOC_MAX_CLASSES) return 0;
  if (cap < 0 || cap > PCR_ASSOC_MAX_OBJECTS * PCR_ASSOC_MAX_OBJECTS) return 0;
  return 1;
}

PCR_EXPORT int pcr_assoc_pairs_i32(const int *track_labels, const int *det_labels, const int *track_lengths,
                                   const int *det_lengths, int *pairs, int *count, int T, int D, int num_classes,
                                   int min_points, int cap, pcr_stream_t stream) {
  if (!pcr_assoc_pairs_ok(T, D, num_classes, cap)) return PCR_ERR_INVALID;
  if (T == 0 || D == 0) return PCR_OK;
  if (!track_labels || !det_labels || !count || (cap > 0 && !pairs)) return PCR_ERR_INVALID;
  const int blocks = max(1, min(256, (cap + kPairSlotsPerBlock - 1) / kPairSlotsPerBlock));
  return pcr_launch<assoc_pairs_kernel>(dim3(blocks), dim3(kPairThreads), 0, pcr_s(stream), track_labels, det_labels,
                                        track_lengths, det_lengths, pairs, count, T, D, num_classes, min_points, cap);
}

PCR_EXPORT int pcr_assoc_cost_f32(const float *logits, const int *pairs, const int *count, const float *track_miss,
                                  const float *det_new, const float *dist, float dist_max, float dist_penalty, float fill,
                                  float *cost, int T, int D, int cap, pcr_stream_t stream) {
  if (!pcr_assoc_pairs_ok(T, D, 1, cap)) return PCR_ERR_INVALID;
  const int N = T + D;
  if (N == 0) return PCR_OK;
  const bool listed = T > 0 && D > 0 && cap > 0;
  if (!cost || (listed && (!logits || !pairs || !count))) return PCR_ERR_INVALID;
  int rc = pcr_launch<assoc_cost_fill_kernel>(dim3((N + 255) / 256, N), dim3(256), 0, pcr_s(stream), track_miss, det_new,
                                              fill, cost, T, D);
  if (rc != PCR_OK || !listed) return rc;
  return pcr_launch<assoc_cost_pairs_kernel>(dim3((cap + 255) / 256), dim3(256), 0, pcr_s(stream), logits, pairs, count,
                                             dist, dist_max, dist_penalty, cost, T, D, cap);
}

PCR_EXPORT int pcr_lsa_ok(int B, int R, int C) {
  return B >= 0 && B <= 65535 && R >= 0 && R <= PCR_LSA_MAX && C >= 0 && C <= PCR_LSA_MAX;
}

PCR_EXPORT int pcr_lsa_f32(const float *cost, int *col4row, int *row4col, float *u, float *v, int *info, int B, int R,
                           int C, pcr_stream_t stream) {
  if (!pcr_lsa_ok(B, R, C)) return PCR_ERR_INVALID;
  if (B == 0 || R == 0 || C == 0) return PCR_OK;
  if (!cost || !col4row || !row4col || !info) return PCR_ERR_INVALID;
  const int nc = R > C ? R : C;
  hipStream_t st = pcr_s(stream);
  if (nc <= 64) return lsa_launch<1>(cost, col4row, row4col, u, v, info, B, R, C, st);
  if (nc <= 128) return lsa_launch<2>(cost, col4row, row4col, u, v, info, B, R, C, st);
  if (nc <= 256) return lsa_launch<4>(cost, col4row, row4col, u, v, info, B, R, C, st);
  if (nc <= 512) return lsa_launch<8>(cost, col4row, row4col, u, v, info, B, R, C, st);
  return lsa_launch<16>(cost, col4row, row4col, u, v, info, B, R, C, st);
}

PCR_EXPORT int pcr_lsa_blocks_ok(int R, int C, int G) {
  return R >= 0 && R <= PCR_LSA_MAX && C >= 0 && C <= PCR_LSA_MAX && G >= 1 && G <= PCR_ASSOC_MAX_CLASSES + 1;
}

PCR_EXPORT int pcr_lsa_blocks_f32(const float *cost, const int *row_block, const int *col_block, int *col4row, int *row4col,
                                  float *u, float *v, int *info, int R, int C, int G, pcr_stream_t stream) {
  if (!pcr_lsa_blocks_ok(R, C, G)) return PCR_ERR_INVALID;
  if (!info || (R > 0 && (!row_block || !col4row)) || (C > 0 && (!col_block || !row4col)) || (R > 0 && C > 0 && !cost))
    return PCR_ERR_INVALID;
  const int nc = R > C ? R : C;
  hipStream_t st = pcr_s(stream);
  if (nc <= 64) return lsa_blocks_launch<1>(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, st);
  if (nc <= 128) return lsa_blocks_launch<2>(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, st);
  if (nc <= 256) return lsa_blocks_launch<4>(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, st);
  if (nc <= 512) return lsa_blocks_launch<8>(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, st);
  return lsa_blocks_launch<16>(cost, row_block, col_block, col4row, row4col, u, v, info, R, C, G, st);
}

PCR_EXPORT int pcr_assoc_blocks_i32(const int *track_labels, const int *det_labels, int *row_block, int *col_block, int T,
                                    int D, int de, int te, int num_classes, pcr_stream_t stream) {
  if (!pcr_assoc_multi_ok(T, D, de, te, 0)) return PCR_ERR_INVALID;
  if (num_classes < 1 || num_classes > PCR_ASSOC_MAX_CLASSES) return PCR_ERR_INVALID;
  const int R = T + de * D, C = D + te * T, N = R > C ? R : C;
  if (N == 0) return PCR_OK;
  if ((T > 0 && !track_labels) || (D > 0 && !det_labels) || (R > 0 && !row_block) || (C > 0 && !col_block))
    return PCR_ERR_INVALID;
  return pcr_launch<assoc_blocks_kernel>(dim3((N + 255) / 256), dim3(256), 0, pcr_s(stream), track_labels, det_labels,
                                         row_block, col_block, T, D, R, C, num_classes);
}
