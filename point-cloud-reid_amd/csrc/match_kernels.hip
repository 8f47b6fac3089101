// Scoring a validation split on the device (include/pcr.h, section A13): a batch of pairs -- logit, target, classes, point
// counts, visibility -- is added to ONE table of 64-bit integer counters from which val_match_acc and every entry of the
// reference's MatchingEval tables are derived on the host, once, at the end.  Fixed-shape launches without a host read, an
// allocation or a float accumulate: every add is an integer atomic, so the table does not depend on the order of the adds
// and is the same bits on every run.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py) like the other books; it holds float compares only.
#include "pcr_common.h"

namespace {

constexpr int kMatchThreads = 256;
constexpr int kSmall = PCR_MATCH_VIS;                       // ALL, CLS0, CLSMAX and PTS: the LDS histogram (27 KiB)
static_assert(PCR_MATCH_CLS0 == PCR_MATCH_ALL + PCR_MATCH_CELLS &&
                  PCR_MATCH_CLSMAX == PCR_MATCH_CLS0 + PCR_MATCH_KEY_BINS * PCR_MATCH_CELLS &&
                  PCR_MATCH_PTS == PCR_MATCH_CLSMAX + PCR_MATCH_KEY_BINS * PCR_MATCH_CELLS &&
                  PCR_MATCH_VIS == PCR_MATCH_PTS + PCR_MATCH_PTS_BINS * PCR_MATCH_PTS_BINS * PCR_MATCH_CELLS &&
                  PCR_MATCH_OBJ == PCR_MATCH_VIS + PCR_MATCH_KEY_BINS * PCR_MATCH_KEY_BINS * PCR_MATCH_CELLS &&
                  PCR_MATCH_TABLE == PCR_MATCH_OBJ + PCR_MATCH_OBJECTS,
              "the table of include/pcr.h");

__device__ __forceinline__ bool key_ok(int v) { return v >= -1 && v <= PCR_MATCH_KEY_BINS - 2; }
__device__ __forceinline__ int pts_bin(int n) { return n == 0 ? 0 : 32 - __clz(n); }    // n >= 0: 1 + floor(log2 n)

// the device-side count, clamped to [0, n]; n without one
__device__ __forceinline__ int live_rows(const int *count, int n) {
  if (!count) return n;
  const int c = count[0];
  return c < 0 ? 0 : c > n ? n : c;
}

// LDS: hist [kSmall] 32-bit counters | flags [1]
__global__ __launch_bounds__(kMatchThreads) void match_record_kernel(pcr_match p) {
  __shared__ int hist[kSmall];
  __shared__ int flags;
  const int tid = threadIdx.x;
  for (int k = tid; k < kSmall; k += kMatchThreads) hist[k] = 0;
  if (tid == 0) flags = 0;
  __syncthreads();

  const int n = live_rows(p.count, p.P);
  unsigned long long *table = reinterpret_cast<unsigned long long *>(p.table);
  int mine = 0;
  const long long step = (long long)gridDim.x * kMatchThreads;
  for (long long i = (long long)blockIdx.x * kMatchThreads + tid; i < n; i += step) {
    const float x = p.logit[i], g = p.gt[i];
    const int gi = g == 1.0f ? 0 : g == 0.0f ? 1 : g == -1.0f ? 2 : -1;
    if (gi < 0) {
      mine |= PCR_MATCH_INFO_GT;
      continue;
    }
    if (x != x) mine |= PCR_MATCH_INFO_NAN;
    const int cell = 2 * gi + (x > 0.0f ? 1 : 0);
    atomicAdd(&hist[PCR_MATCH_ALL + cell], 1);

    const int c0 = p.cls[2 * i], c1 = p.cls[2 * i + 1];
    if (key_ok(c0) && key_ok(c1)) {
      atomicAdd(&hist[PCR_MATCH_CLS0 + (c0 + 1) * PCR_MATCH_CELLS + cell], 1);
      atomicAdd(&hist[PCR_MATCH_CLSMAX + ((c0 > c1 ? c0 : c1) + 1) * PCR_MATCH_CELLS + cell], 1);
    } else {
      mine |= PCR_MATCH_INFO_CLS;
    }

    const int n0 = p.num_points[2 * i], n1 = p.num_points[2 * i + 1];
    if (n0 >= 0 && n1 >= 0) {
      const int key = PCR_MATCH_PTS_BINS * pts_bin(n0 < n1 ? n0 : n1) + pts_bin(n0 < n1 ? n1 : n0);
      atomicAdd(&hist[PCR_MATCH_PTS + key * PCR_MATCH_CELLS + cell], 1);
    } else {
      mine |= PCR_MATCH_INFO_PTS;
    }

    const int v0 = p.vis[2 * i], v1 = p.vis[2 * i + 1];
    if (key_ok(v0) && key_ok(v1)) {
      const int key = PCR_MATCH_KEY_BINS * ((v0 < v1 ? v0 : v1) + 1) + (v0 < v1 ? v1 : v0) + 1;
      atomicAdd(&table[PCR_MATCH_VIS + key * PCR_MATCH_CELLS + cell], 1ull);
    } else {
      mine |= PCR_MATCH_INFO_VIS;
    }
  }
  if (mine != 0) atomicOr(&flags, mine);
  __syncthreads();

  for (int k = tid; k < kSmall; k += kMatchThreads) {
    const int v = hist[k];
    if (v != 0) atomicAdd(&table[k], (unsigned long long)v);
  }
  if (tid == 0 && flags != 0) atomicOr(p.info, flags);
}

// LDS: sums [PCR_MATCH_OBJECTS] | flags [1].  One thread per object, strided.
__global__ __launch_bounds__(kMatchThreads) void match_objects_kernel(const float *__restrict__ cls_logits,
                                                                      const int *__restrict__ cls_gt,
                                                                      const float *__restrict__ fp_logits,
                                                                      const float *__restrict__ fp_gt,
                                                                      const int *__restrict__ count,
                                                                      unsigned long long *__restrict__ objects,
                                                                      int *__restrict__ info, int M, int C, int period) {
  __shared__ int sums[PCR_MATCH_OBJECTS];
  __shared__ int flags;
  const int tid = threadIdx.x;
  if (tid < PCR_MATCH_OBJECTS) sums[tid] = 0;
  if (tid == 0) flags = 0;
  __syncthreads();

  const int live = live_rows(count, period);
  int mine = 0, cls_ok = 0, cls_n = 0, fp_ok = 0, fp_n = 0;
  const long long step = (long long)gridDim.x * kMatchThreads;
  for (long long m = (long long)blockIdx.x * kMatchThreads + tid; m < M; m += step) {
    if ((int)(m % period) >= live) continue;
    if (cls_logits && cls_gt) {
      const float *row = cls_logits + (size_t)m * C;
      float best = row[0];
      int arg = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (best == best && (v > best || v != v)) best = v, arg = c;     // the first NaN stays the maximum
      }
      if (best != best) mine |= PCR_MATCH_INFO_NAN;
      cls_n += 1;
      cls_ok += arg == cls_gt[m] ? 1 : 0;
    }
    if (fp_logits && fp_gt) {
      const float x = fp_logits[m];
      if (x != x) mine |= PCR_MATCH_INFO_NAN;
      fp_n += 1;
      fp_ok += (x > 0.0f ? 1.0f : 0.0f) == fp_gt[m] ? 1 : 0;
    }
  }
  if (cls_n != 0) atomicAdd(&sums[PCR_MATCH_CLS_TOTAL], cls_n);
  if (cls_ok != 0) atomicAdd(&sums[PCR_MATCH_CLS_CORRECT], cls_ok);
  if (fp_n != 0) atomicAdd(&sums[PCR_MATCH_FP_TOTAL], fp_n);
  if (fp_ok != 0) atomicAdd(&sums[PCR_MATCH_FP_CORRECT], fp_ok);
  if (mine != 0) atomicOr(&flags, mine);
  __syncthreads();
  if (tid < PCR_MATCH_OBJECTS && sums[tid] != 0) atomicAdd(&objects[tid], (unsigned long long)sums[tid]);
  if (tid == 0 && flags != 0) atomicOr(info, flags);
}

// workgroups for n rows: one per 256 rows, at most four per compute unit (the kernels stride)
int match_grid(int n) {
  const int want = (n + kMatchThreads - 1) / kMatchThreads, cap = 4 * pcr_cu_count();
  return want < cap ? want : cap;
}

}  // namespace

PCR_EXPORT int pcr_match_ok(int P, int M, int C) {
  return P >= 0 && P <= PCR_MATCH_MAX_ROWS && M >= 0 && M <= PCR_MATCH_MAX_ROWS && C >= 1 && C <= PCR_MATCH_MAX_CLASSES;
}

PCR_EXPORT int pcr_match_record_i64(const pcr_match *p, pcr_stream_t stream) {
  if (!p || !pcr_match_ok(p->P, 0, 1) || !p->table || !p->info) return PCR_ERR_INVALID;
  if (p->P == 0) return PCR_OK;
  if (!p->logit || !p->gt || !p->cls || !p->num_points || !p->vis) return PCR_ERR_INVALID;
  return pcr_launch<match_record_kernel>(dim3(match_grid(p->P)), dim3(kMatchThreads), 0, pcr_s(stream), *p);
}

PCR_EXPORT int pcr_match_record_objects_i64(const float *cls_logits, const int *cls_gt, const float *fp_logits,
                                            const float *fp_gt, const int *count, long long *objects, int *info, int M, int C,
                                            int period, pcr_stream_t stream) {
  if (!pcr_match_ok(0, M, C) || !objects || !info) return PCR_ERR_INVALID;
  if ((cls_logits == nullptr) != (cls_gt == nullptr) || (fp_logits == nullptr) != (fp_gt == nullptr)) return PCR_ERR_INVALID;
  if (M == 0 || (!cls_logits && !fp_logits)) return PCR_OK;
  if (period < 1 || period > M) return PCR_ERR_INVALID;
  return pcr_launch<match_objects_kernel>(dim3(match_grid(M)), dim3(kMatchThreads), 0, pcr_s(stream), cls_logits, cls_gt,
                                          fp_logits, fp_gt, count, reinterpret_cast<unsigned long long *>(objects), info, M, C,
                                          period);
}
