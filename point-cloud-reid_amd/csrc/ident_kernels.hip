// Identity preservation on the device (include/pcr.h, section A9): the per-frame launch that keeps every ground-truth
// track's life (present, tracked, fragments, gaps) and the co-occurrence counts of ground-truth ids and tracker ids, the
// compaction of a scene's counts into the cost matrix of pcr_lsa_f32, and the score launch that adds the scene to a
// persistent 64-bit table.  Every entry is a fixed-shape launch without a host read, an allocation or a float atomic, and
// writes the same bits on every run: the only atomics are integer sums, minima and maxima, whose result does not depend
// on the order.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the binary64 distance sums are compared bit for bit with
// the CPU restatement (tests/ident_ref.py).
#include "pcr_common.h"

namespace {

constexpr int kIdentThreads = 1024;                         // one workgroup of 16 waves
constexpr int kIdentWaves = kIdentThreads / kWave;
constexpr int kNone = 0x7fffffff;                           // an LDS minimum nobody has lowered
constexpr int kCounters = PCR_IDENT_TOTALS;                 // LDS counters of the record launch, one per entry of totals
static_assert(PCR_IDENT_T_DROPPED_ID < kCounters && PCR_IDENT_TRACK_COLS == 8, "the tables of include/pcr.h");

// ---- the frame -------------------------------------------------------------------------------------------------------------
// LDS of record: counters [kCounters] | gid [G]: a valid box's id, or -1 | low_d [G]: the lowest true positive of the box
__global__ __launch_bounds__(kIdentThreads) void ident_record_kernel(pcr_ident p) {
  extern __shared__ int ident_lds[];
  const int D = p.D, G = p.G;
  int *counters = ident_lds, *gid = counters + kCounters, *low_d = gid + G;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  if (tid < kCounters) counters[tid] = tid == PCR_IDENT_T_FRAMES ? 1 : 0;     // the frame itself
  __syncthreads();
  for (int base = 0; base < G; base += kIdentThreads) {
    const int j = base + tid;
    int id = -1;
    if (j < G) {
      id = p.gt_ids[j];
      if (p.gt_labels[j] < 0 || id < 0 || id >= p.gt_cap) id = -1;
      gid[j] = id;
      low_d[j] = kNone;
    }
    wave_count(counters, PCR_IDENT_T_GT_TOTAL, id >= 0, lane);
  }
  __syncthreads();

  // ---- 1. the detections: a true positive lowers its box's minimum ---------------------------------------------------------
  for (int base = 0; base < D; base += kIdentThreads) {
    const int d = base + tid;
    bool tp = false, pred = false;
    if (d < D && p.det_labels[d] >= 0) {
      const int j = p.det_gt[d];
      pred = p.det_id[d] >= 0;
      if (j >= 0 && j < G && gid[j] >= 0) {
        tp = true;
        atomicMin(&low_d[j], d);
      }
    }
    wave_count(counters, PCR_IDENT_T_TP, tp, lane);
    wave_count(counters, PCR_IDENT_T_PRED_TOTAL, pred, lane);
  }
  __syncthreads();

  // ---- 2. the distance sum: wave 0, the true positives in ascending d --------------------------------------------------------
  if (wave == 0) {
    double sum = p.dist_sum[0];
    for (int base = 0; base < D; base += kWave) {
      const int d = base + lane;
      double v = 0.0;
      bool tp = false;
      if (d < D && p.det_labels[d] >= 0) {
        const int j = p.det_gt[d];
        if (j >= 0 && j < G && gid[j] >= 0) tp = true, v = (double)p.cost[(size_t)d * G + j];
      }
      unsigned long long todo = __ballot(tp);
      for (int k = __popcll(todo); k > 0; --k) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        sum = sum + wave_readlane_f64(v, l);
      }
    }
    if (lane == 0) p.dist_sum[0] = sum;
  }

  // ---- 3. the tracks: a wave per box; the first box of an id owns the id's row this frame ------------------------------------
  for (int j = wave; j < G; j += kIdentWaves) {
    const int g = gid[j];                                   // uniform over the wave
    if (g < 0) continue;
    int first = -1, dmin = kNone;
    for (int base = 0; base < G; base += kWave) {
      const int k = base + lane;
      const bool same = k < G && gid[k] == g;
      const unsigned long long bal = __ballot(same);
      if (first < 0 && bal != 0ull) first = base + __ffsll((long long)bal) - 1;
      if (same && low_d[k] < dmin) dmin = low_d[k];
    }
    if (first != j) continue;
    dmin = wave_reduce(dmin, WaveMin());
    if (lane != 0) continue;
    if (g >= p.gt_rows) {
      atomicAdd(&counters[PCR_IDENT_T_DROPPED_GT], 1);
      continue;
    }
    const int i = dmin != kNone ? p.det_id[dmin] : -1;
    int *row = p.gt_track + (size_t)g * PCR_IDENT_TRACK_COLS;
    row[PCR_IDENT_PRESENT] += 1;
    if (i >= 0) {
      row[PCR_IDENT_TRACKED] += 1;
      if (row[PCR_IDENT_EVER] != 0 && row[PCR_IDENT_LAST] == 0) row[PCR_IDENT_FRAGS] += 1;
      if (row[PCR_IDENT_EVER] == 0) row[PCR_IDENT_FIRST_GAP] = row[PCR_IDENT_CUR_GAP];
      row[PCR_IDENT_EVER] = 1, row[PCR_IDENT_CUR_GAP] = 0, row[PCR_IDENT_LAST] = 1;
      if (i < p.id_cap) p.cooc[(size_t)g * p.id_cap + i] += 1;
      else atomicAdd(&counters[PCR_IDENT_T_DROPPED_ID], 1);
    } else {
      const int gap = row[PCR_IDENT_CUR_GAP] + 1;
      row[PCR_IDENT_CUR_GAP] = gap;
      if (gap > row[PCR_IDENT_LONGEST_GAP]) row[PCR_IDENT_LONGEST_GAP] = gap;
      row[PCR_IDENT_LAST] = 0;
    }
  }
  __syncthreads();
  if (tid < kCounters) p.totals[tid] += counters[tid];
}

// ---- the scene's problem ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ident_clear_kernel(int *__restrict__ flags, int *__restrict__ counts, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = 0;
  if (i < PCR_IDENT_COUNTS) counts[i] = 0;
}

// grid (block of 256 columns, group of rows): thread c owns column c over the rows r = blockIdx.y, + gridDim.y, ...  Every
// writer of a flag writes 1; the maximum is an integer atomic.
__global__ __launch_bounds__(256) void ident_activity_kernel(const int *__restrict__ cooc, int *__restrict__ flags,
                                                             int *__restrict__ counts, int gt_rows, int id_cap) {
  const int c = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & (kWave - 1);
  const bool in = c < id_cap;
  int top = 0;
  for (int r = blockIdx.y; r < gt_rows; r += gridDim.y) {
    const int v = in ? cooc[(size_t)r * id_cap + c] : 0;
    const unsigned long long bal = __ballot(v != 0);
    if (lane == 0 && bal != 0ull) flags[r] = 1;
    if (v > top) top = v;
  }
  if (in && top != 0) flags[gt_rows + c] = 1;
  top = wave_reduce(top, WaveMax());
  if (lane == 0 && top > 0) atomicMax(&counts[PCR_IDENT_MAX_COUNT], top);
}

// the ascending list of the set flags, by one workgroup: block 0 ranks the rows, block 1 the columns.  LDS: wave_n [16]
__global__ __launch_bounds__(kIdentThreads) void ident_rank_kernel(pcr_ident_close p) {
  __shared__ int wave_n[kIdentWaves];
  const bool cols = blockIdx.x == 1;
  const int n = cols ? p.id_cap : p.gt_rows, cap = cols ? p.max_cols : p.max_rows;
  const int *flag = cols ? p.flags + p.gt_rows : p.flags;
  int *list = cols ? p.col_list : p.row_list;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int before = 0;                                           // the set flags of the chunks before this one
  for (int base = 0; base < n; base += kIdentThreads) {
    const int i = base + tid;
    const bool set = i < n && flag[i] != 0;
    const unsigned long long bal = __ballot(set);
    if (lane == 0) wave_n[wave] = __popcll(bal);
    __syncthreads();
    int below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kIdentWaves; ++w) {
      const int m = wave_n[w];
      below += w < wave ? m : 0;
      total += m;
    }
    const int rank = before + below + (int)pcr_lanes_below(bal);
    if (set && rank < cap) list[rank] = i;
    before += total;
    __syncthreads();
  }
  for (int r = before + tid; r < cap; r += kIdentThreads) list[r] = -1;
  if (tid == 0) p.counts[cols ? PCR_IDENT_N_COLS : PCR_IDENT_N_ROWS] = before;
}

__global__ __launch_bounds__(256) void ident_gather_kernel(pcr_ident_close p) {
  const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (c >= p.max_cols) return;
  const int nr = p.counts[PCR_IDENT_N_ROWS], nc = p.counts[PCR_IDENT_N_COLS];
  float v = 0.0f;
  if (nr <= p.max_rows && nc <= p.max_cols && r < nr && c < nc) {
    const int g = p.row_list[r], i = p.col_list[c];
    if (g >= 0 && g < p.gt_rows && i >= 0 && i < p.id_cap) {
      const int n = p.cooc[(size_t)g * p.id_cap + i];
      if (n != 0) v = -(float)n;
    }
  }
  p.cost[(size_t)r * p.max_cols + c] = v;
}

// ---- the score -------------------------------------------------------------------------------------------------------------
// LDS: sums [PCR_IDENT_TABLE] 64-bit | mapped [2048]: a bit per ground-truth id that id_map names
__global__ __launch_bounds__(kIdentThreads) void ident_score_kernel(pcr_ident_close p) {
  __shared__ unsigned long long sums[PCR_IDENT_TABLE];
  __shared__ unsigned int mapped[PCR_IDENT_MAX_DIM / 32];
  const int tid = threadIdx.x;
  if (tid < PCR_IDENT_TABLE) sums[tid] = 0ull;
  for (int w = tid; w < PCR_IDENT_MAX_DIM / 32; w += kIdentThreads) mapped[w] = 0u;
  __syncthreads();

  const int nr = p.counts[PCR_IDENT_N_ROWS], nc = p.counts[PCR_IDENT_N_COLS], top = p.counts[PCR_IDENT_MAX_COUNT];
  const bool overflow = nr > p.max_rows || nc > p.max_cols, failed = p.info[0] != 0;
  const long long side = (p.max_rows < p.max_cols ? p.max_rows : p.max_cols) + 1;
  const bool inexact = failed || side * (long long)top >= (1ll << 24);

  // ---- 1. the assigned pairs ---------------------------------------------------------------------------------------------
  unsigned long long idtp = 0ull;
  if (!overflow && !failed) {
    for (int r = tid; r < nr; r += kIdentThreads) {
      const int c = p.col4row[r];
      if (c < 0 || c >= nc) continue;
      const int g = p.row_list[r], i = p.col_list[c];
      if (g < 0 || g >= p.gt_rows || i < 0 || i >= p.id_cap) continue;
      const int n = p.cooc[(size_t)g * p.id_cap + i];
      if (n <= 0) continue;
      idtp += (unsigned long long)n;
      p.id_map[g] = i;
      atomicOr(&mapped[g >> 5], 1u << (g & 31));
    }
  }
  if (idtp != 0ull) atomicAdd(&sums[PCR_IDENT_IDTP], idtp);

  // ---- 2. the tracks -----------------------------------------------------------------------------------------------------
  unsigned long long tracks = 0ull, mt = 0ull, pt = 0ull, ml = 0ull, frag = 0ull, tid_sum = 0ull, lgd_sum = 0ull;
  for (int g = tid; g < p.gt_rows; g += kIdentThreads) {
    const int *row = p.gt_track + (size_t)g * PCR_IDENT_TRACK_COLS;
    const long long present = row[PCR_IDENT_PRESENT], tracked = row[PCR_IDENT_TRACKED];
    if (present <= 0) continue;
    tracks += 1ull;
    if (5 * tracked >= 4 * present) mt += 1ull;
    else if (5 * tracked < present) ml += 1ull;
    else pt += 1ull;
    frag += (unsigned long long)row[PCR_IDENT_FRAGS];
    tid_sum += (unsigned long long)(row[PCR_IDENT_EVER] != 0 ? row[PCR_IDENT_FIRST_GAP] : row[PCR_IDENT_PRESENT]);
    lgd_sum += (unsigned long long)row[PCR_IDENT_LONGEST_GAP];
  }
  if (tracks != 0ull) {
    atomicAdd(&sums[PCR_IDENT_TRACKS], tracks);
    atomicAdd(&sums[PCR_IDENT_MT], mt);
    atomicAdd(&sums[PCR_IDENT_PT], pt);
    atomicAdd(&sums[PCR_IDENT_ML], ml);
    atomicAdd(&sums[PCR_IDENT_FRAG], frag);
    atomicAdd(&sums[PCR_IDENT_TID_SUM], tid_sum);
    atomicAdd(&sums[PCR_IDENT_LGD_SUM], lgd_sum);
  }
  __syncthreads();

  // ---- 3. id_map's other entries; the table ----------------------------------------------------------------------------------
  for (int g = tid; g < p.gt_rows; g += kIdentThreads)
    if ((mapped[g >> 5] >> (g & 31) & 1u) == 0u) p.id_map[g] = -1;
  if (tid == 0) {
    sums[PCR_IDENT_FRAMES] = (unsigned long long)p.totals[PCR_IDENT_T_FRAMES];
    sums[PCR_IDENT_GT_TOTAL] = (unsigned long long)p.totals[PCR_IDENT_T_GT_TOTAL];
    sums[PCR_IDENT_PRED_TOTAL] = (unsigned long long)p.totals[PCR_IDENT_T_PRED_TOTAL];
    sums[PCR_IDENT_TP] = (unsigned long long)p.totals[PCR_IDENT_T_TP];
    sums[PCR_IDENT_DROPPED_GT] = (unsigned long long)p.totals[PCR_IDENT_T_DROPPED_GT];
    sums[PCR_IDENT_DROPPED_ID] = (unsigned long long)p.totals[PCR_IDENT_T_DROPPED_ID];
    sums[PCR_IDENT_OVERFLOW] = overflow ? 1ull : 0ull;
    sums[PCR_IDENT_INEXACT] = inexact ? 1ull : 0ull;
    p.dist_total[0] = p.dist_total[0] + p.dist_sum[0];
  }
  __syncthreads();
  if (tid < PCR_IDENT_TABLE) p.table[tid] += (long long)sums[tid];
}

bool close_block_ok(const pcr_ident_close *p) {
  if (!p || !pcr_ident_ok(0, 0, 1, p->gt_rows, p->id_cap, p->max_rows, p->max_cols)) return false;
  return p->cooc && p->counts && p->row_list && p->col_list;
}

}  // namespace

PCR_EXPORT int pcr_ident_ok(int D, int G, int gt_cap, int gt_rows, int id_cap, int max_rows, int max_cols) {
  return D >= 0 && D <= PCR_LSA_MAX && G >= 0 && G <= PCR_LSA_MAX && gt_cap >= 1 && gt_cap <= PCR_TRUTH_MAX_IDS &&
         gt_rows >= 1 && gt_rows <= PCR_IDENT_MAX_DIM && id_cap >= 1 && id_cap <= PCR_IDENT_MAX_DIM &&
         (long long)gt_rows * id_cap <= (long long)PCR_IDENT_MAX_CELLS && max_rows >= 1 && max_rows <= PCR_LSA_MAX &&
         max_cols >= 1 && max_cols <= PCR_LSA_MAX;
}

PCR_EXPORT int pcr_ident_record_i32(const pcr_ident *p, pcr_stream_t stream) {
  if (!p || !pcr_ident_ok(p->D, p->G, p->gt_cap, p->gt_rows, p->id_cap, 1, 1)) return PCR_ERR_INVALID;
  if (!p->cooc || !p->gt_track || !p->totals || !p->dist_sum) return PCR_ERR_INVALID;
  if (p->D > 0 && (!p->det_labels || !p->det_gt || !p->det_id)) return PCR_ERR_INVALID;
  if (p->G > 0 && (!p->gt_labels || !p->gt_ids)) return PCR_ERR_INVALID;
  if (p->D > 0 && p->G > 0 && !p->cost) return PCR_ERR_INVALID;
  return pcr_launch<ident_record_kernel>(dim3(1), dim3(kIdentThreads), (size_t)(kCounters + 2 * p->G) * sizeof(int),
                                         pcr_s(stream), *p);
}

PCR_EXPORT int pcr_ident_compact_f32(const pcr_ident_close *p, pcr_stream_t stream) {
  if (!close_block_ok(p) || !p->flags || !p->cost) return PCR_ERR_INVALID;
  const int n = p->gt_rows + p->id_cap;
  int st = pcr_launch<ident_clear_kernel>(dim3((n + 255) / 256), dim3(256), 0, pcr_s(stream), p->flags, p->counts, n);
  if (st != PCR_OK) return st;
  const int col_blocks = (p->id_cap + 255) / 256;
  int row_groups = (4 * pcr_cu_count() + col_blocks - 1) / col_blocks;      // about four workgroups per compute unit
  row_groups = row_groups < 1 ? 1 : row_groups > p->gt_rows ? p->gt_rows : row_groups;
  st = pcr_launch<ident_activity_kernel>(dim3(col_blocks, row_groups), dim3(256), 0, pcr_s(stream), p->cooc, p->flags,
                                         p->counts, p->gt_rows, p->id_cap);
  if (st != PCR_OK) return st;
  st = pcr_launch<ident_rank_kernel>(dim3(2), dim3(kIdentThreads), 0, pcr_s(stream), *p);
  if (st != PCR_OK) return st;
  return pcr_launch<ident_gather_kernel>(dim3((p->max_cols + 255) / 256, p->max_rows), dim3(256), 0, pcr_s(stream), *p);
}

PCR_EXPORT int pcr_ident_score_i32(const pcr_ident_close *p, pcr_stream_t stream) {
  if (!close_block_ok(p) || !p->gt_track || !p->totals || !p->dist_sum || !p->col4row || !p->info || !p->id_map ||
      !p->table || !p->dist_total)
    return PCR_ERR_INVALID;
  return pcr_launch<ident_score_kernel>(dim3(1), dim3(kIdentThreads), 0, pcr_s(stream), *p);
}
