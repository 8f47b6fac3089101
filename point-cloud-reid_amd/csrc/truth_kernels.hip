// Scoring the tracker against ground-truth tracks on the device (include/pcr.h, section A7): the matching cost between
// detections and ground-truth boxes, the frame's true decisions with the reference's counters, and the book that carries
// every track's ground-truth id and time to end from frame to frame, with the MOT counters.  Every entry is a fixed-shape
// launch without a host read, an allocation or a float atomic, and writes the same bits on every run: the only atomics
// are integer sums and minima in LDS, whose result does not depend on the order.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the cost is compared bit for bit with the CPU restatement
// (tests/truth_ref.py).
#include "pcr_common.h"

namespace {

constexpr int kTruthThreads = 1024;                         // one workgroup of 16 waves
constexpr int kTruthWaves = kTruthThreads / kWave;
constexpr int kNone = 0x7fffffff;                           // an LDS minimum nobody has lowered
constexpr int kCounters = 16;                               // LDS counters of a launch

// cost (D, G): grid (block of 256 ground-truth boxes, detection)
__global__ __launch_bounds__(256) void truth_cost_kernel(const float *__restrict__ det_boxes, const int *__restrict__ det_labels,
                                                         const float *__restrict__ gt_boxes, const int *__restrict__ gt_labels,
                                                         const int *__restrict__ gt_ids, const float *__restrict__ iou,
                                                         float *__restrict__ cost, int G, int W, int gt_cap) {
  const int d = blockIdx.y, g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  float base;
  if (iou != nullptr) {
    base = -iou[(size_t)d * G + g];
  } else {
    const float dx = det_boxes[(size_t)d * W] - gt_boxes[(size_t)g * W];
    const float dy = det_boxes[(size_t)d * W + 1] - gt_boxes[(size_t)g * W + 1];
    const float a = dx * dx;
    const float b = dy * dy;
    base = sqrtf(a + b);
  }
  const int dl = det_labels[d], gl = gt_labels[g], id = gt_ids[g];
  const bool same = dl >= 0 && gl >= 0 && id >= 0 && id < gt_cap && dl == gl;
  cost[(size_t)d * G + g] = base + (same ? 0.0f : 10000.0f);
}

// ---- the rules both launches share ----------------------------------------------------------------------------------------
__device__ __forceinline__ bool gt_valid(const pcr_truth &p, int j) {
  const int id = p.gt_ids[j];
  return p.gt_labels[j] >= 0 && id >= 0 && id < p.gt_cap;
}

// pcr_bank_plan_i32's rules for the tracker's own decisions, from the state before the update
__device__ __forceinline__ bool slot_killed(const pcr_truth &p, int s) { return p.kill != nullptr && p.kill[s] != 0; }

__device__ __forceinline__ bool slot_matched(const pcr_truth &p, int s) {
  if (p.ids[s] < 0 || slot_killed(p, s)) return false;
  const int d = p.track_to_det[s];
  if (d < 0 || d >= p.D) return false;
  return p.det_labels[d] >= 0 && p.det_to_track[d] == s;
}

// the lowest index i < n with table[i] == key, by one wave (every lane calls it with the same key and n), or -1
__device__ __forceinline__ int first_equal(const int *__restrict__ table, int n, int key, int lane) {
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    const unsigned long long bal = __ballot(i < n && table[i] == key);
    if (bal != 0ull) return base + __ffsll((long long)bal) - 1;
  }
  return -1;
}

// LDS of decide: counters [kCounters] | held [C]: the id an active slot is booked as, or -1 | take [C]: the lowest true
// positive of the id the slot holds | det_track [D]: g(d) of a true positive, or -1 | det_holder [D]: the slot that holds it
constexpr int kDmatchGt = 0, kDmatchBoth = 1, kDmatchPred = 2, kBornGt = 3, kBornBoth = 4, kBornPred = 5, kDfpGt = 6,
              kDfpBoth = 7, kDfpPred = 8, kFnGt = 9, kFnBoth = 10, kFnPred = 11, kTfpGt = 12, kTfpBoth = 13, kTfpPred = 14;

__global__ __launch_bounds__(kTruthThreads) void truth_decide_kernel(pcr_truth p) {
  extern __shared__ int truth_lds[];
  const int C = p.C, D = p.D, G = p.G;
  int *counters = truth_lds, *held = counters + kCounters, *take = held + C, *det_track = take + C, *det_holder = det_track + D;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  // ---- 1. the true positives; what every slot is booked as ---------------------------------------------------------------
  if (tid < kCounters) counters[tid] = 0;
  for (int s = tid; s < C; s += kTruthThreads) {
    const int g = p.slot_gt[s];
    held[s] = p.ids[s] >= 0 && g >= 0 ? g : -1;
    take[s] = kNone;
  }
  const bool solved = D > 0 && G > 0 && p.info[0] == 0;
  const float thresh = p.thresh[0];
  for (int d = tid; d < D; d += kTruthThreads) {
    int j = -1;
    if (solved && p.det_labels[d] >= 0) {
      const int c = p.col4row[d];
      if (c >= 0 && c < G && p.row4col[c] == d && gt_valid(p, c) && p.gt_labels[c] == p.det_labels[d] &&
          p.cost[(size_t)d * G + c] < thresh)
        j = c;
    }
    p.det_gt[d] = j;
    det_track[d] = j >= 0 ? p.gt_ids[j] : -1;
    det_holder[d] = -1;
  }
  __syncthreads();

  // ---- 2. the join: a wave per detection finds the lowest slot that holds its id ------------------------------------------
  for (int d = wave; d < D; d += kTruthWaves) {
    const int g = det_track[d];                             // uniform over the wave
    if (g < 0) continue;
    const int s = first_equal(held, C, g, lane);
    if (lane == 0 && s >= 0) {
      det_holder[d] = s;
      atomicMin(&take[s], d);
    }
  }
  __syncthreads();

  // ---- 3. the decisions and the frame's counts.  A slot's and a detection's entries are written by their owner only -----
  for (int base = 0; base < C; base += kTruthThreads) {
    const int s = base + tid;
    const bool in = s < C;
    const bool active = in && p.ids[s] >= 0;
    int t2d = -1, truth = -1;
    bool killed = false, matched = false;
    if (active) {
      if (take[s] != kNone) t2d = take[s];
      truth = t2d >= 0 ? 0 : (p.slot_gt[s] < 0 || p.slot_tte[s] < 0) ? 2 : 1;
      killed = p.forced ? truth == 2 : slot_killed(p, s);
      matched = p.forced ? truth == 0 : slot_matched(p, s);
    }
    if (in) p.true_t2d[s] = t2d, p.track_truth[s] = truth;
    const bool missed = active && !killed && !matched;
    wave_count(counters, kDmatchGt, truth == 0, lane);
    wave_count(counters, kDmatchPred, matched, lane);
    wave_count(counters, kDmatchBoth, matched && truth == 0 && (p.forced || p.track_to_det[s] == t2d), lane);
    wave_count(counters, kFnGt, truth == 1, lane);
    wave_count(counters, kFnPred, missed, lane);
    wave_count(counters, kFnBoth, missed && truth == 1, lane);
    wave_count(counters, kTfpGt, truth == 2, lane);
    wave_count(counters, kTfpPred, killed, lane);
    wave_count(counters, kTfpBoth, killed && truth == 2, lane);
  }
  for (int base = 0; base < D; base += kTruthThreads) {
    const int d = base + tid;
    const bool valid = d < D && p.det_labels[d] >= 0;
    int d2t = -1, truth = -1;
    bool born = false, rejected = false;
    if (valid) {
      const int h = det_holder[d];
      if (h >= 0 && take[h] == d) d2t = h;
      truth = d2t >= 0 ? 0 : det_track[d] >= 0 ? 1 : 2;
      if (p.forced) {
        born = truth == 1, rejected = truth == 2;
      } else {
        const int t = p.det_to_track[d];
        const bool matched = t >= 0 && t < C && p.track_to_det[t] == d && slot_matched(p, t);
        born = !matched && (p.born == nullptr || p.born[d] != 0);
        rejected = !matched && !born;
      }
    }
    if (d < D) p.true_d2t[d] = d2t, p.det_truth[d] = truth;
    wave_count(counters, kBornGt, truth == 1, lane);
    wave_count(counters, kBornPred, born, lane);
    wave_count(counters, kBornBoth, born && truth == 1, lane);
    wave_count(counters, kDfpGt, truth == 2, lane);
    wave_count(counters, kDfpPred, rejected, lane);
    wave_count(counters, kDfpBoth, rejected && truth == 2, lane);
  }
  __syncthreads();

  // ---- 4. get_stats: thread k adds kind k; the two totals are thread 0's ------------------------------------------------------
  const bool adds = tid < 5 && (p.skip_empty == 0 || counters[3 * tid] > 0);
  if (adds) {
    p.stats[3 * tid] += counters[3 * tid];
    p.stats[3 * tid + 1] += counters[3 * tid + 1];
    p.stats[3 * tid + 2] += counters[3 * tid + 2];
  }
  if (tid == 0) {
    int gt = 0, correct = 0;
    for (int k = 0; k < 5; ++k)
      if (p.skip_empty == 0 || counters[3 * k] > 0) gt += counters[3 * k], correct += counters[3 * k + 1];
    p.stats[PCR_TRUTH_TOTAL_GT] += gt;
    p.stats[PCR_TRUTH_TOTAL_CORRECT] += correct;
  }
}

// LDS of record: counters [kCounters] | slot_det [C]: the lowest detection that joined the slot | det_track [D] | gt_hit [G]
constexpr int kGtTotal = 0, kTp = 1, kFp = 2, kFn = 3, kSwitches = 4, kUntracked = 5;

__global__ __launch_bounds__(kTruthThreads) void truth_record_kernel(pcr_truth p) {
  extern __shared__ int truth_lds[];
  const int C = p.C, D = p.D, G = p.G;
  int *counters = truth_lds, *slot_det = counters + kCounters, *det_track = slot_det + C, *gt_hit = det_track + D;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  if (tid < kCounters) counters[tid] = 0;
  for (int s = tid; s < C; s += kTruthThreads) slot_det[s] = kNone;
  for (int j = tid; j < G; j += kTruthThreads) gt_hit[j] = 0;
  __syncthreads();

  // ---- 1. the detections: their ground-truth track, the slot they joined ---------------------------------------------------
  for (int base = 0; base < D; base += kTruthThreads) {
    const int d = base + tid;
    int g = -1;
    bool valid = false;
    if (d < D) {
      valid = p.det_labels[d] >= 0;
      const int j = p.det_gt[d];
      if (valid && j >= 0 && j < G && gt_valid(p, j)) {
        g = p.gt_ids[j];
        gt_hit[j] = 1;
      }
      det_track[d] = g;
      const int s = p.det_slot[d];
      if (s >= 0 && s < C) atomicMin(&slot_det[s], d);
    }
    wave_count(counters, kTp, g >= 0, lane);
    wave_count(counters, kFp, valid && g < 0, lane);
  }
  __syncthreads();

  // ---- 2. the book, a slot by its owner --------------------------------------------------------------------------------------
  for (int s = tid; s < C; s += kTruthThreads) {
    int g = p.slot_gt[s], tte = p.slot_tte[s];
    if (p.track_truth[s] >= 0) tte -= 1;
    const int d = slot_det[s];
    if (d != kNone) {
      g = det_track[d];
      tte = g >= 0 ? p.gt_tte[p.det_gt[d]] : -1;
    }
    if (p.ids[s] < 0) g = -1, tte = -1;
    p.slot_gt[s] = g;
    p.slot_tte[s] = tte;
  }

  // ---- 3. the MOT counters -----------------------------------------------------------------------------------------------------
  for (int base = 0; base < G; base += kTruthThreads) {
    const int j = base + tid;
    const bool valid = j < G && gt_valid(p, j);
    wave_count(counters, kGtTotal, valid, lane);
    wave_count(counters, kFn, valid && gt_hit[j] == 0, lane);
  }
  for (int d = wave; d < D; d += kTruthWaves) {             // a wave per detection: is a lower true positive of its track?
    const int g = det_track[d];                             // uniform over the wave
    if (g < 0) continue;
    const int first = first_equal(det_track, d, g, lane);
    if (lane != 0) continue;
    const int id = p.det_id[d];
    if (id < 0) atomicAdd(&counters[kUntracked], 1);
    if (first < 0) {                                        // the only writer of gt_last[g] in this launch
      const int last = p.gt_last[g];
      if (last >= 0 && last != id) atomicAdd(&counters[kSwitches], 1);
      p.gt_last[g] = id;
    }
  }
  __syncthreads();
  if (tid == 0) {
    p.stats[PCR_TRUTH_FRAMES] += 1;
    p.stats[PCR_TRUTH_GT_TOTAL] += counters[kGtTotal];
    p.stats[PCR_TRUTH_TP] += counters[kTp];
    p.stats[PCR_TRUTH_FP] += counters[kFp];
    p.stats[PCR_TRUTH_FN] += counters[kFn];
    p.stats[PCR_TRUTH_SWITCHES] += counters[kSwitches];
    p.stats[PCR_TRUTH_UNTRACKED] += counters[kUntracked];
  }
}

// what both launches need whatever they do
bool truth_block_ok(const pcr_truth *p) {
  if (!p || !pcr_truth_ok(p->C, p->D, p->G, 7, p->gt_cap)) return false;
  if (!p->ids || !p->slot_gt || !p->slot_tte || !p->stats || !p->track_truth) return false;
  if (p->D > 0 && (!p->det_labels || !p->det_gt)) return false;
  if (p->G > 0 && (!p->gt_labels || !p->gt_ids || !p->gt_tte)) return false;
  return true;
}

}  // namespace

PCR_EXPORT int pcr_truth_ok(int C, int D, int G, int W, int gt_cap) {
  return C >= 1 && C <= PCR_ASSOC_MAX_OBJECTS && D >= 0 && D <= PCR_LSA_MAX && G >= 0 && G <= PCR_LSA_MAX &&
         (W == 7 || W == 9) && gt_cap >= 1 && gt_cap <= PCR_TRUTH_MAX_IDS;
}

PCR_EXPORT int pcr_truth_cost_f32(const float *det_boxes, const int *det_labels, const float *gt_boxes, const int *gt_labels,
                                  const int *gt_ids, const float *iou, float *cost, int D, int G, int W, int gt_cap,
                                  pcr_stream_t stream) {
  if (!pcr_truth_ok(1, D, G, W, gt_cap)) return PCR_ERR_INVALID;
  if (D == 0 || G == 0) return PCR_OK;
  if (!det_labels || !gt_labels || !gt_ids || !cost || (!iou && (!det_boxes || !gt_boxes))) return PCR_ERR_INVALID;
  return pcr_launch<truth_cost_kernel>(dim3((G + 255) / 256, D), dim3(256), 0, pcr_s(stream), det_boxes, det_labels,
                                       gt_boxes, gt_labels, gt_ids, iou, cost, G, W, gt_cap);
}

PCR_EXPORT int pcr_truth_decide_i32(const pcr_truth *p, pcr_stream_t stream) {
  if (!truth_block_ok(p) || !p->thresh || !p->true_t2d) return PCR_ERR_INVALID;
  if (p->D > 0 && (!p->true_d2t || !p->det_truth)) return PCR_ERR_INVALID;
  if (!p->forced && (!p->track_to_det || (p->D > 0 && !p->det_to_track))) return PCR_ERR_INVALID;
  if (p->D > 0 && p->G > 0 && (!p->col4row || !p->row4col || !p->info || !p->cost)) return PCR_ERR_INVALID;
  return pcr_launch<truth_decide_kernel>(dim3(1), dim3(kTruthThreads), (size_t)(kCounters + 2 * p->C + 2 * p->D) * sizeof(int),
                                         pcr_s(stream), *p);
}

PCR_EXPORT int pcr_truth_record_i32(const pcr_truth *p, pcr_stream_t stream) {
  if (!truth_block_ok(p) || !p->gt_last) return PCR_ERR_INVALID;
  if (p->D > 0 && (!p->det_slot || !p->det_id)) return PCR_ERR_INVALID;
  return pcr_launch<truth_record_kernel>(dim3(1), dim3(kTruthThreads), (size_t)(kCounters + p->C + p->D + p->G) * sizeof(int),
                                         pcr_s(stream), *p);
}
