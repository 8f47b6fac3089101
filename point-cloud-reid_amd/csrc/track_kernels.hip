// Track state on the device (include/pcr.h, sections A5 and A11): a fixed-capacity bank of tracks that a frame's assignment
// updates in place -- births, deaths, feature replacement, propagation of missed tracks -- the distance prior between the
// stored tracks and a frame's detections, the retirement of suppressed tracks, the same update under the reference's
// per-decision rules with its output table, and the scene log that table is appended to.  Every entry is a fixed-shape launch
// without a host read, an allocation or an atomic, and writes the same bits on every run.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the propagated boxes and the distances are compared bit
// for bit with the CPU restatement (tests/track_ref.py).
#include "pcr_common.h"

namespace {

constexpr int kPlanThreads = 1024;                          // one workgroup of 16 waves: 64 words of 64 entries in 4 passes
constexpr int kPlanWords = PCR_ASSOC_MAX_OBJECTS / kWave;   // ballot words per side
constexpr int kMoveThreads = 256;
constexpr int kMoveChunk = kMoveThreads * 4 * 4;            // floats of a row one workgroup copies: 4 x 16 bytes per thread

static_assert(PCR_ASSOC_MAX_OBJECTS % kPlanThreads == 0 && kPlanWords <= kWave, "one wave scans a side's words");

// what the plan knows of a detection once the old state has been read
constexpr int kDetNone = -1;                                // joins no track
constexpr int kDetBorn = -2;                                // a newborn, if a slot is left for it

// y = ((m0 * x + m1 * y) + m2 * z) + m3, left to right, each operation rounded to binary32
__device__ __forceinline__ float affine_row(const float *__restrict__ m, float x, float y, float z) {
  const float a = m[0] * x;
  const float b = m[1] * y;
  const float c = m[2] * z;
  const float ab = a + b;
  const float abc = ab + c;
  return abc + m[3];
}

// a missed track's box one frame on, in place: the centre moves by half the velocity (W == 9) and through carry
__device__ __forceinline__ void propagate_box(float *__restrict__ b, int W, const float *__restrict__ carry) {
  float x = b[0], y = b[1];
  const float z = b[2];
  if (W == 9) {
    x = x + b[7] / 2.0f;
    y = y + b[8] / 2.0f;
  }
  if (carry != nullptr) {
    b[0] = affine_row(carry, x, y, z);
    b[1] = affine_row(carry + 4, x, y, z);
    b[2] = affine_row(carry + 8, x, y, z);
  } else {
    b[0] = x, b[1] = y;
  }
}

// the matched rule, from the OLD state only (ids, kill and the two maps; nothing here is written before the barrier)
__device__ __forceinline__ bool slot_killed(const pcr_bank &p, int s) { return p.kill != nullptr && p.kill[s] != 0; }

__device__ __forceinline__ bool slot_matched(const pcr_bank &p, int s) {
  if (p.ids[s] < 0 || slot_killed(p, s)) return false;
  const int d = p.track_to_det[s];
  if (d < 0 || d >= p.D) return false;
  return p.det_labels[d] >= 0 && p.det_to_track[d] == s;
}

// exclusive prefix of the words' popcounts by one wave (lane = word), and their total
__device__ __forceinline__ void scan_words(const unsigned long long *__restrict__ words, int *__restrict__ prefix,
                                           int *__restrict__ total, int lane) {
  const int mine = __popcll(words[lane]);
  int inc = mine;
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    const int o = __shfl_up(inc, k, kWave);
    inc += lane >= k ? o : 0;
  }
  prefix[lane] = inc - mine;
  if (lane == kWave - 1) total[0] = inc;
}

// LDS, all of it dynamic (a kernel that is opted in to the large dynamic size keeps no static LDS beside it, as
// crop_boxes_kernel): the ballot words of both sides, their prefixes and totals (kPlanScratch ints), then
// slot_of_rank [Cp] | det_of_rank [Dp] | det_state [Dp] | det_old_id [Dp], Cp / Dp = C / D rounded up to the pass size,
// so that every thread of a pass owns an element.
constexpr int kPlanScratch = 2 * 2 * kWave + 2 * kWave + 8;

__global__ __launch_bounds__(kPlanThreads) void bank_plan_kernel(pcr_bank p, int Cp, int Dp) {
  extern __shared__ unsigned long long plan_lds[];
  unsigned long long *free_words = plan_lds, *born_words = plan_lds + kWave;
  int *free_prefix = reinterpret_cast<int *>(plan_lds + 2 * kWave), *born_prefix = free_prefix + kWave;
  int *totals = born_prefix + kWave;
  int *slot_of_rank = reinterpret_cast<int *>(plan_lds) + kPlanScratch, *det_of_rank = slot_of_rank + Cp;
  int *det_state = det_of_rank + Dp, *det_old_id = det_state + Dp;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int C = p.C, D = p.D;
  const int first_id = p.next_id[0];                        // every thread reads it here; thread 0 writes it at the end

  // ---- 1. the old state: which slots are free, which detections are matched or newborn -----------------------------
  if (tid < kWave) free_words[tid] = 0ull, born_words[tid] = 0ull;
  __syncthreads();
  for (int base = 0; base < Cp; base += kPlanThreads) {
    const int s = base + tid;
    const unsigned long long bal = __ballot(s < C && p.ids[s] < 0);
    if (lane == 0) free_words[base / kWave + wave] = bal;
  }
  for (int base = 0; base < Dp; base += kPlanThreads) {
    const int d = base + tid;
    int state = kDetNone, old_id = -1;
    if (d < D && p.det_labels[d] >= 0) {
      const int t = p.det_to_track[d];
      if (t >= 0 && t < C && p.track_to_det[t] == d && slot_matched(p, t)) {
        state = t;
        old_id = p.ids[t];
      } else if (p.born == nullptr || p.born[d] != 0) {
        state = kDetBorn;
      }
    }
    det_state[d] = state;
    det_old_id[d] = old_id;
    const unsigned long long bal = __ballot(state == kDetBorn);
    if (lane == 0) born_words[base / kWave + wave] = bal;
  }
  __syncthreads();

  // ---- 2. ranks: the k-th free slot, the k-th newborn ------------------------------------------------------------------
  if (wave == 0) scan_words(free_words, free_prefix, totals, lane);
  if (wave == 1) scan_words(born_words, born_prefix, totals + 1, lane);
  __syncthreads();
  const int n_free = totals[0], n_new = totals[1];
  for (int base = 0; base < Cp; base += kPlanThreads) {
    const int s = base + tid, w = base / kWave + wave;
    const unsigned long long word = free_words[w];
    if ((word >> lane) & 1ull) slot_of_rank[free_prefix[w] + __popcll(word & ((1ull << lane) - 1ull))] = s;
  }
  for (int base = 0; base < Dp; base += kPlanThreads) {
    const int d = base + tid, w = base / kWave + wave;
    const unsigned long long word = born_words[w];
    if ((word >> lane) & 1ull) det_of_rank[born_prefix[w] + __popcll(word & ((1ull << lane) - 1ull))] = d;
  }
  __syncthreads();

  // ---- 3. the new state.  A slot is written by its owner only, a detection's outputs by its owner only ----------------
  const int W = p.W;
  for (int base = 0; base < Cp; base += kPlanThreads) {
    const int s = base + tid, w = base / kWave + wave;
    if (s >= C) continue;
    int src = -1;
    if (p.ids[s] < 0) {
      // free before this launch: the k-th free slot takes the k-th newborn
      const unsigned long long word = free_words[w];
      const int k = free_prefix[w] + __popcll(word & ((1ull << lane) - 1ull));
      if (k < n_new) {
        const int d = det_of_rank[k];
        p.ids[s] = first_id + k;
        p.steps[s] = 1;
        p.misses[s] = 0;
        p.labels[s] = p.det_labels[d];
        p.lengths[s] = p.det_lengths[d];
        p.scores[s] = p.det_scores[d];
        for (int c = 0; c < W; ++c) p.boxes[(size_t)s * W + c] = p.det_boxes[(size_t)d * W + c];
        src = d;
      }
    } else if (slot_killed(p, s)) {
      p.ids[s] = -1, p.labels[s] = -1, p.lengths[s] = 0;
    } else if (slot_matched(p, s)) {
      const int d = p.track_to_det[s];
      p.labels[s] = p.det_labels[d];
      p.scores[s] = p.det_scores[d];
      for (int c = 0; c < W; ++c) p.boxes[(size_t)s * W + c] = p.det_boxes[(size_t)d * W + c];
      p.steps[s] = p.steps[s] + 1;
      if (p.reset_on_match) p.misses[s] = 0;
      const int len = p.det_lengths[d];
      if (p.replace_all || p.lengths[s] <= len) {
        p.lengths[s] = len;
        src = d;
      }
    } else {
      const int m = p.misses[s] + 1;
      p.misses[s] = m;
      if (m >= p.frame_limit) {
        p.ids[s] = -1, p.labels[s] = -1, p.lengths[s] = 0;
      } else if (p.propagate) {
        propagate_box(p.boxes + (size_t)s * W, W, p.carry);
        p.scores[s] = p.scores[s] * 0.01f;
        p.steps[s] = p.steps[s] + 1;
      }
    }
    p.src[s] = src;
  }
  for (int base = 0; base < Dp; base += kPlanThreads) {
    const int d = base + tid, w = base / kWave + wave;
    if (d >= D) continue;
    const int state = det_state[d];
    int slot = -1, id = -1;
    if (state >= 0) {
      slot = state, id = det_old_id[d];
    } else if (state == kDetBorn) {
      const unsigned long long word = born_words[w];
      const int k = born_prefix[w] + __popcll(word & ((1ull << lane) - 1ull));
      if (k < n_free) slot = slot_of_rank[k], id = first_id + k;
    }
    p.det_slot[d] = slot;
    p.det_id[d] = id;
  }
  if (tid == 0) {
    const int n_born = min(n_new, n_free);
    p.next_id[0] = first_id + n_born;
    p.info[0] = n_new - n_born;
  }
}

// grid (row chunk, slot): the chunks of the feature row first, then those of the xyz row.  VEC bit 0 / 1: the feature /
// xyz rows are copied in 16-byte pieces (the row size is a multiple of 4 floats and both bases are 16-byte aligned).
__global__ __launch_bounds__(kMoveThreads) void bank_move_kernel(const int *__restrict__ src,
                                                                 const float *__restrict__ det_feats,
                                                                 const float *__restrict__ det_xyz,
                                                                 float *__restrict__ feats, float *__restrict__ xyz,
                                                                 int D, int feat_floats, int xyz_floats,
                                                                 int feat_chunks, int vec) {
  const int s = blockIdx.y, d = src[s];
  if (d < 0 || d >= D) return;                              // uniform: an idle slot's workgroups leave at once
  int chunk = blockIdx.x, n = feat_floats;
  const float *from = det_feats;
  float *to = feats;
  bool wide = vec & 1;
  if (chunk >= feat_chunks) chunk -= feat_chunks, n = xyz_floats, from = det_xyz, to = xyz, wide = vec & 2;
  from += (size_t)d * n;
  to += (size_t)s * n;
  const int lo = chunk * kMoveChunk, hi = min(lo + kMoveChunk, n);
  if (wide) {
    const float4 *f4 = reinterpret_cast<const float4 *>(from);
    float4 *t4 = reinterpret_cast<float4 *>(to);
    const int lo4 = lo / 4, hi4 = hi / 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = lo4 + k * kMoveThreads + (int)threadIdx.x;
      if (i < hi4) t4[i] = f4[i];
    }
  } else {
    for (int i = lo + (int)threadIdx.x; i < hi; i += kMoveThreads) to[i] = from[i];
  }
}

// out (C, D): grid (block of 256 detections, slot); the detection's centre is taken back by every thread that needs it
__global__ __launch_bounds__(256) void bank_dist_kernel(const float *__restrict__ boxes, const int *__restrict__ ids,
                                                        const float *__restrict__ det_boxes,
                                                        const float *__restrict__ carry_inv, float *__restrict__ out,
                                                        int D, int W) {
  const int s = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float v = 0.f;
  if (ids[s] >= 0) {
    const float *db = det_boxes + (size_t)d * W;
    float px = db[0], py = db[1];
    if (carry_inv != nullptr) {
      const float x = px, y = py, z = db[2];
      px = affine_row(carry_inv, x, y, z);
      py = affine_row(carry_inv + 4, x, y, z);
    }
    const float dx = boxes[(size_t)s * W] - px, dy = boxes[(size_t)s * W + 1] - py;
    const float a = dx * dx;
    const float b = dy * dy;
    v = sqrtf(a + b);
  }
  out[(size_t)s * D + d] = v;
}

__global__ void bank_retire_kernel(const int *__restrict__ mask, int *__restrict__ labels, int *__restrict__ ids,
                                   int *__restrict__ lengths, int C) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= C) return;
  if (ids[s] >= 0 && mask[s] != 0) ids[s] = -1, labels[s] = -1, lengths[s] = 0;
}

// ---- section A11: the updater as configured, and the scene log -------------------------------------------------------

constexpr int kMaxDec = PCR_ASSOC_MAX_DECISIONS;
constexpr int kLogWords = 2 * kPlanWords;                   // ballot words of an output table of C + D rows

// the matched rule of pcr_bank_plan_rules_i32, from the OLD state and the frame's inputs only
__device__ __forceinline__ bool rules_matched(const pcr_bank_rules &p, int s) {
  if (p.ids[s] < 0 || p.track_decision[s] != 0) return false;
  const int d = p.track_to_det[s];
  if (d < 0 || d >= p.D) return false;
  return p.det_labels[d] >= 0 && p.det_to_track[d] == s && p.det_decision[d] == 0;
}

// how many set bits of a side's ballot words lie below entry i
__device__ __forceinline__ int rank_below(const unsigned long long *__restrict__ words, const int *__restrict__ prefix, int i) {
  const int w = i / kWave;
  return prefix[w] + __popcll(words[w] & ((1ull << (i & (kWave - 1))) - 1ull));
}

// a[i] of a parameter block's small array by compares: a run-time index would move the block into scratch
__device__ __forceinline__ int pick(const int (&a)[kMaxDec], int i) {
  return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3];
}

// one row of the output table, by its owner; box == nullptr: an invalid row
__device__ __forceinline__ void put_row(const pcr_bank_rules &p, int r, const float *__restrict__ box, int id, int label,
                                        float score, int flags) {
  const bool valid = box != nullptr;
  p.out_valid[r] = valid ? 1 : 0;
  p.out_ids[r] = valid ? id : -1;
  p.out_labels[r] = valid ? label : -1;
  p.out_scores[r] = valid ? score : 0.f;
  p.out_flags[r] = valid ? flags : 0;
  for (int c = 0; c < p.W; ++c) p.out_boxes[(size_t)r * p.W + c] = valid ? box[c] : 0.f;
}

// LDS, all dynamic as bank_plan_kernel's: the ballot words of the free slots and of every detection decision, their
// prefixes (kRulesScratch ints in all, the totals and the per-wave row counts behind them), then slot_of_rank [Cp] |
// det_of_rank [Dp] | det_state [Dp] | det_old_id [Dp].  det_state: a slot (matched), kDetNone, or kDetBorn - i for a
// newborn of decision i.
constexpr int kRulesSets = 1 + kMaxDec;
constexpr int kRulesScratch = kRulesSets * 2 * kWave + kRulesSets * kWave + 8 + kPlanThreads / kWave;

__global__ __launch_bounds__(kPlanThreads) void bank_plan_rules_kernel(pcr_bank_rules p, int Cp, int Dp) {
  extern __shared__ unsigned long long rules_lds[];
  unsigned long long *free_words = rules_lds, *new_words = rules_lds + kWave;          // new_words [kMaxDec][kWave]
  int *free_prefix = reinterpret_cast<int *>(rules_lds + kRulesSets * kWave), *new_prefix = free_prefix + kWave;
  int *totals = new_prefix + kMaxDec * kWave;               // [0] free slots, [1 + i] newborns of decision i
  int *wave_rows = totals + 8;
  int *slot_of_rank = reinterpret_cast<int *>(rules_lds) + kRulesScratch, *det_of_rank = slot_of_rank + Cp;
  int *det_state = det_of_rank + Dp, *det_old_id = det_state + Dp;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int C = p.C, D = p.D, W = p.W, dd = p.dd, td = p.td;
  const int first_id = p.next_id[0];                        // every thread reads it here; thread 0 writes it at the end

  // ---- 1. the old state: which slots are free, which detections are matched or new, decision by decision --------------
  for (int i = tid; i < kRulesSets * kWave; i += kPlanThreads) rules_lds[i] = 0ull;
  __syncthreads();
  for (int base = 0; base < Cp; base += kPlanThreads) {
    const int s = base + tid;
    const unsigned long long bal = __ballot(s < C && p.ids[s] < 0);
    if (lane == 0) free_words[base / kWave + wave] = bal;
  }
  for (int base = 0; base < Dp; base += kPlanThreads) {
    const int d = base + tid;
    int state = kDetNone, old_id = -1;
    if (d < D && p.det_labels[d] >= 0) {
      const int code = p.det_decision[d];
      if (code == 0) {
        const int t = p.det_to_track[d];
        if (t >= 0 && t < C && p.track_to_det[t] == d && rules_matched(p, t)) {
          state = t;
          old_id = p.ids[t];
        }
      } else if (code >= 1 && code <= dd) {
        state = kDetBorn - (code - 1);
      }
    }
    det_state[d] = state;
    det_old_id[d] = old_id;
#pragma unroll
    for (int i = 0; i < kMaxDec; ++i) {
      const unsigned long long bal = __ballot(state == kDetBorn - i);
      if (lane == 0) new_words[i * kWave + base / kWave + wave] = bal;
    }
  }
  __syncthreads();

  // ---- 2. ranks: the k-th free slot; per decision, the k-th newborn ---------------------------------------------------
  if (wave == 0) scan_words(free_words, free_prefix, totals, lane);
  if (wave >= 1 && wave <= kMaxDec) scan_words(new_words + (wave - 1) * kWave, new_prefix + (wave - 1) * kWave, totals + wave, lane);
  __syncthreads();
  // the prefix over the decisions: where decision i starts among the numbered and among the ACTIVE newborns
  int id_base[kMaxDec], act_base[kMaxDec];
  int n_new = 0, n_act = 0;
#pragma unroll
  for (int i = 0; i < kMaxDec; ++i) {
    const int n = i < dd ? totals[1 + i] : 0;
    id_base[i] = n_new, act_base[i] = n_act;
    n_new += n;
    if (i < dd && (p.det_rule[i] & PCR_RULE_ACTIVE)) n_act += n;
  }
  const int n_free = totals[0];
  for (int base = 0; base < Cp; base += kPlanThreads) {
    const int s = base + tid;
    if ((free_words[s / kWave] >> lane) & 1ull) slot_of_rank[rank_below(free_words, free_prefix, s)] = s;
  }
  for (int base = 0; base < Dp; base += kPlanThreads) {
    const int d = base + tid, state = det_state[d];
#pragma unroll
    for (int i = 0; i < kMaxDec; ++i)
      if (i < dd && state == kDetBorn - i && (p.det_rule[i] & PCR_RULE_ACTIVE))
        det_of_rank[act_base[i] + rank_below(new_words + i * kWave, new_prefix + i * kWave, d)] = d;
  }
  __syncthreads();

  // ---- 3. the new state and the output table.  A slot and its row are written by the slot's owner only, a detection's
  //         outputs and its row C + d by the detection's owner only -----------------------------------------------------------
  int rows = 0;
  for (int base = 0; base < Cp; base += kPlanThreads) {
    const int s = base + tid;
    if (s >= C) continue;
    int src = -1, rule = -1, flags = 0;                     // rule < 0: no rule word applies to the slot
    if (p.ids[s] < 0) {
      // free before this launch: the k-th free slot takes the k-th ACTIVE newborn
      const int k = rank_below(free_words, free_prefix, s);
      if (k < n_act) {
        const int d = det_of_rank[k], i = kDetBorn - det_state[d];
        int idr = 0;
#pragma unroll
        for (int q = 0; q < kMaxDec; ++q)
          if (q == i) idr = id_base[q] + rank_below(new_words + q * kWave, new_prefix + q * kWave, d);
        p.ids[s] = first_id + idr;
        p.steps[s] = 1;
        p.misses[s] = 0;
        p.labels[s] = p.det_labels[d];
        p.lengths[s] = p.det_lengths[d];
        p.scores[s] = p.det_scores[d];
        for (int c = 0; c < W; ++c) p.boxes[(size_t)s * W + c] = p.det_boxes[(size_t)d * W + c];
        src = d;
        rule = pick(p.det_rule, i);
      }
    } else if (rules_matched(p, s)) {
      const int d = p.track_to_det[s];
      p.labels[s] = p.det_labels[d];
      p.scores[s] = p.det_scores[d];
      for (int c = 0; c < W; ++c) p.boxes[(size_t)s * W + c] = p.det_boxes[(size_t)d * W + c];
      p.steps[s] = p.steps[s] + 1;
      if (p.reset_on_match) p.misses[s] = 0;
      const int len = p.det_lengths[d];
      if (p.replace_all || p.lengths[s] <= len) {
        p.lengths[s] = len;
        src = d;
      }
      rule = p.match_rule;
    } else {
      const int code = p.track_decision[s];
      const int j = code >= 1 && code <= td ? code - 1 : -1;
      if (j >= 0 && pick(p.trk_kind, j) == PCR_TRK_KEEP) {
        rule = pick(p.trk_rule, j);
      } else {
        // track_false_negative, or a track that waits
        const int m = p.misses[s] + 1;
        p.misses[s] = m;
        if (m >= p.frame_limit) {
          p.ids[s] = -1, p.labels[s] = -1, p.lengths[s] = 0;
        } else if (j >= 0) {
          propagate_box(p.boxes + (size_t)s * W, W, p.carry);
          p.scores[s] = p.scores[s] * 0.01f;
          p.steps[s] = p.steps[s] + 1;
          rule = pick(p.trk_rule, j);
          flags = 2;
        }
      }
    }
    const bool out = rule >= 0 && (rule & PCR_RULE_OUTPUT);
    if (rule >= 0 && (rule & PCR_RULE_DECOM)) flags |= 1;
    put_row(p, s, out ? p.boxes + (size_t)s * W : nullptr, p.ids[s], p.labels[s], p.scores[s], flags);
    rows += out;
    if (rule >= 0 && !(rule & PCR_RULE_ACTIVE)) p.ids[s] = -1, p.labels[s] = -1, p.lengths[s] = 0;
    p.src[s] = src;
  }
  for (int base = 0; base < Dp; base += kPlanThreads) {
    const int d = base + tid;
    if (d >= D) continue;
    const int state = det_state[d];
    int slot = -1, id = -1;
    bool out = false;
    int flags = 0;
    if (state >= 0) {
      slot = state, id = det_old_id[d];
    } else if (state <= kDetBorn) {
      const int i = kDetBorn - state;
      int rule = 0, idr = 0, act = 0;
#pragma unroll
      for (int q = 0; q < kMaxDec; ++q)
        if (q == i) {
          const int r = rank_below(new_words + q * kWave, new_prefix + q * kWave, d);
          rule = p.det_rule[q], idr = id_base[q] + r, act = act_base[q] + r;
        }
      id = first_id + idr;
      if ((rule & PCR_RULE_ACTIVE) && act < n_free) slot = slot_of_rank[act];
      out = slot < 0 && (rule & PCR_RULE_OUTPUT);
      flags = (rule & PCR_RULE_DECOM) ? 1 : 0;
    }
    p.det_slot[d] = slot;
    p.det_id[d] = id;
    put_row(p, C + d, out ? p.det_boxes + (size_t)d * W : nullptr, id, p.det_labels[d], p.det_scores[d], flags);
    rows += out;
  }
  // the valid rows: every thread's count, summed over the wave and then over the waves by thread 0
#pragma unroll
  for (int k = kWave / 2; k >= 1; k >>= 1) rows += __shfl_xor(rows, k, kWave);
  if (lane == 0) wave_rows[wave] = rows;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < kPlanThreads / kWave; ++w) total += wave_rows[w];
    p.next_id[0] = first_id + n_new;
    p.info[0] = max(n_act - n_free, 0);
    p.info[1] = total;
  }
}

// One workgroup over an R-row table (R <= kLogWords * kWave): the valid rows' ballot words, their prefix by wave 0 in two
// halves, then every valid row is written by its owner at cursor + its rank, if it fits.
__global__ __launch_bounds__(kPlanThreads) void scene_log_append_kernel(pcr_scene_log p, int Rp) {
  __shared__ unsigned long long words[kLogWords];
  __shared__ int prefix[kLogWords];
  __shared__ int total[2];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int R = p.R, W = p.W;
  int cursor = p.cursor[0];                                  // every thread reads the counters here; thread 0 writes them
  const int frame = p.frame_no[0], lost = p.dropped[0];     // at the end
  if (cursor < 0 || cursor > p.rows_max) cursor = p.rows_max;
  if (tid < kLogWords) words[tid] = 0ull;
  __syncthreads();
  for (int base = 0; base < Rp; base += kPlanThreads) {
    const int r = base + tid;
    const unsigned long long bal = __ballot(r < R && p.in_valid[r] != 0);
    if (lane == 0) words[base / kWave + wave] = bal;
  }
  __syncthreads();
  if (wave == 0) {
    scan_words(words, prefix, total, lane);
    scan_words(words + kWave, prefix + kWave, total + 1, lane);
  }
  __syncthreads();
  const int n = total[0] + total[1], room = p.rows_max - cursor;
  for (int base = 0; base < Rp; base += kPlanThreads) {
    const int r = base + tid;
    if (r >= R || !((words[r / kWave] >> lane) & 1ull)) continue;
    const int k = rank_below(words, prefix, r) + (r / kWave >= kWave ? total[0] : 0);
    if (k >= room) continue;
    const size_t at = (size_t)cursor + k;
    p.frame[at] = frame;
    p.id[at] = p.in_ids[r];
    p.label[at] = p.in_labels[r];
    p.flags[at] = p.in_flags[r];
    p.score[at] = p.in_scores[r];
    for (int c = 0; c < W; ++c) p.box[at * W + c] = p.in_boxes[(size_t)r * W + c];
  }
  if (tid == 0) {
    const int written = min(n, room);
    p.cursor[0] = cursor + written;
    p.dropped[0] = lost + (n - written);
    p.frame_no[0] = frame + 1;
  }
}

bool aligned16(const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace

PCR_EXPORT int pcr_bank_ok(int C, int D, int W, int feat_floats, int xyz_floats) {
  return C >= 1 && C <= PCR_ASSOC_MAX_OBJECTS && D >= 0 && D <= PCR_ASSOC_MAX_OBJECTS && (W == 7 || W == 9) &&
         feat_floats >= 0 && feat_floats <= PCR_BANK_MAX_ROW && xyz_floats >= 0 && xyz_floats <= PCR_BANK_MAX_ROW;
}

PCR_EXPORT int pcr_bank_plan_i32(const pcr_bank *p, pcr_stream_t stream) {
  if (!p || !pcr_bank_ok(p->C, p->D, p->W, 0, 0) || p->frame_limit < 1) return PCR_ERR_INVALID;
  if (!p->lengths || !p->boxes || !p->scores || !p->labels || !p->ids || !p->steps || !p->misses || !p->next_id ||
      !p->info || !p->track_to_det || !p->src)
    return PCR_ERR_INVALID;
  if (p->D > 0 && (!p->det_to_track || !p->det_labels || !p->det_lengths || !p->det_boxes || !p->det_scores ||
                   !p->det_slot || !p->det_id))
    return PCR_ERR_INVALID;
  const int Cp = (p->C + kPlanThreads - 1) / kPlanThreads * kPlanThreads;
  const int Dp = (p->D + kPlanThreads - 1) / kPlanThreads * kPlanThreads;
  return pcr_launch_lds<bank_plan_kernel>(dim3(1), dim3(kPlanThreads), (size_t)(kPlanScratch + Cp + 3 * Dp) * sizeof(int), pcr_s(stream),
                                          *p, Cp, Dp);
}

PCR_EXPORT int pcr_bank_move_f32(const int *src, const float *det_feats, const float *det_xyz, float *feats, float *xyz,
                                 int C, int D, int feat_floats, int xyz_floats, pcr_stream_t stream) {
  if (!pcr_bank_ok(C, D, 7, feat_floats, xyz_floats)) return PCR_ERR_INVALID;
  if (D == 0 || feat_floats + xyz_floats == 0) return PCR_OK;
  if (!src || (feat_floats > 0 && (!det_feats || !feats)) || (xyz_floats > 0 && (!det_xyz || !xyz))) return PCR_ERR_INVALID;
  const int feat_chunks = (feat_floats + kMoveChunk - 1) / kMoveChunk, xyz_chunks = (xyz_floats + kMoveChunk - 1) / kMoveChunk;
  const int vec = (feat_floats % 4 == 0 && aligned16(det_feats) && aligned16(feats) ? 1 : 0) |
                  (xyz_floats % 4 == 0 && aligned16(det_xyz) && aligned16(xyz) ? 2 : 0);
  return pcr_launch<bank_move_kernel>(dim3(feat_chunks + xyz_chunks, C), dim3(kMoveThreads), 0, pcr_s(stream), src,
                                      det_feats, det_xyz, feats, xyz, D, feat_floats, xyz_floats, feat_chunks, vec);
}

PCR_EXPORT int pcr_bank_dist_f32(const float *boxes, const int *ids, const float *det_boxes, const float *carry_inv,
                                 float *out, int C, int D, int W, pcr_stream_t stream) {
  if (!pcr_bank_ok(C, D, W, 0, 0)) return PCR_ERR_INVALID;
  if (D == 0) return PCR_OK;
  if (!boxes || !ids || !det_boxes || !out) return PCR_ERR_INVALID;
  return pcr_launch<bank_dist_kernel>(dim3((D + 255) / 256, C), dim3(256), 0, pcr_s(stream), boxes, ids, det_boxes,
                                      carry_inv, out, D, W);
}

PCR_EXPORT int pcr_bank_retire_i32(const int *mask, int *labels, int *ids, int *lengths, int C, pcr_stream_t stream) {
  if (!pcr_bank_ok(C, 0, 7, 0, 0)) return PCR_ERR_INVALID;
  if (!mask || !labels || !ids || !lengths) return PCR_ERR_INVALID;
  return pcr_launch<bank_retire_kernel>(dim3((C + 255) / 256), dim3(256), 0, pcr_s(stream), mask, labels, ids, lengths, C);
}

PCR_EXPORT int pcr_bank_rules_ok(int C, int D, int W, int dd, int td) {
  return pcr_bank_ok(C, D, W, 0, 0) && dd >= 0 && dd <= PCR_ASSOC_MAX_DECISIONS && td >= 0 && td <= PCR_ASSOC_MAX_DECISIONS;
}

static bool rule_word_ok(int r) {
  return (r & ~(PCR_RULE_OUTPUT | PCR_RULE_ACTIVE | PCR_RULE_DECOM)) == 0 && !((r & PCR_RULE_ACTIVE) && (r & PCR_RULE_DECOM));
}

PCR_EXPORT int pcr_bank_plan_rules_i32(const pcr_bank_rules *p, pcr_stream_t stream) {
  if (!p || !pcr_bank_rules_ok(p->C, p->D, p->W, p->dd, p->td) || p->frame_limit < 1) return PCR_ERR_INVALID;
  if (!rule_word_ok(p->match_rule)) return PCR_ERR_INVALID;
  for (int i = 0; i < p->dd; ++i)
    if (!rule_word_ok(p->det_rule[i])) return PCR_ERR_INVALID;
  for (int j = 0; j < p->td; ++j)
    if (!rule_word_ok(p->trk_rule[j]) || (p->trk_kind[j] != PCR_TRK_KEEP && p->trk_kind[j] != PCR_TRK_MISS)) return PCR_ERR_INVALID;
  if (!p->lengths || !p->boxes || !p->scores || !p->labels || !p->ids || !p->steps || !p->misses || !p->next_id ||
      !p->info || !p->track_to_det || !p->track_decision || !p->src || !p->out_valid || !p->out_ids || !p->out_labels ||
      !p->out_scores || !p->out_boxes || !p->out_flags)
    return PCR_ERR_INVALID;
  if (p->D > 0 && (!p->det_to_track || !p->det_labels || !p->det_lengths || !p->det_boxes || !p->det_scores ||
                   !p->det_decision || !p->det_slot || !p->det_id))
    return PCR_ERR_INVALID;
  const int Cp = (p->C + kPlanThreads - 1) / kPlanThreads * kPlanThreads;
  const int Dp = (p->D + kPlanThreads - 1) / kPlanThreads * kPlanThreads;
  return pcr_launch_lds<bank_plan_rules_kernel>(dim3(1), dim3(kPlanThreads), (size_t)(kRulesScratch + Cp + 3 * Dp) * sizeof(int),
                                                pcr_s(stream), *p, Cp, Dp);
}

PCR_EXPORT int pcr_scene_log_ok(int rows_max, int R, int W) {
  return rows_max >= 1 && rows_max <= PCR_LOG_MAX_ROWS && R >= 1 && R <= 2 * PCR_ASSOC_MAX_OBJECTS && (W == 7 || W == 9);
}

PCR_EXPORT int pcr_scene_log_append_i32(const pcr_scene_log *p, pcr_stream_t stream) {
  if (!p || !pcr_scene_log_ok(p->rows_max, p->R, p->W)) return PCR_ERR_INVALID;
  if (!p->in_valid || !p->in_ids || !p->in_labels || !p->in_scores || !p->in_boxes || !p->in_flags || !p->frame || !p->id ||
      !p->label || !p->flags || !p->score || !p->box || !p->cursor || !p->dropped || !p->frame_no)
    return PCR_ERR_INVALID;
  const int Rp = (p->R + kPlanThreads - 1) / kPlanThreads * kPlanThreads;
  return pcr_launch<scene_log_append_kernel>(dim3(1), dim3(kPlanThreads), 0, pcr_s(stream), *p, Rp);
}
