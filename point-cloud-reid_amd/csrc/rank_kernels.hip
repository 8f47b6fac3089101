// Ranking a gallery on the device (include/pcr.h, section A8): the score matrix from a pair list, the ranking of every query's
// row -- top-k, the first hit and the average precision against identities -- and the table an evaluation over chunks of
// queries adds them to.  Every entry is a fixed-shape launch without a host read, an allocation or an atomic, and writes
// the same bits on every run.  Section A12 ranks rows too wide for LDS (rank_wide_kernel): the same rules and bits, the row
// in global memory, integer LDS adds only (their sum does not depend on the order).
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the binary64 quotients and sums are compared bit for bit
// with the CPU restatement (tests/rank_ref.py).
#include "pcr_common.h"

namespace {

constexpr float kNegInf = -__builtin_inff();

// ---- the score matrix ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_fill_kernel(float *__restrict__ scores, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) scores[i] = kNegInf;
}

__global__ __launch_bounds__(256) void rank_scatter_kernel(const float *__restrict__ logits, const int *__restrict__ pairs,
                                                           const int *__restrict__ count, float *__restrict__ scores, int Q,
                                                           int G, int cap) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  int n = count[0];
  n = n < 0 ? 0 : n > cap ? cap : n;
  if (k >= n) return;
  const int q = pairs[2 * (size_t)k], g = pairs[2 * (size_t)k + 1];
  if (q < 0 || q >= Q || g < 0 || g >= G) return;
  scores[(size_t)q * G + g] = logits[k];
}

// ---- the ranking -----------------------------------------------------------------------------------------------------------
// (order-preserving score bits, inverted index): the larger key is the better candidate.  A zero of either sign is +0, as
// the float compare has them equal; no key of a candidate is 0 (its low word is at least 2^32 - 1 - 4095; 2^32 - 2^22 over a
// wide row).
__device__ __forceinline__ unsigned long long rank_key(float s, int g) {
  const float z = s == 0.0f ? 0.0f : s;
  return ((unsigned long long)pcr_orderable(z) << 32) | (0xFFFFFFFFu - (uint32_t)g);
}

// LDS of a query: row [G] f32, a non-candidate holds -inf | hit [G] i32: the true candidates' ranks, ascending
__global__ __launch_bounds__(kWave) void rank_gallery_kernel(pcr_rank p) {
  extern __shared__ float rank_lds[];
  const int G = p.G, K = p.K, q = blockIdx.x, lane = threadIdx.x;
  float *row = rank_lds;
  int *hit = reinterpret_cast<int *>(rank_lds + G);
  const int chunks = (G + kWave - 1) / kWave;               // <= 64: lane c keeps chunk c's word of the true set
  const int qid = p.query_ids[q];
  int ex = p.exclude != nullptr ? p.exclude[q] : -1;
  if (ex < 0 || ex >= G) ex = -1;

  // ---- 1. the row: candidates, NaNs, the true set --------------------------------------------------------------------------
  int n_cand = 0, n_true = 0;
  bool flagged = false;
  unsigned long long true_word = 0ull;
  for (int c = 0; c < chunks; ++c) {
    const int g = c * kWave + lane;
    float s = kNegInf;
    if (g < G && g != ex) s = p.scores[(size_t)q * G + g];
    const bool cand = s != kNegInf;                         // (true for a NaN)
    const bool truth = cand && qid >= 0 && p.gallery_ids[g] == qid;
    if (g < G) row[g] = s;
    const unsigned long long nans = __ballot(cand && s != s);
    flagged = flagged || nans != 0ull;
    n_cand += __popcll(__ballot(cand));
    const unsigned long long tb = __ballot(truth);
    n_true += __popcll(tb);
    if (lane == c) true_word = tb;
  }
  __syncthreads();                                          // (the workgroup is this one wave)

  if (flagged) {
    for (int r = lane; r < K; r += kWave) p.topk_idx[(size_t)q * K + r] = -1, p.topk_score[(size_t)q * K + r] = kNegInf;
    if (lane == 0) p.n_cand[q] = 0, p.n_true[q] = 0, p.first_hit[q] = -1, p.ap[q] = 0.0f, p.info[q] = 1;
    return;
  }

  // ---- 2. top-k: round r takes the largest key below round r - 1's; lane r keeps the winner ------------------------------
  const int rounds = K < n_cand ? K : n_cand;
  unsigned long long below = ~0ull;
  int my_idx = -1;
  float my_score = kNegInf;
  for (int r = 0; r < rounds; ++r) {
    unsigned long long best = 0ull;
    for (int c = 0; c < chunks; ++c) {
      const int g = c * kWave + lane;
      const float s = g < G ? row[g] : kNegInf;
      const unsigned long long key = s != kNegInf ? rank_key(s, g) : 0ull;
      if (key < below && key > best) best = key;
    }
    below = pcr_wave_max_u64(best);                         // never 0: r < n_cand
    const int g = (int)(0xFFFFFFFFu - (uint32_t)below);
    if (lane == r && below != 0ull) my_idx = g, my_score = row[g];
  }
  if (lane < K) p.topk_idx[(size_t)q * K + lane] = my_idx, p.topk_score[(size_t)q * K + lane] = my_score;

  // ---- 3. the true candidates: rank, and place among the true ones, by ballot popcounts over the row --------------------
  for (int c = 0; c < chunks; ++c) {
    unsigned long long todo = wave_readlane_u64(true_word, c);
    for (int n = __popcll(todo); n > 0; --n) {
      const int g = c * kWave + __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const float sg = row[g];
      int rank = 0, place = 0;
      for (int c2 = 0; c2 < chunks; ++c2) {
        const int j = c2 * kWave + lane;
        const float sj = j < G ? row[j] : kNegInf;           // (-inf beats nothing and equals no candidate's score)
        const unsigned long long beats = __ballot(sj > sg || (sj == sg && j < g));
        rank += __popcll(beats);
        place += __popcll(beats & wave_readlane_u64(true_word, c2));
      }
      if (lane == 0) hit[place] = rank;                      // the places are a permutation of [0, n_true)
    }
  }
  __syncthreads();

  // ---- 4. average precision: the quotients by the lanes, the sum in ascending place by all of them alike -----------------
  double sum = 0.0;
  for (int base = 0; base < n_true; base += kWave) {
    const int i = base + lane;
    double quot = 0.0;
    if (i < n_true) quot = (double)(i + 1) / (double)(hit[i] + 1);
    const int m = n_true - base < kWave ? n_true - base : kWave;
    for (int l = 0; l < m; ++l) sum = sum + wave_readlane_f64(quot, l);
  }
  if (lane == 0) {
    p.n_cand[q] = n_cand;
    p.n_true[q] = n_true;
    p.first_hit[q] = n_true > 0 ? hit[0] : -1;
    p.ap[q] = n_true > 0 ? (float)(sum / (double)n_true) : 0.0f;
    p.info[q] = 0;
  }
}

// ---- a wide gallery (section A12) ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_scatter_window_kernel(const float *__restrict__ logits,
                                                                  const int *__restrict__ pairs,
                                                                  const int *__restrict__ count, float *__restrict__ scores,
                                                                  int Q, int G, int cap, int col0, int width) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;      // (cap may be near 2^31)
  int n = count[0];
  n = n < 0 ? 0 : n > cap ? cap : n;
  if (k >= n) return;
  const int q = pairs[2 * (size_t)k], g = pairs[2 * (size_t)k + 1];
  if (q < 0 || q >= Q || g < 0 || g >= width) return;
  scores[(size_t)q * G + col0 + g] = logits[k];
}

constexpr int kWideThreads = 256;                           // four waves sweep a row; no result depends on the number
constexpr int kWideTile = 1024;                             // columns per step of the sweeps
constexpr int kWidePer = kWideTile / kWideThreads;

// `truth` lanes of the wave take consecutive slots behind *counter (one integer LDS add per wave): -> the lane's slot.
// The slots of a step are a permutation of what any other order of arrival gives; both lists filled this way are read
// as sets (a maximum, a sort).
__device__ __forceinline__ int wide_append(bool take, int *counter, int lane) {
  const unsigned long long who = __ballot(take);
  if (who == 0ull) return 0;
  const int leader = __ffsll((long long)who) - 1;
  int first = 0;
  if (lane == leader) first = atomicAdd(counter, __popcll(who));
  first = __shfl(first, leader, kWave);
  return first + __popcll(who & ((1ull << lane) - 1ull));
}

// One workgroup per query; the row stays in global memory and is read twice (the second time only when there is a true
// candidate), plus min(K, n_cand) single reads of the winners' scores.  LDS (57.6 KiB, two workgroups a CU):
//   tk   [4096] u64  the true candidates' keys, sorted descending between the sweeps
//   cnt  [4096] i32  sweep 2: cnt[i] = #{candidates whose key lies in (tk[i], tk[i - 1])}, tk[i - 1] itself included;
//                    then, by a prefix sum, the rank of the true candidate at place i
//   surv [1024] u64  the keys of a step that beat the carried K-th key | win [64] u64 the carried top-k, descending, 0 = none
__global__ __launch_bounds__(kWideThreads) void rank_wide_kernel(pcr_rank p) {
  __shared__ unsigned long long tk[PCR_RANK_WIDE_MAX_TRUE];
  __shared__ unsigned long long surv[kWideTile];
  __shared__ unsigned long long win[kWave];
  __shared__ int cnt[PCR_RANK_WIDE_MAX_TRUE];
  __shared__ int part[kWideThreads];
  __shared__ int tally[5];                                  // n_cand, n_true, a NaN, the survivors appended so far (x2)
  const int G = p.G, K = p.K, q = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const float *__restrict__ row = p.scores + (size_t)q * G;
  const int qid = p.query_ids[q];
  int ex = p.exclude != nullptr ? p.exclude[q] : -1;
  if (ex < 0 || ex >= G) ex = -1;
  if (tid < kWave) win[tid] = 0ull;
  if (tid < 5) tally[tid] = 0;
  __syncthreads();

  // ---- sweep 1: candidates, NaNs, the true keys, and the top-k step by step ------------------------------------------------
  // A step's keys above the carried K-th key are appended to surv; wave 0 then selects the K largest of win + surv by
  // rank_gallery_kernel's rounds.  A key at or below the carried K-th key has K larger keys before it for good.  The two
  // append counters alternate and are never reset: a step reads the one it filled after its barrier, and the next add
  // to that one comes two steps later, behind the next step's barrier.
  int my_cand = 0, seen = 0, seen_next = 0;                // of this step's counter, of the other one
  bool my_nan = false;
  for (int base = 0, step = 0; base < G; base += kWideTile, ++step) {
    float s[kWidePer];
    int id[kWidePer];
#pragma unroll
    for (int i = 0; i < kWidePer; ++i) {
      const int g = base + i * kWideThreads + tid;
      s[i] = kNegInf, id[i] = -1;
      if (g < G && g != ex) s[i] = row[g];
      if (g < G && qid >= 0) id[i] = p.gallery_ids[g];
    }
    const unsigned long long kth = win[K - 1];
    int *counter = &tally[3 + (step & 1)];
#pragma unroll
    for (int i = 0; i < kWidePer; ++i) {
      const int g = base + i * kWideThreads + tid;
      const bool cand = s[i] != kNegInf;                    // (true for a NaN)
      const bool truth = cand && qid >= 0 && id[i] == qid;
      const unsigned long long key = cand ? rank_key(s[i], g) : 0ull;
      my_cand += cand ? 1 : 0;
      my_nan = my_nan || (cand && s[i] != s[i]);
      const int slot = wide_append(truth, &tally[1], lane);
      if (truth && slot < PCR_RANK_WIDE_MAX_TRUE) tk[slot] = key;
      const bool over = key > kth;                          // (never for a non-candidate: its key is 0)
      const int at = wide_append(over, counter, lane) - seen;
      if (over) surv[at] = key;                             // at < kWideTile: a step appends at most its columns
    }
    __syncthreads();
    const int total = *counter, ns = total - seen;
    seen = seen_next, seen_next = total;
    if (ns > 0) {                                           // (the same for every thread)
      if (wave == 0) {
        const unsigned long long held = win[lane];
        unsigned long long below = ~0ull, mine = 0ull;
        for (int r = 0; r < K; ++r) {
          unsigned long long best = held < below ? held : 0ull;
          for (int c = lane; c < ns; c += kWave) {
            const unsigned long long key = surv[c];
            if (key < below && key > best) best = key;
          }
          below = pcr_wave_max_u64(best);
          if (below == 0ull) break;                         // fewer than K keys so far
          if (lane == r) mine = below;
        }
        win[lane] = mine;
      }
      __syncthreads();
    }
  }
  atomicAdd(&tally[0], my_cand);
  if (my_nan) atomicOr(&tally[2], 1);
  __syncthreads();
  const int n_cand = tally[0], n_true = tally[1];
  const bool flagged = tally[2] != 0;

  if (flagged || n_true > PCR_RANK_WIDE_MAX_TRUE) {
    for (int r = tid; r < K; r += kWideThreads) p.topk_idx[(size_t)q * K + r] = -1, p.topk_score[(size_t)q * K + r] = kNegInf;
    if (tid == 0) p.n_cand[q] = 0, p.n_true[q] = 0, p.first_hit[q] = -1, p.ap[q] = 0.0f, p.info[q] = flagged ? 1 : 2;
    return;
  }
  if (tid < K) {
    const unsigned long long key = win[tid];
    const int g = (int)(0xFFFFFFFFu - (uint32_t)key);
    p.topk_idx[(size_t)q * K + tid] = key != 0ull ? g : -1;
    p.topk_score[(size_t)q * K + tid] = key != 0ull ? row[g] : kNegInf;      // as stored: the sign of a zero included
  }
  if (n_true == 0) {
    if (tid == 0) p.n_cand[q] = n_cand, p.n_true[q] = 0, p.first_hit[q] = -1, p.ap[q] = 0.0f, p.info[q] = 0;
    return;
  }

  // ---- between the sweeps: the true keys descending (a bitonic network over the next power of two, 0 = padding) ----------
  int pow2 = 1;
  while (pow2 < n_true) pow2 <<= 1;                         // <= 4096
  for (int i = n_true + tid; i < pow2; i += kWideThreads) tk[i] = 0ull;
  for (int i = tid; i < n_true; i += kWideThreads) cnt[i] = 0;
  __syncthreads();
  for (int k = 2; k <= pow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < pow2 / 2; t += kWideThreads) {
        const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
        const unsigned long long a = tk[lo], b = tk[hi];
        if ((a < b) == ((lo & k) == 0)) tk[lo] = b, tk[hi] = a;
      }
      __syncthreads();
    }

  // ---- sweep 2: candidate j counts for the ranks of the true keys below key_j: one integer add at the first such place --
  const unsigned long long last = tk[n_true - 1];
  for (int base = 0; base < G; base += kWideTile) {
    float s[kWidePer];
#pragma unroll
    for (int i = 0; i < kWidePer; ++i) {
      const int g = base + i * kWideThreads + tid;
      s[i] = kNegInf;
      if (g < G && g != ex) s[i] = row[g];
    }
#pragma unroll
    for (int i = 0; i < kWidePer; ++i) {
      const int g = base + i * kWideThreads + tid;
      const unsigned long long key = s[i] != kNegInf ? rank_key(s[i], g) : 0ull;
      bool need = key > last;                               // otherwise it is before no true candidate
      int lo = 0, hi = n_true - 1;                          // the first place with tk[place] < key, in [lo, hi]
      for (int it = 0; it < 12 && need && lo < hi; ++it) {
        const int mid = (lo + hi) >> 1;
        if (tk[mid] < key) hi = mid; else lo = mid + 1;
      }
      for (int round = 0; round < 2; ++round) {             // the lanes of one place add once, for the two commonest places
        const unsigned long long todo = __ballot(need);
        if (todo == 0ull) break;
        const int leader = __ffsll((long long)todo) - 1, place = __shfl(lo, leader, kWave);
        const unsigned long long same = __ballot(need && lo == place);
        if (lane == leader) atomicAdd(&cnt[place], __popcll(same));
        if (lo == place) need = false;
      }
      if (need) atomicAdd(&cnt[lo], 1);
    }
  }
  __syncthreads();

  // ---- the ranks: cnt becomes its own inclusive prefix sum ------------------------------------------------------------------
  const int per = (n_true + kWideThreads - 1) / kWideThreads, from = tid * per, to = from + per < n_true ? from + per : n_true;
  int mine = 0;
  for (int i = from; i < to; ++i) mine += cnt[i];
  part[tid] = mine;
  __syncthreads();
  int run = 0;
  for (int t = 0; t < tid; ++t) run += part[t];
  for (int i = from; i < to; ++i) run += cnt[i], cnt[i] = run;
  __syncthreads();
  if (wave != 0) return;

  // ---- average precision: rank_gallery_kernel's step 4 over hit = cnt ------------------------------------------------------
  const int *hit = cnt;
  double sum = 0.0;
  for (int b = 0; b < n_true; b += kWave) {
    const int i = b + lane;
    double quot = 0.0;
    if (i < n_true) quot = (double)(i + 1) / (double)(hit[i] + 1);
    const int m = n_true - b < kWave ? n_true - b : kWave;
    for (int l = 0; l < m; ++l) sum = sum + wave_readlane_f64(quot, l);
  }
  if (lane == 0) {
    p.n_cand[q] = n_cand;
    p.n_true[q] = n_true;
    p.first_hit[q] = hit[0];
    p.ap[q] = (float)(sum / (double)n_true);
    p.info[q] = 0;
  }
}

// ---- the table -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rank_accumulate_kernel(pcr_rank_acc p) {
  const int lane = threadIdx.x;
  int n = p.Q;
  if (p.valid != nullptr) {
    const int v = p.valid[0];
    n = v < 0 ? 0 : v > p.Q ? p.Q : v;
  }
  int scored = 0, unscored = 0, flagged = 0;
  int cmc[PCR_RANK_MAX_RANKS];
#pragma unroll
  for (int i = 0; i < PCR_RANK_MAX_RANKS; ++i) cmc[i] = 0;
  double sum_ap = p.sums[0], sum_rr = p.sums[1];
  for (int base = 0; base < n; base += kWave) {
    const int q = base + lane;
    const bool in = q < n;
    const int info = in ? p.info[q] : 0, nt = in ? p.n_true[q] : 0, fh = in ? p.first_hit[q] : 0;
    const bool is_flagged = in && info != 0, is_scored = in && info == 0 && nt > 0;
    double ap = 0.0, rr = 0.0;
    if (is_scored) ap = (double)p.ap[q], rr = 1.0 / (double)(fh + 1);
    unsigned long long todo = __ballot(is_scored);
    scored += __popcll(todo);
    flagged += __popcll(__ballot(is_flagged));
    unscored += __popcll(__ballot(in && !is_flagged && !is_scored));
#pragma unroll
    for (int i = 0; i < PCR_RANK_MAX_RANKS; ++i)
      if (i < p.nranks) cmc[i] += __popcll(__ballot(is_scored && fh < p.ranks[i]));
    for (int k = __popcll(todo); k > 0; --k) {               // the scored queries, ascending
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      sum_ap = sum_ap + wave_readlane_f64(ap, l);
      sum_rr = sum_rr + wave_readlane_f64(rr, l);
    }
  }
  if (lane == 0) {
    p.counts[0] += scored;
    p.counts[1] += unscored;
    p.counts[2] += flagged;
    p.sums[0] = sum_ap;
    p.sums[1] = sum_rr;
  }
#pragma unroll
  for (int i = 0; i < PCR_RANK_MAX_RANKS; ++i)
    if (lane == 0 && i < p.nranks) p.counts[3 + i] += cmc[i];
}

}  // namespace

PCR_EXPORT int pcr_rank_ok(int Q, int G, int K, int cap) {
  return Q >= 0 && Q <= PCR_RANK_MAX_QUERIES && G >= 0 && G <= PCR_RANK_MAX_GALLERY && K >= 1 && K <= PCR_RANK_MAX_K &&
         cap >= 0 && (long long)cap <= (long long)Q * G;
}

PCR_EXPORT int pcr_rank_scores_f32(const float *logits, const int *pairs, const int *count, float *scores, int Q, int G,
                                   int cap, pcr_stream_t stream) {
  if (!pcr_rank_ok(Q, G, 1, cap)) return PCR_ERR_INVALID;
  if (Q == 0 || G == 0) return PCR_OK;
  if (!scores || (cap > 0 && (!logits || !pairs || !count))) return PCR_ERR_INVALID;
  const long long total = (long long)Q * G;
  const int st = pcr_launch<rank_fill_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, pcr_s(stream), scores, total);
  if (st != PCR_OK || cap == 0) return st;
  return pcr_launch<rank_scatter_kernel>(dim3((cap + 255) / 256), dim3(256), 0, pcr_s(stream), logits, pairs, count, scores, Q,
                                         G, cap);
}

PCR_EXPORT int pcr_rank_gallery_f32(const pcr_rank *p, pcr_stream_t stream) {
  if (!p || !pcr_rank_ok(p->Q, p->G, p->K, 0)) return PCR_ERR_INVALID;
  if (p->Q == 0) return PCR_OK;
  if (!p->query_ids || !p->topk_idx || !p->topk_score || !p->n_cand || !p->n_true || !p->first_hit || !p->ap || !p->info)
    return PCR_ERR_INVALID;
  if (p->G > 0 && (!p->scores || !p->gallery_ids)) return PCR_ERR_INVALID;
  return pcr_launch<rank_gallery_kernel>(dim3(p->Q), dim3(kWave), (size_t)2 * p->G * sizeof(float), pcr_s(stream), *p);
}

PCR_EXPORT int pcr_rank_wide_ok(int Q, int G, int K) {
  return Q >= 0 && Q <= PCR_RANK_MAX_QUERIES && G >= 0 && G <= PCR_RANK_WIDE_MAX_GALLERY && K >= 1 && K <= PCR_RANK_MAX_K;
}

PCR_EXPORT int pcr_rank_fill_f32(float *scores, int Q, int G, pcr_stream_t stream) {
  if (!pcr_rank_wide_ok(Q, G, 1)) return PCR_ERR_INVALID;
  const long long total = (long long)Q * G;
  if (total == 0) return PCR_OK;
  if (!scores) return PCR_ERR_INVALID;
  return pcr_launch<rank_fill_kernel>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, pcr_s(stream), scores, total);
}

PCR_EXPORT int pcr_rank_scatter_f32(const float *logits, const int *pairs, const int *count, float *scores, int Q, int G,
                                    int cap, int col0, int width, pcr_stream_t stream) {
  if (!pcr_rank_wide_ok(Q, G, 1) || col0 < 0 || width < 0 || (long long)col0 + width > G || cap < 0 ||
      (long long)cap > (long long)Q * width)
    return PCR_ERR_INVALID;
  if (cap == 0) return PCR_OK;
  if (!logits || !pairs || !count || !scores) return PCR_ERR_INVALID;
  return pcr_launch<rank_scatter_window_kernel>(dim3((unsigned)(((long long)cap + 255) / 256)), dim3(256), 0, pcr_s(stream),
                                                logits, pairs, count, scores, Q, G, cap, col0, width);
}

PCR_EXPORT int pcr_rank_wide_f32(const pcr_rank *p, pcr_stream_t stream) {
  if (!p || !pcr_rank_wide_ok(p->Q, p->G, p->K)) return PCR_ERR_INVALID;
  if (p->Q == 0) return PCR_OK;
  if (!p->query_ids || !p->topk_idx || !p->topk_score || !p->n_cand || !p->n_true || !p->first_hit || !p->ap || !p->info)
    return PCR_ERR_INVALID;
  if (p->G > 0 && (!p->scores || !p->gallery_ids)) return PCR_ERR_INVALID;
  return pcr_launch<rank_wide_kernel>(dim3(p->Q), dim3(kWideThreads), 0, pcr_s(stream), *p);
}

PCR_EXPORT int pcr_rank_accumulate(const pcr_rank_acc *p, pcr_stream_t stream) {
  if (!p || !pcr_rank_ok(p->Q, p->G, 1, 0) || p->nranks < 0 || p->nranks > PCR_RANK_MAX_RANKS) return PCR_ERR_INVALID;
  for (int i = 0; i < p->nranks; ++i)
    if (p->ranks[i] < 1 || p->ranks[i] > p->G) return PCR_ERR_INVALID;
  if (!p->counts || !p->sums) return PCR_ERR_INVALID;
  if (p->Q == 0) return PCR_OK;
  if (!p->n_true || !p->first_hit || !p->info || !p->ap) return PCR_ERR_INVALID;
  return pcr_launch<rank_accumulate_kernel>(dim3(1), dim3(kWave), 0, pcr_s(stream), *p);
}
