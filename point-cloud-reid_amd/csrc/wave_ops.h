// The cross-lane primitives of the gfx950 kernels (wave64): the ONE home of the DPP move, the ds_swizzle exchange and what
// is built from them.  Included through pcr_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- the DPP move ---------------------------------------------------------------------------------------------------
// dpp_ctrl values.  A "row" is 16 consecutive lanes, a "quad" four.
constexpr int kDppXor1 = 0xB1;          // quad_perm [1,0,3,2]: lane ^ 1
constexpr int kDppXor2 = 0x4E;          // quad_perm [2,3,0,1]: lane ^ 2
constexpr int kDppQuadMirror = 0x1B;    // quad_perm [3,2,1,0]: lane ^ 3
constexpr int kDppHalfMirror = 0x141;   // row_half_mirror: lane ^ 7
constexpr int kDppRowMirror = 0x140;    // row_mirror: lane ^ 15
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118;   // lane - n inside the row
constexpr int kDppWaveShl1 = 0x130;     // wave_shl:1: lane + 1 across the wave
constexpr int kDppRowBcast15 = 0x142;   // lane 15 of a row to the next row (with row_mask 0xA: into rows 1 and 3)
constexpr int kDppRowBcast31 = 0x143;   // lane 31 to rows 2 and 3 (row_mask 0xC)

template <class T>
__device__ __forceinline__ int wave_bits(T v) {      // (the cross-lane builtins move 32-bit patterns and are typed int)
  static_assert(sizeof(T) == 4, "32-bit values only");
  return __builtin_bit_cast(int, v);
}

// v of the lane that CTRL names; 0 where that lane does not exist or the row is masked out
template <int CTRL, int ROW_MASK = 0xF, class T>
__device__ __forceinline__ T wave_dpp(T v) {
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, wave_bits(v), CTRL, ROW_MASK, 0xF, true));
}
// the same with bound_ctrl off: such a lane keeps `old`
template <int CTRL, int ROW_MASK = 0xF, class T>
__device__ __forceinline__ T wave_dpp_or(T old, T v) {
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(wave_bits(old), wave_bits(v), CTRL, ROW_MASK, 0xF, false));
}
template <int PATTERN, class T>
__device__ __forceinline__ T wave_swizzle(T v) {     // ds_swizzle bit mode: 0x401F = lane ^ 16, 0x7C1F = lane ^ 31, ...
  return __builtin_bit_cast(T, __builtin_amdgcn_ds_swizzle(wave_bits(v), PATTERN));
}
template <class T>
__device__ __forceinline__ T wave_readlane(T v, int lane) {
  return __builtin_bit_cast(T, __builtin_amdgcn_readlane(wave_bits(v), lane));
}

// ---- reductions -----------------------------------------------------------------------------------------------------
struct WaveAdd {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct WaveMax {     // (floats: no NaN among the operands)
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct WaveMin {
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; }
};

// THE row reduction.  Contract: afterwards EVERY lane holds op over the 16 lanes of its row, and the operands were paired
// as the xor butterfly pairs them (lane ^ 1, ^ 2, then the other quad of the 8-lane half, then the other half of the row),
// so a float sum has the bits of the `__shfl_xor` butterfly over masks 1, 2, 4, 8.  STEPS < 4 stops early: 2 = the quad,
// 3 = the half row.  Four VALU instructions with DPP operands, no LDS traffic (a __shfl_xor is a ds_bpermute round trip).
// KEEP: the moves are wave_dpp_or(v, v) -- the same values (under these four patterns every lane has a source), but v and the
// moved value may then share a register; a kernel written with one form keeps it, the generated code differs.
template <int CTRL, bool KEEP, class T>
__device__ __forceinline__ T row_move(T v) {
  if constexpr (KEEP) return wave_dpp_or<CTRL>(v, v);
  else return wave_dpp<CTRL>(v);
}
template <int STEPS = 4, bool KEEP = false, class T, class Op>
__device__ __forceinline__ T row_reduce(T v, Op op) {
  if constexpr (STEPS > 0) v = op(v, row_move<kDppXor1, KEEP>(v));
  if constexpr (STEPS > 1) v = op(v, row_move<kDppXor2, KEEP>(v));
  if constexpr (STEPS > 2) v = op(v, row_move<kDppHalfMirror, KEEP>(v));
  if constexpr (STEPS > 3) v = op(v, row_move<kDppRowMirror, KEEP>(v));
  return v;
}
// over the wave, wave-uniform: the four rows' results through v_readlane, combined as (r0 . r1) . (r2 . r3)
template <bool KEEP = false, class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
  v = row_reduce<4, KEEP>(v, op);
  const int b = wave_bits(v);
  auto row = [&](int l) __attribute__((always_inline)) { return __builtin_bit_cast(T, __builtin_amdgcn_readlane(b, l)); };
  return op(op(row(0), row(16)), op(row(32), row(48)));
}
__device__ __forceinline__ float quad_sum(float v) { return row_reduce<2>(v, WaveAdd()); }
__device__ __forceinline__ float row_sum(float v) { return row_reduce(v, WaveAdd()); }
// over the 32 lanes of each wave half, every lane (one ds_swizzle, lane ^ 16, on top of the row sums)
__device__ __forceinline__ float half_sum(float v) {
  v = row_sum(v);
  return v + wave_swizzle<0x401F>(v);
}
__device__ __forceinline__ float wave_sum_dpp(float v) { return wave_reduce(v, WaveAdd()); }
__device__ __forceinline__ float wave_max_dpp(float v) { return wave_reduce(v, WaveMax()); }
// over the dh lanes of a head, every lane (dh a wave-uniform power of two <= 64; heads are aligned lane groups)
__device__ __forceinline__ float head_sum(float a, int dh) {
  if (dh > 1) a += wave_dpp<kDppXor1>(a);
  if (dh > 2) a += wave_dpp<kDppXor2>(a);
  if (dh > 4) a += wave_dpp<kDppHalfMirror>(a);
  if (dh > 8) a += wave_dpp<kDppRowMirror>(a);
  if (dh > 16) a += wave_swizzle<0x401F>(a);
  if (dh > 32) a += __shfl_xor(a, 32, 64);
  return a;
}

// the xor butterfly through ds_bpermute (six dependent LDS round trips): every lane gets the wave's result
// (optim_kernels.hip keeps its own butterfly over doubles inside block_sum: folding it in here changes that unit's code)
__device__ __forceinline__ float wave_sum_shfl(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_max_shfl(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// ---- inclusive prefix sums ------------------------------------------------------------------------------------------
// OR0: a lane without a source reads its 0 through wave_dpp_or(0, .) instead of wave_dpp -- the same values, other generated
// code; each user keeps the form it was written and measured with.
template <int CTRL, bool OR0>
__device__ __forceinline__ int scan_move(int v) {
  if constexpr (OR0) return wave_dpp_or<CTRL>(0, v);
  else return wave_dpp<CTRL>(v);
}
template <bool OR0 = false>
__device__ __forceinline__ int row_incl_scan(int x) {      // over the lanes of each 16-lane row (four row shifts)
  x += scan_move<kDppRowShr1, OR0>(x);
  x += scan_move<kDppRowShr2, OR0>(x);
  x += scan_move<kDppRowShr4, OR0>(x);
  x += scan_move<kDppRowShr8, OR0>(x);
  return x;
}
__device__ __forceinline__ int wave_incl_scan(int x) {     // over the 64 lanes: the row scans, then the two row broadcasts
  x = row_incl_scan<true>(x);
  x += wave_dpp_or<kDppRowBcast15, 0xA>(0, x);
  x += wave_dpp_or<kDppRowBcast31, 0xC>(0, x);
  return x;
}

// ---- a wave's own LDS traffic needs no workgroup barrier, only program order: its writes before its later reads
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the number of lanes below the calling one whose bit is set in a ballot: a passing lane's slot in an ordered compaction
__device__ __forceinline__ uint32_t pcr_lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// counters[k] += the number of lanes with flag (counters: an LDS table of integer sums); every lane of the wave calls it
__device__ __forceinline__ void wave_count(int *counters, int k, bool flag, int lane) {
  const unsigned long long bal = __ballot(flag);
  if (lane == 0 && bal != 0ull) atomicAdd(&counters[k], __popcll(bal));
}

// a wave-uniform 64-bit word / binary64 out of lane `l` (wave-uniform): two v_readlane
__device__ __forceinline__ unsigned long long wave_readlane_u64(unsigned long long v, int l) {
  const uint32_t lo = wave_readlane((uint32_t)v, l), hi = wave_readlane((uint32_t)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double wave_readlane_f64(double v, int l) {
  return __longlong_as_double((long long)wave_readlane_u64((unsigned long long)__double_as_longlong(v), l));
}

__device__ __forceinline__ unsigned long long pcr_wave_max_u64(unsigned long long k) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    unsigned long long o = __shfl_xor(k, m, 64);
    k = o > k ? o : k;
  }
  return k;
}

__device__ __forceinline__ unsigned long long pcr_wave_min_u64(unsigned long long k) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    unsigned long long o = __shfl_xor(k, m, 64);
    k = o < k ? o : k;
  }
  return k;
}

// ---- sorting network over the 64 lanes of a wave (bitonic, 21 compare-exchange steps) -------------------------
// Used where a wave ranks <= 64 keys (kNN selection): a rank count over v_readlane broadcasts costs 64 x 3
// instructions for 32-bit keys and ~64 x 7 for 64-bit keys; the network costs 21 x (exchange + compare + select).
// Exchanges: xor 1 / 2 and the mirrors inside 4 / 8 / 16 lanes are DPP modifiers (no extra instruction latency),
// xor 4 / 8 / 16 and the mirror inside 32 lanes are ds_swizzle bit-mode patterns, the one cross-half step uses
// gfx950's v_permlane32_swap.  Step (K, 0) "flips" a sorted block of K/2 against its mirror neighbour, steps (K, J)
// are the xor-J merges below it; after the (64, *) group the keys ascend with the lane index.
__device__ __forceinline__ uint32_t pcr_lane_xor32(uint32_t v, bool upper_half) {
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);   // {lanes 0..31 twice, lanes 32..63 twice}
  return upper_half ? r[0] : r[1];
}

template <int K, int J>
__device__ __forceinline__ uint32_t pcr_sort_partner(uint32_t v, int lane) {
  if constexpr (J == 0) {
    if constexpr (K == 2) return wave_dpp<kDppXor1>(v);
    else if constexpr (K == 4) return wave_dpp<kDppQuadMirror>(v);
    else if constexpr (K == 8) return wave_dpp<kDppHalfMirror>(v);
    else if constexpr (K == 16) return wave_dpp<kDppRowMirror>(v);
    else if constexpr (K == 32) return wave_swizzle<0x7C1F>(v);                             // xor 31
    else return pcr_lane_xor32(wave_swizzle<0x7C1F>(v), lane >= 32);                        // xor 63
  } else {
    if constexpr (J == 1) return wave_dpp<kDppXor1>(v);
    else if constexpr (J == 2) return wave_dpp<kDppXor2>(v);
    else if constexpr (J == 4) return wave_swizzle<0x101F>(v);
    else if constexpr (J == 8) return wave_swizzle<0x201F>(v);
    else return wave_swizzle<0x401F>(v);
  }
}

#define PCR_SORT_NETWORK(STEP)                                                                      \
  STEP(2, 0, 1)                                                                                     \
  STEP(4, 0, 2) STEP(4, 1, 1)                                                                       \
  STEP(8, 0, 4) STEP(8, 2, 2) STEP(8, 1, 1)                                                         \
  STEP(16, 0, 8) STEP(16, 4, 4) STEP(16, 2, 2) STEP(16, 1, 1)                                       \
  STEP(32, 0, 16) STEP(32, 8, 8) STEP(32, 4, 4) STEP(32, 2, 2) STEP(32, 1, 1)                       \
  STEP(64, 0, 32) STEP(64, 16, 16) STEP(64, 8, 8) STEP(64, 4, 4) STEP(64, 2, 2) STEP(64, 1, 1)

// ascending over the lanes; the lower lane of a pair keeps the smaller key
__device__ __forceinline__ uint32_t pcr_wave_sort_u32(uint32_t v, int lane) {
#define PCR_STEP32(K, J, BIT)                                   \
  {                                                             \
    const uint32_t o = pcr_sort_partner<K, J>(v, lane);         \
    const bool up = (lane & BIT) != 0;                          \
    v = ((o < v) != up) ? o : v;                                \
  }
  PCR_SORT_NETWORK(PCR_STEP32)
#undef PCR_STEP32
  return v;
}

// The same network for keys that are the BITS OF NON-NEGATIVE, NON-NaN FLOATS (denormals included: the kernels run
// with float_denorm_mode_32 = 3), two VALU instructions per step instead of three plus their vcc round trip.  A
// lane that keeps the larger key of its pair holds the key NEGATED: then both lanes of a pair execute the same
// x = min(x, -partner(x)) -- for the keeper of the minimum that is min(x, y), for the keeper of the maximum
// min(-y, -x) = -max(x, y) -- and the negation of the partner is a source modifier of v_min_f32 (on the DPP operand
// where the exchange is a DPP pattern).  Between two steps a lane whose role changes flips its sign (v_cndmask with a
// negated source under a constant lane mask).  Float order on these keys is their unsigned order.
constexpr unsigned long long pcr_lane_bit_mask(int bit) {   // the lanes whose bit `bit` (a power of two, 0 = none) is set
  return bit == 1 ? 0xAAAAAAAAAAAAAAAAull : bit == 2 ? 0xCCCCCCCCCCCCCCCCull : bit == 4 ? 0xF0F0F0F0F0F0F0F0ull
       : bit == 8 ? 0xFF00FF00FF00FF00ull : bit == 16 ? 0xFFFF0000FFFF0000ull : bit == 32 ? 0xFFFFFFFF00000000ull : 0ull;
}

template <int K, int J, int BIT>
__device__ __forceinline__ uint32_t pcr_sortf_step(uint32_t v, int lane) {
  // lanes with bit BIT set keep the larger key in this step; in the previous step it was bit PREV
  constexpr int PREV = J == 0 ? (K == 2 ? 0 : 1) : 2 * BIT;
  const unsigned long long flip = pcr_lane_bit_mask(PREV) ^ pcr_lane_bit_mask(BIT);
#define PCR_SORTF_DPP(CTRL)                                                                              \
  asm("v_cndmask_b32_e64 %0, %0, -%0, %1\n\ts_nop 1\n\t"                                                \
      "v_min_f32_dpp %0, -%0, %0 " CTRL " row_mask:0xf bank_mask:0xf" : "+v"(v) : "s"(flip))
  constexpr bool dpp = (J == 0 && K <= 16) || J == 1 || J == 2 || J == 8;
  if constexpr (J == 4) {
    // xor 4 inside a row of 16: the lanes of banks 0 / 2 take lane + 4, those of banks 1 / 3 lane - 4 -- two DPP
    // minima under bank masks instead of a ds_swizzle round trip
    uint32_t w;
    asm("v_cndmask_b32_e64 %1, %1, -%1, %2\n\ts_nop 1\n\t"
        "v_min_f32_dpp %0, -%1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_min_f32_dpp %0, -%1, %1 row_shr:4 row_mask:0xf bank_mask:0xa"
        : "=&v"(w), "+v"(v) : "s"(flip));
    v = w;
  } else if constexpr (dpp) {
    if constexpr (J == 1 || (J == 0 && K == 2)) PCR_SORTF_DPP("quad_perm:[1,0,3,2]");
    else if constexpr (J == 2) PCR_SORTF_DPP("quad_perm:[2,3,0,1]");
    else if constexpr (J == 8) PCR_SORTF_DPP("row_ror:8");
    else if constexpr (K == 4) PCR_SORTF_DPP("quad_perm:[3,2,1,0]");
    else if constexpr (K == 8) PCR_SORTF_DPP("row_half_mirror");
    else PCR_SORTF_DPP("row_mirror");
  } else {
    asm("v_cndmask_b32_e64 %0, %0, -%0, %1" : "+v"(v) : "s"(flip));
    const uint32_t o = pcr_sort_partner<K, J>(v, lane);
    asm("v_min_f32_e64 %0, %1, -%2" : "=v"(v) : "v"(v), "v"(o));
  }
#undef PCR_SORTF_DPP
  return v;
}

__device__ __forceinline__ uint32_t pcr_wave_sort_posf32(uint32_t v, int lane) {
#define PCR_STEPF(K, J, BIT) v = pcr_sortf_step<K, J, BIT>(v, lane);
  PCR_SORT_NETWORK(PCR_STEPF)
#undef PCR_STEPF
  return v & 0x7FFFFFFFu;   // the last step's keepers of the maximum (odd lanes) still hold their key negated
}

__device__ __forceinline__ unsigned long long pcr_wave_sort_u64(unsigned long long key, int lane) {
  uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
#define PCR_STEP64(K, J, BIT)                                                        \
  {                                                                                  \
    const uint32_t ohi = pcr_sort_partner<K, J>(hi, lane), olo = pcr_sort_partner<K, J>(lo, lane); \
    const bool less = (((unsigned long long)ohi << 32) | olo) < (((unsigned long long)hi << 32) | lo); \
    const bool up = (lane & BIT) != 0;                                               \
    const bool take = less != up;                                                    \
    hi = take ? ohi : hi;                                                            \
    lo = take ? olo : lo;                                                            \
  }
  PCR_SORT_NETWORK(PCR_STEP64)
#undef PCR_STEP64
  return ((unsigned long long)hi << 32) | lo;
}
