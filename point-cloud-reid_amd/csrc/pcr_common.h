// Shared helpers for the gfx950 kernels of libpcr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcr.h"

#define PCR_EXPORT extern "C" __attribute__((visibility("default")))

static inline hipStream_t pcr_s(pcr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kWave = 64;
constexpr int kMaxDynLds = 160 * 1024;

// ---- launch helpers (host) ----------------------------------------------------------------------------------------
// The current device's compute-unit count, queried once (256 if the query fails): the grid cap of the persistent kernels.
static inline int pcr_cu_count() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n < 1)
      return 256;
    return n;
  }();
  return ncu;
}

// Launches KERN; PCR_OK, or PCR_ERR_LAUNCH if the runtime reports an error.
template <auto KERN, class... Args>
static inline int pcr_launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(KERN, grid, block, lds, st, args...);
  return hipGetLastError() == hipSuccess ? PCR_OK : PCR_ERR_LAUNCH;
}

// Dynamic LDS beyond the default 64 KiB: KERN is opted in to kMaxDynLds once per process.  pcr_launch_lds does it at the
// kernel's first launch; only a dispatcher whose occupancy query must see the opt-in calls it directly.
template <auto KERN>
static inline void allow_big_lds() {
  static const bool opted = hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                kMaxDynLds) == hipSuccess;
  (void)opted;
}
template <auto KERN, class... Args>
static inline int pcr_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  allow_big_lds<KERN>();
  return pcr_launch<KERN>(grid, block, lds, st, args...);
}

// Diagnostics for bench.py's roofline object: the arithmetic (PCR_PREC_*) of the matrix phases of the model launch the
// calling thread issued last (pcr_last_launch_arith, probe_kernels.hip).  Every dispatcher of section B notes what the
// kernel it launches really runs -- the requested precision is only a request (shapes a bf16 unit does not hold run f32).
void pcr_note_arith(int prec);

// Tuning / ablation knobs (PCR_SA_DBG, PCR_TD_VARIANT, ...) are read from the environment ONLY in builds made with
// -DPCR_TUNING=1 (PCR_EXTRA_HIPCC_FLAGS); the shipped library ignores the environment on its launch paths.
#ifndef PCR_TUNING
#define PCR_TUNING 0
#endif
#include <stdlib.h>
static inline const char *pcr_tune_str(const char *name) { return PCR_TUNING ? getenv(name) : nullptr; }
static inline int pcr_tune_int(const char *name) {
  const char *v = pcr_tune_str(name);
  return v ? atoi(v) : 0;
}

// (x2-x1)^2+(y2-y1)^2+(z2-z1)^2, left to right, never contracted into fma: the file is built
// with -ffp-contract=off and the products are kept in separate statements.
__device__ __forceinline__ float pcr_sqdist3(float x1, float y1, float z1, float x2, float y2,
                                             float z2) {
  float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
  float a = dx * dx;
  float b = dy * dy;
  float c = dz * dz;
  float s = a + b;
  return s + c;
}

// Monotone float -> uint32 map (total order of finite floats, -0 < +0).
__device__ __forceinline__ uint32_t pcr_orderable(float v) {
  uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The 32-bit finaliser of the counter-based generators of pcr.h (sections A2 and A6): one definition, so that the crop
// kernel's words and the crop store's are the same function by construction.
__device__ __forceinline__ uint32_t pcr_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// h of pcr.h (section A6) after (seed, stream, key): W(seed, stream, key, k) = pcr_mix32(h ^ k); pick(u, len) beside it.
// The crop store draws with streams 1 and 2, the triplet draw of section C2 with stream 3.
__device__ __forceinline__ uint32_t pcr_word_prefix(unsigned long long seed, uint32_t stream, uint32_t key) {
  uint32_t h = pcr_mix32((uint32_t)seed ^ 0x9e3779b9u);
  h = pcr_mix32(h ^ (uint32_t)(seed >> 32));
  h = pcr_mix32(h ^ stream);
  return pcr_mix32(h ^ key);
}

__device__ __forceinline__ uint32_t pcr_pick(uint32_t u, uint32_t len) {
  return (uint32_t)(((unsigned long long)u * len) >> 32);
}

#include "wave_ops.h"   // the cross-lane primitives: DPP move, row / wave reductions, scans, the wave sorting network

// ---- MFMA token (round 6).  The counters say the wave-autonomous kernels overlap almost nothing: matrix pipe busy 0.57 +
// VALU issue 0.31 of a launch's cycles with 0.10 of them in both states (SQ_VALU_MFMA_COEXEC_CYCLES; 0.014 for the kv
// kernel) -- the two waves of a SIMD run the same phases on equal blocks and fall into step, so the VALU phase of one
// does not sit under the MFMA phase of the other.  A token per SIMD (an LDS word: the waves of a workgroup that share a
// SIMD are found by HW_ID.SIMD_ID) makes the matrix phases of the SIMD's waves mutually exclusive: while one wave holds
// it and runs layers 2 / 3, the other gathers, seeds, splits, reduces -- or sleeps at the gate.
// Measured (tools/scratch/probe_coexec*.hip, one wave per SIMD with an instruction-level interleave): under a running
// v_mfma_f32_32x32x16_bf16 integer / transcendental / LDS instructions are nearly free, plain f32 VALU instructions keep
// about two of their three cycles, packed f32 instructions (v_pk_add / mul / fma_f32) hide almost nothing -- the matrix pipe and
// the f32 vector lanes are one datapath.  So the token buys what the integer part of the other wave's VALU phase is worth:
// sa_stream_kernel<4,4> 2.20-2.26 -> 2.06-2.09 ms (pt1024 SA3, same bits); the attention stream kernels (four short matrix
// phases per block, f32-heavy LayerNorm / normaliser between them) gain nothing from it (measured: 0 to -2 %): not used there.
__device__ __forceinline__ int pcr_simd_id() { return __builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4); }   // HW_ID[5:4]
__device__ __forceinline__ void mfma_token_acquire(int *tok, int lane) {
  if (!tok) return;
  __builtin_amdgcn_sched_barrier(0);
  int busy;
  do {
    int old = 1;
    if (lane == 0) old = atomicCAS(tok, 0, 1);
    busy = __builtin_amdgcn_readfirstlane(old);
    if (busy) __builtin_amdgcn_s_sleep(1);
  } while (busy);
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void mfma_token_release(int *tok, int lane) {
  if (!tok) return;
  __builtin_amdgcn_sched_barrier(0);
  if (lane == 0) __hip_atomic_store(tok, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_sched_barrier(0);
}

