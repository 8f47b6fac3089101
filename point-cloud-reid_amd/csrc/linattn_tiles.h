// The tile steps shared by the linear-attention training kernels (train_attn_kernels.hip: the fused core per cloud;
// train_pair_kernels.hip: the same core split into per-object state and per-slot apply launches): staging a pair of
// (DH x 64-token) tiles, and the small matrix products on v_mfma_f32_32x32x2_f32.
#pragma once

#include "tile_dense.h"

constexpr int kAT = 64;        // tokens per staged chunk

__device__ __forceinline__ float elu1f(float x) { return x > 0.f ? x + 1.0f : __expf(x); }

template <class AF, class BF>
__device__ __forceinline__ f32x16 mm_tile(int K, AF af, BF bf, f32x16 acc) {
  const int l31 = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
#pragma unroll 8
  for (int ks = 0; ks < K / 2; ks++)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af(l31, 2 * ks + h), bf(l31, 2 * ks + h), acc, 0, 0, 0);
  return acc;
}
template <class F>
__device__ __forceinline__ void mm_each(const f32x16 &acc, F f) {   // f(m, n, value) over the lane's 16 results
  const int l31 = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
#pragma unroll
  for (int r = 0; r < 16; r++) f((r & 3) + 8 * (r >> 2) + 4 * h, l31, acc[r]);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; r++) z[r] = 0.f;
  return z;
}

// Two (DH x 64-token) tiles into LDS, every global load of a thread in flight before its first LDS write (a load ->
// store loop serialises on the load latency: 8 .. 16 round trips per tile and tensor).
template <int DH, class FA, class FB>
__device__ __forceinline__ void stage_pair(float *dA, float *dB, const float *sA, const float *sB, int Lrow, int l0,
                                           int nl, FA fa, FB fb) {
  constexpr int RP = kAT + 1, NE = DH * kAT / 256;
  float va[NE], vb[NE];
#pragma unroll
  for (int u = 0; u < NE; u++) {
    const int e = threadIdx.x + u * 256, i = e / kAT, l = e % kAT;
    const bool ok = l < nl;
    const size_t o = (size_t)i * Lrow + l0 + (ok ? l : 0);
    va[u] = sA[o];
    vb[u] = sB ? sB[o] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < NE; u++) {
    const int e = threadIdx.x + u * 256, i = e / kAT, l = e % kAT;
    const bool ok = l < nl;
    dA[i * RP + l] = ok ? fa(va[u]) : 0.f;
    if (dB) dB[i * RP + l] = ok ? fb(vb[u]) : 0.f;
  }
}
