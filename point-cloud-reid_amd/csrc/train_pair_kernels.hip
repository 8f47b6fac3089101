// Training on a pair list (include/pcr.h, section C3): the scatter primitive of the feature, and the linear-attention core
// split into per-object state and per-slot apply launches that are addressed by index lists.
//
// A pair list is many-to-one: object m may be named by any number of slots, so the gradient of "gather the object a slot
// names" is a sum over those slots.  pcr_index_sum_f32 forms it with one owner per accumulator and one order of addition
// (increasing slot), so the result is the same bits on every run: no float atomics.  The fused core of
// train_attn_kernels.hip writes dk / dv of the cloud it read (kv_roll is a permutation: one writer per block); here the key /
// value state A | ks and its gradient are per OBJECT, the slots leave [dA | dks] records, and pcr_index_sum_f32 carries them
// to the objects.  tests/pair_list_ref.py restates all of it in float64.
#include <type_traits>

#include "linattn_tiles.h"

namespace {

constexpr int kSumThreads = 256, kSumPerThread = 4, kSumCols = kSumThreads * kSumPerThread;   // columns of dst per workgroup
constexpr int kSumList = 1024;                                                     // slots compacted per round

// One workgroup per (object m, chunk of kSumCols columns).  Wave 0 walks the index list kSumList slots at a time and leaves the
// LIVE slots that name m in LDS, in list order (ballot + the count of passing lanes below: an ordered compaction); then
// every thread adds the rows of those slots to its kSumPerThread accumulators, in that order.  A thread's loads of one slot
// are independent (kSumPerThread in flight), its additions per column sequential.  An index outside [0, M) equals no m.
__global__ __launch_bounds__(kSumThreads) void index_sum_kernel(const float *__restrict__ src, const int *__restrict__ idx,
                                                             const int *__restrict__ count, float *__restrict__ dst, int P,
                                                             int R) {
  __shared__ int slots[kSumList];
  __shared__ int nslots;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int m = blockIdx.x;
  const long r0 = (long)blockIdx.y * kSumCols + tid;   // (long: the last chunk's columns may pass 2^31)
  int n = count ? *count : P;
  n = n < 0 ? 0 : (n > P ? P : n);
  float acc[kSumPerThread];
#pragma unroll
  for (int u = 0; u < kSumPerThread; u++) acc[u] = 0.f;
  for (int p0 = 0; p0 < n; p0 += kSumList) {
    if (p0) __syncthreads();       // (the previous round's list is still being read)
    if (tid < kWave) {
      int base = 0;
      for (int t = 0; t < kSumList && p0 + t < n; t += kWave) {
        const int p = p0 + t + lane;
        const bool hit = p < n && idx[p] == m;
        const unsigned long long mask = __ballot(hit);
        if (hit) slots[base + (int)pcr_lanes_below(mask)] = p;
        base += __popcll(mask);
      }
      if (lane == 0) nslots = base;
    }
    __syncthreads();
    const int ns = nslots;
    for (int t = 0; t < ns; t++) {
      const float *row = src + (size_t)slots[t] * R;
      float v[kSumPerThread];
#pragma unroll
      for (int u = 0; u < kSumPerThread; u++) {
        const long r = r0 + (long)u * kSumThreads;
        v[u] = r < R ? row[r] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kSumPerThread; u++) acc[u] += v[u];
    }
  }
#pragma unroll
  for (int u = 0; u < kSumPerThread; u++) {
    const long r = r0 + (long)u * kSumThreads;
    if (r < R) dst[(size_t)m * R + r] = acc[u];
  }
}

// ----------------------------------------------------------------- indexed linear attention ----
// The arithmetic of linattn_{fwd,bwd}_mfma_kernel (train_attn_kernels.hip), tile for tile: Q' = elu(q)+1, K' = elu(k)+1,
// V' = v / L, A = sum_s K'_s V'_s^T, ks = sum_s K'_s, out_l = (Q'_l^T A) L / (Q'_l . ks + eps); Lq = Sk = L.
// q / k / v are per-OBJECT (M, ., L) blocks addressed by a batch stride.  Slot r reads the queries of object qi[r] and the
// state of object si[r]; a slot with either index outside [0, M) is dead: its output block is zeros, its backward writes
// nothing (pcr_index_sum_f32 gives such a slot to no object, given lists in which it is dead in BOTH: the caller masks
// them).  blockIdx.x = object or slot, blockIdx.y = head.
struct PairAttn {
  const float *q, *k, *v;
  long q_bs, k_bs, v_bs;       // floats between objects
  const int *qi, *si;          // (R)
  int M, L, d, H;
  const float *eps;            // one f32 on the device
  float *A, *ks;               // state: (M,H,dh,dh), (M,H,dh)
  float *out;                  // (R,d,L)
  const float *dout;           // (R,d,L)
  float *dqs;                  // (R,d,L): the slot's query gradient
  float *rec;                  // (R,H,dh*(dh+1)): the slot's [dA (dh x dh) | dks (dh)]
  const float *drec;           // (M,H,dh*(dh+1)): the records summed per object
  float *dk, *dv;
  long dk_bs, dv_bs;
};

__device__ __forceinline__ bool pair_slot_dead(const PairAttn &a, int r, int &qo, int &so) {
  qo = a.qi[r];
  so = a.si[r];
  return qo < 0 || qo >= a.M || so < 0 || so >= a.M;
}

// per (object, head): A and ks of the object's own keys / values
template <int DH>
__global__ __launch_bounds__(256) void pair_state_fwd_kernel(PairAttn a) {
  constexpr int RP = kAT + 1, MT = DH / 32;
  __shared__ float Kt[DH * RP], Vt[DH * RP];
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t m = blockIdx.x;
  const int h = blockIdx.y;
  const float *k = a.k + m * a.k_bs + (size_t)h * DH * a.L;
  const float *v = a.v + m * a.v_bs + (size_t)h * DH * a.L;
  const float sk = (float)a.L;
  f32x16 accA = zero16();              // tile `wave` of A (MT x MT tiles; DH = 32: wave 0 only)
  const bool a_owner = wave < MT * MT;
  const int amt = wave / MT, ant = wave % MT;
  float ksum = 0.f;
  for (int s0 = 0; s0 < a.L; s0 += kAT) {
    const int ns = a.L - s0 < kAT ? a.L - s0 : kAT;
    if (s0) __syncthreads();
    stage_pair<DH>(Kt, Vt, k, v, a.L, s0, ns, [](float x) { return elu1f(x); }, [&](float x) { return x / sk; });
    __syncthreads();
    const int KT = ns > 32 ? 64 : 32;      // (the padding tokens are zeros)
    if (a_owner)
      accA = mm_tile(KT, [&](int mm, int kk) { return Kt[(amt * 32 + mm) * RP + kk]; },
                     [&](int n, int kk) { return Vt[(ant * 32 + n) * RP + kk]; }, accA);
    if (tid < DH) {
      const float *kr = Kt + tid * RP;
      float s = 0.f;
      for (int t = 0; t < kAT; t++) s += kr[t];
      ksum += s;
    }
  }
  float *Ag = a.A + (m * a.H + h) * DH * DH;
  if (a_owner) mm_each(accA, [&](int mm, int n, float val) { Ag[(amt * 32 + mm) * DH + ant * 32 + n] = val; });
  if (tid < DH) a.ks[(m * a.H + h) * DH + tid] = ksum;
}

// A | ks of object `so` into LDS (A padded to DH + 1 floats per row), every load in flight before the first LDS write
template <int DH>
__device__ __forceinline__ void pair_load_state(const PairAttn &a, size_t so, int h, float *Al, float *ksl) {
  constexpr int AP = DH + 1, NA = DH * DH / 256;
  const int tid = threadIdx.x;
  const float *Ag = a.A + (so * a.H + h) * DH * DH;
  float va[NA];
#pragma unroll
  for (int u = 0; u < NA; u++) va[u] = Ag[tid + u * 256];
#pragma unroll
  for (int u = 0; u < NA; u++) {
    const int e = tid + u * 256;
    Al[(e / DH) * AP + e % DH] = va[u];
  }
  if (tid < DH) ksl[tid] = a.ks[(so * a.H + h) * DH + tid];
}

// per (slot, head): the queries of object qi[r] against the state of object si[r]
template <int DH>
__global__ __launch_bounds__(256) void pair_apply_fwd_kernel(PairAttn a) {
  constexpr int RP = kAT + 1, AP = DH + 1, MT = DH / 32, NT = kAT / 32;
  __shared__ float Qt[DH * RP], Al[DH * AP], ksl[DH], zl[kAT];
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const int h = blockIdx.y;
  float *out = a.out + (r * a.d + (size_t)h * DH) * a.L;
  int qo, so;
  if (pair_slot_dead(a, (int)r, qo, so)) {          // (workgroup-uniform)
    for (int e = tid; e < DH * a.L; e += 256) out[e] = 0.f;
    return;
  }
  const float *q = a.q + (size_t)qo * a.q_bs + (size_t)h * DH * a.L;
  const float sk = (float)a.L;
  const float eps = *a.eps;
  pair_load_state<DH>(a, (size_t)so, h, Al, ksl);
  for (int l0 = 0; l0 < a.L; l0 += kAT) {
    const int nl = a.L - l0 < kAT ? a.L - l0 : kAT;
    __syncthreads();
    stage_pair<DH>(Qt, (float *)nullptr, q, (const float *)nullptr, a.L, l0, nl, [](float x) { return elu1f(x); },
                   [](float x) { return x; });
    __syncthreads();
    if (tid < kAT) {
      float z = 0.f;
      for (int i = 0; i < DH; i++) z += Qt[i * RP + tid] * ksl[i];
      zl[tid] = tid < nl ? 1.0f / (z + eps) : 0.f;       // (a padding token has Q' = 0: 1 / eps, inf at eps = 0)
    }
    __syncthreads();
    for (int tile = wave; tile < MT * NT; tile += 4) {      // out[v][l] = sum_i A[i][v] Q'[i][l]
      const int mt = tile / NT, nt = tile % NT;
      if (nt * 32 >= nl) continue;
      const f32x16 acc = mm_tile(DH, [&](int mm, int kk) { return Al[kk * AP + mt * 32 + mm]; },
                                 [&](int n, int kk) { return Qt[kk * RP + nt * 32 + n]; }, zero16());
      mm_each(acc, [&](int mm, int n, float val) {
        const int vv = mt * 32 + mm, l = nt * 32 + n;
        if (l < nl) out[(size_t)vv * a.L + l0 + l] = val * zl[l] * sk;
      });
    }
  }
}

// per (slot, head): dq of the slot, and its record [dA = sum_l Q'_l dnum_l^T | dks = sum_l dden_l Q'_l]
template <int DH>
__global__ __launch_bounds__(256) void pair_apply_bwd_kernel(PairAttn a) {
  constexpr int RP = kAT + 1, AP = DH + 1, MT = DH / 32, NT = kAT / 32;
  extern __shared__ __attribute__((aligned(16))) float smem[];    // 67 KB at DH = 64: dynamic
  float *Qt = smem, *Gt = Qt + DH * RP, *Dn = Gt + DH * RP, *Al = Dn + DH * RP;
  float *ksl = Al + DH * AP, *zl = ksl + DH, *ddl = zl + kAT;
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const int h = blockIdx.y;
  int qo, so;
  if (pair_slot_dead(a, (int)r, qo, so)) return;     // (workgroup-uniform; nothing of a dead slot is read later)
  const float *q = a.q + (size_t)qo * a.q_bs + (size_t)h * DH * a.L;
  const float *go = a.dout + (r * a.d + (size_t)h * DH) * a.L;
  float *dq = a.dqs + (r * a.d + (size_t)h * DH) * a.L;
  const float sk = (float)a.L;
  const float eps = *a.eps;
  pair_load_state<DH>(a, (size_t)so, h, Al, ksl);
  f32x16 accdA = zero16();             // tile `wave` of dA
  const bool a_owner = wave < MT * MT;
  const int amt = wave / MT, ant = wave % MT;
  float dks = 0.f;
  for (int l0 = 0; l0 < a.L; l0 += kAT) {
    const int nl = a.L - l0 < kAT ? a.L - l0 : kAT;
    const int KT = nl > 32 ? 64 : 32;
    __syncthreads();
    stage_pair<DH>(Qt, Gt, q, go, a.L, l0, nl, [](float x) { return elu1f(x); }, [](float x) { return x; });
    __syncthreads();
    if (tid < kAT) {
      float z = 0.f;
      for (int i = 0; i < DH; i++) z += Qt[i * RP + tid] * ksl[i];
      zl[tid] = tid < nl ? 1.0f / (z + eps) : 0.f;       // padding tokens inert at every eps: Dn = ddl = 0, never inf 0
    }
    __syncthreads();
    // num[v][l] = Q'_l . A[:,v];  dnum = dout z L;  dout * num * L is summed over v into dz below
    for (int tile = wave; tile < MT * NT; tile += 4) {
      const int mt = tile / NT, nt = tile % NT;
      if (nt * 32 >= KT) continue;
      const f32x16 acc = mm_tile(DH, [&](int mm, int kk) { return Al[kk * AP + mt * 32 + mm]; },
                                 [&](int n, int kk) { return Qt[kk * RP + nt * 32 + n]; }, zero16());
      mm_each(acc, [&](int mm, int n, float num) {
        const int vv = mt * 32 + mm, l = nt * 32 + n;
        const float gv = Gt[vv * RP + l];
        Dn[vv * RP + l] = gv * zl[l] * sk;
        Gt[vv * RP + l] = gv * num * sk;
      });
    }
    __syncthreads();
    if (tid < kAT) {
      float dz = 0.f;
      if (tid < KT)
        for (int vv = 0; vv < DH; vv++) dz += Gt[vv * RP + tid];
      ddl[tid] = -zl[tid] * zl[tid] * dz;      // gradient of the denominator Q'.ks + eps (zero on padding tokens)
    }
    __syncthreads();
    for (int tile = wave; tile < MT * NT; tile += 4) {      // dq[i][l] = ddl[l] ks[i] + sum_v A[i][v] dnum[v][l]
      const int mt = tile / NT, nt = tile % NT;
      if (nt * 32 >= nl) continue;
      const f32x16 acc = mm_tile(DH, [&](int mm, int kk) { return Al[(mt * 32 + mm) * AP + kk]; },
                                 [&](int n, int kk) { return Dn[kk * RP + nt * 32 + n]; }, zero16());
      mm_each(acc, [&](int mm, int n, float val) {
        const int i = mt * 32 + mm, l = nt * 32 + n;
        const float qp = Qt[i * RP + l];
        if (l < nl) dq[(size_t)i * a.L + l0 + l] = (val + ddl[l] * ksl[i]) * (qp > 1.0f ? 1.0f : qp);   // elu' = 1 | Q'
      });
    }
    if (a_owner)
      accdA = mm_tile(KT, [&](int mm, int kk) { return Qt[(amt * 32 + mm) * RP + kk]; },
                      [&](int n, int kk) { return Dn[(ant * 32 + n) * RP + kk]; }, accdA);
    if (tid < DH) {
      const float *qr = Qt + tid * RP;
      float s = 0.f;
      for (int t = 0; t < KT; t++) s += ddl[t] * qr[t];
      dks += s;
    }
  }
  float *rec = a.rec + (r * a.H + h) * (size_t)(DH * (DH + 1));
  if (a_owner) mm_each(accdA, [&](int mm, int n, float val) { rec[(amt * 32 + mm) * DH + ant * 32 + n] = val; });
  if (tid < DH) rec[DH * DH + tid] = dks;
}

// per (object, head): dK' = dA V' + dks, dV' = dA^T K' from the object's summed record and its own k, v
template <int DH>
__global__ __launch_bounds__(256) void pair_state_bwd_kernel(PairAttn a) {
  constexpr int RP = kAT + 1, AP = DH + 1, MT = DH / 32, NT = kAT / 32, NA = DH * DH / 256;
  __shared__ float Kt[DH * RP], Vt[DH * RP], dAl[DH * AP], dksl[DH];
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t m = blockIdx.x;
  const int h = blockIdx.y;
  const float *k = a.k + m * a.k_bs + (size_t)h * DH * a.L;
  const float *v = a.v + m * a.v_bs + (size_t)h * DH * a.L;
  float *dk = a.dk + m * a.dk_bs + (size_t)h * DH * a.L;
  float *dv = a.dv + m * a.dv_bs + (size_t)h * DH * a.L;
  const float sk = (float)a.L;
  const float *rec = a.drec + (m * a.H + h) * (size_t)(DH * (DH + 1));
  {
    float va[NA];
#pragma unroll
    for (int u = 0; u < NA; u++) va[u] = rec[tid + u * 256];
#pragma unroll
    for (int u = 0; u < NA; u++) {
      const int e = tid + u * 256;
      dAl[(e / DH) * AP + e % DH] = va[u];
    }
  }
  if (tid < DH) dksl[tid] = rec[DH * DH + tid];
  for (int s0 = 0; s0 < a.L; s0 += kAT) {
    const int ns = a.L - s0 < kAT ? a.L - s0 : kAT;
    __syncthreads();
    stage_pair<DH>(Kt, Vt, k, v, a.L, s0, ns, [](float x) { return elu1f(x); }, [&](float x) { return x / sk; });
    __syncthreads();
    for (int tile = wave; tile < MT * NT; tile += 4) {
      const int mt = tile / NT, nt = tile % NT;
      if (nt * 32 >= ns) continue;
      const f32x16 ak = mm_tile(DH, [&](int mm, int kk) { return dAl[(mt * 32 + mm) * AP + kk]; },
                                [&](int n, int kk) { return Vt[kk * RP + nt * 32 + n]; }, zero16());
      const f32x16 av = mm_tile(DH, [&](int mm, int kk) { return dAl[kk * AP + mt * 32 + mm]; },
                                [&](int n, int kk) { return Kt[kk * RP + nt * 32 + n]; }, zero16());
      const int l31 = threadIdx.x & 31, hh = (threadIdx.x >> 5) & 1, s = nt * 32 + l31;
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const int i = mt * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * hh;
        if (s < ns) {
          const float kp = Kt[i * RP + s];
          dk[(size_t)i * a.L + s0 + s] = (ak[rr] + dksl[i]) * (kp > 1.0f ? 1.0f : kp);
          dv[(size_t)i * a.L + s0 + s] = av[rr] / sk;
        }
      }
    }
  }
}

template <class F>
int dh_dispatch(int d, int H, F f) {      // head width 32 or 64 (pcr_linattn_pairs_ok)
  if (d / H == 32) return f(std::integral_constant<int, 32>());
  return f(std::integral_constant<int, 64>());
}

}  // namespace

PCR_EXPORT int pcr_index_sum_f32(const float *src, const int *idx, const int *count, float *dst, int P, int M, int R,
                                 pcr_stream_t stream) {
  const long chunks = ((long)R + kSumCols - 1) / kSumCols;          // grid.y: a 16-bit dimension
  if (P < 0 || M < 0 || R < 1 || chunks > 65535) return PCR_ERR_INVALID;
  if (M == 0) return PCR_OK;
  if (!dst || (P > 0 && (!src || !idx))) return PCR_ERR_INVALID;
  return pcr_launch<index_sum_kernel>(dim3(M, (unsigned)chunks), dim3(kSumThreads), 0, pcr_s(stream), src, idx, count, dst, P,
                                      R);
}

PCR_EXPORT int pcr_linattn_pairs_ok(int d, int H) {
  return d >= 1 && H >= 1 && H <= 65535 && d % H == 0 && (d / H == 32 || d / H == 64);
}

PCR_EXPORT int pcr_linattn_state_fwd_f32(const float *k, const float *v, int kv_bs, float *A, float *ks, int M, int L, int d,
                                         int H, pcr_stream_t stream) {
  if (!pcr_linattn_pairs_ok(d, H) || M < 0 || L < 1 || !k || !v || !A || !ks) return PCR_ERR_INVALID;
  if (M == 0) return PCR_OK;
  PairAttn a{};
  a.k = k; a.v = v; a.k_bs = a.v_bs = kv_bs; a.A = A; a.ks = ks; a.M = M; a.L = L; a.d = d; a.H = H;
  return dh_dispatch(d, H, [&](auto tag) {
    return pcr_launch<pair_state_fwd_kernel<decltype(tag)::value>>(dim3(M, H), dim3(256), 0, pcr_s(stream), a);
  });
}

PCR_EXPORT int pcr_linattn_apply_fwd_f32(const float *q, int q_bs, const float *A, const float *ks, const int *qi,
                                         const int *si, const float *eps, float *out, int M, int R, int L, int d, int H,
                                         pcr_stream_t stream) {
  if (!pcr_linattn_pairs_ok(d, H) || M < 0 || R < 0 || L < 1 || !q || !A || !ks || !qi || !si || !eps || !out)
    return PCR_ERR_INVALID;
  if (R == 0) return PCR_OK;
  PairAttn a{};
  a.q = q; a.q_bs = q_bs; a.A = const_cast<float *>(A); a.ks = const_cast<float *>(ks); a.qi = qi; a.si = si; a.eps = eps;
  a.out = out; a.M = M; a.L = L; a.d = d; a.H = H;
  return dh_dispatch(d, H, [&](auto tag) {
    return pcr_launch<pair_apply_fwd_kernel<decltype(tag)::value>>(dim3(R, H), dim3(256), 0, pcr_s(stream), a);
  });
}

PCR_EXPORT int pcr_linattn_apply_bwd_f32(const float *q, int q_bs, const float *A, const float *ks, const int *qi,
                                         const int *si, const float *eps, const float *dout, float *dqs, float *rec, int M,
                                         int R, int L, int d, int H, pcr_stream_t stream) {
  if (!pcr_linattn_pairs_ok(d, H) || M < 0 || R < 0 || L < 1 || !q || !A || !ks || !qi || !si || !eps || !dout || !dqs || !rec)
    return PCR_ERR_INVALID;
  if (R == 0) return PCR_OK;
  PairAttn a{};
  a.q = q; a.q_bs = q_bs; a.A = const_cast<float *>(A); a.ks = const_cast<float *>(ks); a.qi = qi; a.si = si; a.eps = eps;
  a.dout = dout; a.dqs = dqs; a.rec = rec; a.M = M; a.L = L; a.d = d; a.H = H;
  return dh_dispatch(d, H, [&](auto tag) {
    constexpr int DH = decltype(tag)::value;
    const size_t lds = (3 * (size_t)DH * (kAT + 1) + (size_t)DH * (DH + 1) + DH + 2 * kAT) * sizeof(float);
    return pcr_launch_lds<pair_apply_bwd_kernel<DH>>(dim3(R, H), dim3(256), lds, pcr_s(stream), a);
  });
}

PCR_EXPORT int pcr_linattn_state_bwd_f32(const float *k, const float *v, int kv_bs, const float *drec, float *dk, float *dv,
                                         int dkv_bs, int M, int L, int d, int H, pcr_stream_t stream) {
  if (!pcr_linattn_pairs_ok(d, H) || M < 0 || L < 1 || !k || !v || !drec || !dk || !dv) return PCR_ERR_INVALID;
  if (M == 0) return PCR_OK;
  PairAttn a{};
  a.k = k; a.v = v; a.k_bs = a.v_bs = kv_bs; a.drec = drec; a.dk = dk; a.dv = dv; a.dk_bs = a.dv_bs = dkv_bs;
  a.M = M; a.L = L; a.d = d; a.H = H;
  return dh_dispatch(d, H, [&](auto tag) {
    return pcr_launch<pair_state_bwd_kernel<decltype(tag)::value>>(dim3(M, H), dim3(256), 0, pcr_s(stream), a);
  });
}
