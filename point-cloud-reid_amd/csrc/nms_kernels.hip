// Bird's-eye-view box overlap and duplicate suppression (include/pcr.h, section A4): nearest_bev, the three pairwise
// overlaps of the reference's iou3d extension, greedy NMS (ranking, ballot mask, one-wave sweep) and the tracker's
// pairwise suppression rule, each a fixed-shape launch without a host read.
//
// The file is built with -ffp-contract=off (pcr_amd/build.py): the axis-aligned values, the ranking and the sweep are
// compared bit for bit with the CPU restatement (tests/nms_ref.py), the rotated overlap operation for operation up to
// the last place of atan2f.
#include "pcr_common.h"

namespace {

constexpr float kBevEps = 1e-8f;          // EPS, iou3d_kernel.cu:16
constexpr float kBevMargin = 1e-5f;       // MARGIN, iou3d_kernel.cu:56
constexpr int kBevPts = 24;               // 16 edge crossings + 8 corners: what the reference's cross_points[16] can be
                                          // asked to hold; here every one of them has a slot
constexpr int kBevLds = 3 * kBevPts * kWave;   // (x, y, angle) per slot, one column per lane of a 64-thread workgroup
constexpr int kRankThreads = 256;
constexpr int kNmsFlags = 64;             // workspace words for the per-workgroup "bad input" flags (<= 16 are used)

// (cos, sin) of a BEV box's angle -- the ONLY trigonometry of this file; pcr_bev_frames_f32 writes what it returns.
// The reference also takes cos(-angle) and sin(-angle) (check_in_box2d): those are c and -s, exactly.
__device__ __forceinline__ void pcr_bev_frame(float angle, float &c, float &s) {
  c = cosf(angle);
  s = sinf(angle);
}

struct BevBox {
  float x1, y1, x2, y2, c, s;
};

struct Pt {
  float x, y;
};

__device__ __forceinline__ bool bev_non_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// iou_normal (iou3d_kernel.cu:335-343)
__device__ __forceinline__ float iou_axis(const BevBox &a, const BevBox &b) {
  const float left = fmaxf(a.x1, b.x1), right = fminf(a.x2, b.x2);
  const float top = fmaxf(a.y1, b.y1), bottom = fminf(a.y2, b.y2);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a.x2 - a.x1) * (a.y2 - a.y1);
  const float sb = (b.x2 - b.x1) * (b.y2 - b.y1);
  return inter / fmaxf(sa + sb - inter, kBevEps);
}

// cross(p1, p2, p0) (:40-43)
__device__ __forceinline__ float cross3(Pt p1, Pt p2, Pt p0) {
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// rotate_around_center (:111-119)
__device__ __forceinline__ Pt bev_rotate(float cx, float cy, float c, float s, float x, float y) {
  Pt r;
  r.x = (x - cx) * c + (y - cy) * s + cx;
  r.y = -(x - cx) * s + (y - cy) * c + cy;
  return r;
}

// check_in_box2d (:54-77): cos(-angle) = c, sin(-angle) = -s
__device__ __forceinline__ bool bev_in_box(const BevBox &b, Pt p) {
  const float cx = (b.x1 + b.x2) / 2, cy = (b.y1 + b.y2) / 2;
  const float ac = b.c, as = -b.s;
  const float rx = (p.x - cx) * ac + (p.y - cy) * as + cx;
  const float ry = -(p.x - cx) * as + (p.y - cy) * ac + cy;
  return rx > b.x1 - kBevMargin && rx < b.x2 + kBevMargin && ry > b.y1 - kBevMargin && ry < b.y2 + kBevMargin;
}

// intersection (:79-109) of the segments p0-p1 and q0-q1
__device__ __forceinline__ bool bev_intersection(Pt p1, Pt p0, Pt q1, Pt q0, Pt &ans) {
  // check_rect_cross(p0, p1, q0, q1) (:45-52)
  if (!(fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
        fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y)))
    return false;
  const float s1 = cross3(q0, p1, p0);
  const float s2 = cross3(p1, q1, p0);
  const float s3 = cross3(p0, q1, q0);
  const float s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > kBevEps) {
    ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    ans.x = (b0 * c1 - b1 * c0) / D;
    ans.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

// box_overlap (:127-242).  The polygon's points live in LDS (pts: kBevLds floats of the workgroup, this lane's column),
// so that the appends and the sort index them without a scratch-backed private array.
__device__ float bev_overlap(const BevBox &a, const BevBox &b, float *pts, int lane) {
  float *px = pts + lane, *py = pts + kBevPts * kWave + lane, *pa = pts + 2 * kBevPts * kWave + lane;
  const float acx = (a.x1 + a.x2) / 2, acy = (a.y1 + a.y2) / 2;
  const float bcx = (b.x1 + b.x2) / 2, bcy = (b.y1 + b.y2) / 2;
  Pt ca[5], cb[5];
  ca[0] = bev_rotate(acx, acy, a.c, a.s, a.x1, a.y1);
  ca[1] = bev_rotate(acx, acy, a.c, a.s, a.x2, a.y1);
  ca[2] = bev_rotate(acx, acy, a.c, a.s, a.x2, a.y2);
  ca[3] = bev_rotate(acx, acy, a.c, a.s, a.x1, a.y2);
  ca[4] = ca[0];
  cb[0] = bev_rotate(bcx, bcy, b.c, b.s, b.x1, b.y1);
  cb[1] = bev_rotate(bcx, bcy, b.c, b.s, b.x2, b.y1);
  cb[2] = bev_rotate(bcx, bcy, b.c, b.s, b.x2, b.y2);
  cb[3] = bev_rotate(bcx, bcy, b.c, b.s, b.x1, b.y2);
  cb[4] = cb[0];

  int cnt = 0;
  float sx = 0.f, sy = 0.f;                                 // poly_center
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Pt ans;
      if (bev_intersection(ca[i + 1], ca[i], cb[j + 1], cb[j], ans)) {
        sx = sx + ans.x, sy = sy + ans.y;
        px[cnt * kWave] = ans.x, py[cnt * kWave] = ans.y;
        ++cnt;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (bev_in_box(a, cb[k])) {
      sx = sx + cb[k].x, sy = sy + cb[k].y;
      px[cnt * kWave] = cb[k].x, py[cnt * kWave] = cb[k].y;
      ++cnt;
    }
    if (bev_in_box(b, ca[k])) {
      sx = sx + ca[k].x, sy = sy + ca[k].y;
      px[cnt * kWave] = ca[k].x, py[cnt * kWave] = ca[k].y;
      ++cnt;
    }
  }
  if (cnt == 0) return 0.f;                                 // (the reference's 0 / 0 centroid is never used)
  sx = sx / (float)cnt, sy = sy / (float)cnt;

  // point_cmp's angles (:121-125), once per point, then the reference's bubble sort (:215-224): cnt <= 24 passes
  for (int k = 0; k < cnt; ++k) pa[k * kWave] = atan2f(py[k * kWave] - sy, px[k * kWave] - sx);
  for (int j = 0; j < cnt - 1; ++j) {
    float hx = px[0], hy = py[0], ha = pa[0];               // the element the pass carries upwards
    for (int i = 0; i < cnt - j - 1; ++i) {
      const float nx = px[(i + 1) * kWave], ny = py[(i + 1) * kWave], na = pa[(i + 1) * kWave];
      if (ha > na) {
        px[i * kWave] = nx, py[i * kWave] = ny, pa[i * kWave] = na;
      } else {
        px[i * kWave] = hx, py[i * kWave] = hy, pa[i * kWave] = ha;
        hx = nx, hy = ny, ha = na;
      }
    }
    px[(cnt - j - 1) * kWave] = hx, py[(cnt - j - 1) * kWave] = hy, pa[(cnt - j - 1) * kWave] = ha;
  }

  const float x0 = px[0], y0 = py[0];
  float area = 0.f;
  float ux = x0 - x0, uy = y0 - y0;                         // cross_points[k] - cross_points[0]
  for (int k = 0; k < cnt - 1; ++k) {
    const float vx = px[(k + 1) * kWave] - x0, vy = py[(k + 1) * kWave] - y0;
    area = area + (ux * vy - uy * vx);
    ux = vx, uy = vy;
  }
  return fabsf(area) / 2.0f;
}

// iou_bev (:244-251)
__device__ __forceinline__ float iou_rotated(const BevBox &a, const BevBox &b, float *pts, int lane) {
  const float sa = (a.x2 - a.x1) * (a.y2 - a.y1);
  const float sb = (b.x2 - b.x1) * (b.y2 - b.y1);
  const float ov = bev_overlap(a, b, pts, lane);
  return ov / fmaxf(sa + sb - ov, kBevEps);
}

template <int KIND>
__device__ __forceinline__ float bev_pair(const BevBox &a, const BevBox &b, float *pts, int lane) {
  if constexpr (KIND == PCR_IOU_AXIS) return iou_axis(a, b);
  else if constexpr (KIND == PCR_IOU_ROTATED) return iou_rotated(a, b, pts, lane);
  else return bev_overlap(a, b, pts, lane);
}

template <int KIND>
__device__ __forceinline__ BevBox bev_load(const float *box) {
  BevBox r;
  r.x1 = box[0], r.y1 = box[1], r.x2 = box[2], r.y2 = box[3];
  r.c = 1.f, r.s = 0.f;
  if constexpr (KIND != PCR_IOU_AXIS) pcr_bev_frame(box[4], r.c, r.s);
  return r;
}

// a row of the ranked table the NMS kernels share: {x1, y1, x2, y2, cos, sin, 0, 0}
__device__ __forceinline__ BevBox bev_table(const float *table, int k) {
  const float4 lo = *reinterpret_cast<const float4 *>(table + 8 * (size_t)k);
  const float2 hi = *reinterpret_cast<const float2 *>(table + 8 * (size_t)k + 4);
  BevBox r;
  r.x1 = lo.x, r.y1 = lo.y, r.x2 = lo.z, r.y2 = lo.w, r.c = hi.x, r.s = hi.y;
  return r;
}

__global__ void nearest_bev_kernel(const float *__restrict__ boxes, float *__restrict__ out, int N) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const float *b = boxes + 7 * (size_t)k;
  const float pi = 3.14159265358979323846f, quarter = 0.78539816339744830962f;
  const float rz = b[6];
  const float r = fabsf(rz - floorf(rz / pi + 0.5f) * pi);            // |limit_period(rz, 0.5, pi)|
  const bool swap = r > quarter;
  const float w = swap ? b[4] : b[3], l = swap ? b[3] : b[4];
  float *o = out + 5 * (size_t)k;
  o[0] = b[0] - w / 2, o[1] = b[1] - l / 2, o[2] = b[0] + w / 2, o[3] = b[1] + l / 2, o[4] = 0.f;
}

__global__ void bev_frames_kernel(const float *__restrict__ boxes, float *__restrict__ frames, int N) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  float c, s;
  pcr_bev_frame(boxes[5 * (size_t)k + 4], c, s);
  frames[2 * (size_t)k] = c;
  frames[2 * (size_t)k + 1] = s;
}

// out (A,B): one wave per (row, 64 columns); the lane's column box stays in registers, the row box is uniform
template <int KIND>
__global__ __launch_bounds__(kWave) void iou_bev_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                        float *__restrict__ out, int A, int B) {
  __shared__ float pts[KIND == PCR_IOU_AXIS ? 1 : kBevLds];
  const int lane = threadIdx.x, i = blockIdx.y, j = blockIdx.x * kWave + lane;
  const BevBox bb = bev_load<KIND>(b + 5 * (size_t)min(j, B - 1));
  const BevBox ba = bev_load<KIND>(a + 5 * (size_t)i);
  const float v = bev_pair<KIND>(ba, bb, pts, lane);
  if (j < B) out[(size_t)i * B + j] = v;
}

// ---- greedy NMS ---------------------------------------------------------------------------------------------------
// rank_i = #{j : s_j > s_i, or s_j == s_i and j < i}; a NaN score ranks behind every number (NaNs among themselves by
// index), so that order is a permutation whatever the scores hold.  order[rank] = i; the boxes of the first n ranks go
// to the table with their frames.  flags[workgroup] = a NaN score or a non-finite used box was seen.
__global__ __launch_bounds__(kRankThreads) void nms_rank_kernel(const float *__restrict__ boxes,
                                                                const float *__restrict__ scores,
                                                                int *__restrict__ order, float *__restrict__ table,
                                                                int *__restrict__ flags, int N, int n, int kind) {
  __shared__ float ss[kRankThreads];
  const int tid = threadIdx.x, i = blockIdx.x * kRankThreads + tid;
  const float si = i < N ? scores[i] : 0.f;
  const bool nan_i = si != si;
  int rank = 0;
  for (int base = 0; base < N; base += kRankThreads) {
    __syncthreads();
    if (base + tid < N) ss[tid] = scores[base + tid];
    __syncthreads();
    const int m = min(kRankThreads, N - base);
    for (int t = 0; t < m; ++t) {
      const float sj = ss[t];
      const int j = base + t;
      const bool nan_j = sj != sj;
      const bool before = nan_i ? (!nan_j || j < i) : (sj > si || (sj == si && j < i));
      rank += before ? 1 : 0;
    }
  }
  int bad = 0;
  if (i < N) {
    order[rank] = i;
    bad = nan_i ? 1 : 0;
    if (rank < n) {
      const float *bx = boxes + 5 * (size_t)i;
      const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3], ang = bx[4];
      float c = 1.f, s = 0.f;
      if (kind == PCR_IOU_ROTATED) pcr_bev_frame(ang, c, s);
      if (bev_non_finite(x1) || bev_non_finite(y1) || bev_non_finite(x2) || bev_non_finite(y2) ||
          (kind == PCR_IOU_ROTATED && bev_non_finite(ang)))
        bad = 1;
      float *row = table + 8 * (size_t)rank;
      *reinterpret_cast<float4 *>(row) = make_float4(x1, y1, x2, y2);
      *reinterpret_cast<float4 *>(row + 4) = make_float4(c, s, 0.f, 0.f);
    }
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) flags[blockIdx.x] = bad ? 1 : 0;
}

// One wave per 64 x 64 tile of the ranked boxes, column blocks >= the row block only: lane = column, the row box is
// uniform, and one ballot is one word of the reference's mask (nms_kernel, :284-333; bit c of word (r, cb) <=>
// column 64 cb + c > r and iou(row r, that column) > thresh).  Lane r keeps row r's word and stores it at the end.
template <int KIND>
__global__ __launch_bounds__(kWave) void nms_mask_kernel(const float *__restrict__ table,
                                                         const float *__restrict__ thresh,
                                                         unsigned long long *__restrict__ mask, int n, int nb) {
  __shared__ float pts[KIND == PCR_IOU_AXIS ? 1 : kBevLds];
  const int lane = threadIdx.x, cb = blockIdx.x, rb = blockIdx.y;
  if (cb < rb) return;
  const float thr = thresh[0];
  const int col = cb * kWave + lane;
  const BevBox bc = bev_table(table, min(col, n - 1));
  const int rows = min(kWave, n - rb * kWave);
  unsigned long long mine = 0;
  for (int r = 0; r < rows; ++r) {
    const int row = rb * kWave + r;
    const BevBox br = bev_table(table, row);
    const float v = bev_pair<KIND>(br, bc, pts, lane);
    const unsigned long long bal = __ballot(v > thr && col > row && col < n);
    if (lane == r) mine = bal;
  }
  if (lane < rows) mask[(size_t)(rb * kWave + lane) * nb + cb] = mine;
}

__device__ __forceinline__ unsigned long long lane_read_u64(unsigned long long v, int src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

constexpr int kSweepBlockWords = kWave * kWave;             // one row block of the mask in LDS: 64 rows x 64 words
constexpr int kSweepLdsBytes = 2 * kSweepBlockWords * (int)sizeof(unsigned long long);   // two of them: 64 KiB

// The 64 mask rows of row block rb into registers (lane = word) and the block's order entries (lane = row).  The loads
// are unconditional, from clamped addresses inside the mask, so that they issue back to back; sweep_word drops what
// was not written (words below the row block) or does not exist when the words are used.
__device__ __forceinline__ void sweep_load(const unsigned long long *__restrict__ mask, const int *__restrict__ order,
                                           int rb, int n, int nb, int lane, unsigned long long (&rows)[kWave],
                                           int &ord) {
  const int w = min(lane, nb - 1);
#pragma unroll
  for (int r = 0; r < kWave; ++r) rows[r] = mask[(size_t)min(rb * kWave + r, n - 1) * nb + w];
  ord = order[min(rb * kWave + lane, n - 1)];
}

__device__ __forceinline__ unsigned long long sweep_word(unsigned long long v, int rb, int r, int n, int nb, int lane) {
  return (lane >= rb && lane < nb && rb * kWave + r < n) ? v : 0ull;
}

// The sweep of iou3d.cpp:128-143 by ONE wave: lane w holds remv word w (n <= 4096 = 64 words); the bit of row i is read
// with a lane read, a kept row ORs its words in.  Row blocks of 64 rows pass through two LDS buffers (a lane only ever
// reads back the words it wrote itself, so no barrier is needed): the global loads of block rb + 1 are issued, then the 64
// decisions of block rb run on LDS and registers alone, and only then are the loaded words waited for and parked in the
// other buffer.  The kept rows of a block are collected as bits of one scalar word and stored AFTER its decisions (lane r
// writes at the block's base + the number of kept rows below r), so neither a load nor a store sits in the dependent chain.
__global__ __launch_bounds__(kWave) void nms_sweep_kernel(const unsigned long long *__restrict__ mask,
                                                          const int *__restrict__ order,
                                                          const int *__restrict__ flags, int nflags,
                                                          int *__restrict__ keep, int *__restrict__ count,
                                                          int *__restrict__ info, int N, int n, int nb) {
  extern __shared__ unsigned long long sweep_lds[];
  const int lane = threadIdx.x;
  int bad = 0;
  for (int k = lane; k < nflags; k += kWave) bad |= flags[k];
  if (__ballot(bad != 0)) {
    for (int k = lane; k < N; k += kWave) keep[k] = -1;
    if (lane == 0) count[0] = 0, info[0] = 1;
    return;
  }
  unsigned long long remv = 0;
  int ocur, cnt = 0;
  {
    unsigned long long first[kWave];
    sweep_load(mask, order, 0, n, nb, lane, first, ocur);
#pragma unroll
    for (int r = 0; r < kWave; ++r) sweep_lds[r * kWave + lane] = sweep_word(first[r], 0, r, n, nb, lane);
  }
  for (int rb = 0; rb < nb; ++rb) {
    unsigned long long nxt[kWave];
    int onxt;
    sweep_load(mask, order, min(rb + 1, nb - 1), n, nb, lane, nxt, onxt);
    __builtin_amdgcn_sched_barrier(0);                      // the loads above are in flight; nothing below needs them
    const unsigned long long *cur = sweep_lds + (rb & 1) * kSweepBlockWords + lane;
    const int rows = min(kWave, n - rb * kWave);
    const int owner = __builtin_amdgcn_readfirstlane(rb);
    unsigned long long kept = 0;                            // uniform: bit r = row r of this block is kept
#pragma unroll
    for (int r = 0; r < kWave; ++r) {
      const unsigned long long mine = cur[r * kWave];       // straight-line code: the LDS reads run ahead of the decisions
      const unsigned long long w = lane_read_u64(remv, owner);
      const bool take = r < rows && !((w >> r) & 1ull);     // uniform
      kept |= take ? 1ull << r : 0ull;
      remv |= take ? mine : 0ull;
    }
    __builtin_amdgcn_sched_barrier(0);                      // stores and the wait for block rb + 1 stay behind the chain
    if ((kept >> lane) & 1ull) keep[cnt + __popcll(kept & ((1ull << lane) - 1ull))] = ocur;
    cnt += __popcll(kept);
    if (rb + 1 < nb) {
      unsigned long long *dst = sweep_lds + ((rb + 1) & 1) * kSweepBlockWords + lane;
#pragma unroll
      for (int r = 0; r < kWave; ++r) dst[r * kWave] = sweep_word(nxt[r], rb + 1, r, n, nb, lane);
    }
    ocur = onxt;
  }
  for (int k = cnt + lane; k < N; k += kWave) keep[k] = -1;
  if (lane == 0) count[0] = cnt, info[0] = 0;
}

// ---- the tracker's pairwise rule (virtual_tracker.py:232-259) ---------------------------------------------------------
// A thread owns track k and meets every other track m through LDS tiles; the pair is (i, j) = (min, max).
__global__ __launch_bounds__(kRankThreads) void track_nms_kernel(const float *__restrict__ boxes,
                                                                 const int *__restrict__ classes,
                                                                 const float *__restrict__ scores,
                                                                 const float *__restrict__ thresh,
                                                                 int *__restrict__ suppressed, int N) {
  __shared__ float sb[kRankThreads * 4];
  __shared__ float ss[kRankThreads];
  __shared__ int sc[kRankThreads];
  const int tid = threadIdx.x, k = blockIdx.x * kRankThreads + tid, kc = min(k, N - 1);
  const float thr = thresh[0];
  BevBox own;
  own.x1 = boxes[5 * (size_t)kc], own.y1 = boxes[5 * (size_t)kc + 1], own.x2 = boxes[5 * (size_t)kc + 2];
  own.y2 = boxes[5 * (size_t)kc + 3], own.c = 1.f, own.s = 0.f;
  const float sk = scores[kc];
  const int ck = classes[kc];
  int sup = 0;
  for (int base = 0; base < N; base += kRankThreads) {
    __syncthreads();
    if (base + tid < N) {
      const float *bx = boxes + 5 * (size_t)(base + tid);
      sb[4 * tid] = bx[0], sb[4 * tid + 1] = bx[1], sb[4 * tid + 2] = bx[2], sb[4 * tid + 3] = bx[3];
      ss[tid] = scores[base + tid];
      sc[tid] = classes[base + tid];
    }
    __syncthreads();
    const int cntm = min(kRankThreads, N - base);
    for (int t = 0; t < cntm; ++t) {
      const int m = base + t;
      if (m == k || sc[t] != ck) continue;
      BevBox other;
      other.x1 = sb[4 * t], other.y1 = sb[4 * t + 1], other.x2 = sb[4 * t + 2], other.y2 = sb[4 * t + 3];
      other.c = 1.f, other.s = 0.f;
      if (k < m) {                                          // k is the pair's i
        if (iou_axis(own, other) > thr && sk - ss[t] <= 0) sup = 1;
      } else {                                              // k is the pair's j
        if (iou_axis(other, own) > thr && ss[t] - sk > 0) sup = 1;
      }
    }
  }
  if (k < N) suppressed[k] = sup;
}

constexpr size_t nms_table_bytes(int N) { return (size_t)N * 8 * sizeof(float); }

}  // namespace

PCR_EXPORT int pcr_nearest_bev_f32(const float *boxes7, float *out5, int N, pcr_stream_t stream) {
  if (N < 0) return PCR_ERR_INVALID;
  if (N == 0) return PCR_OK;
  if (!boxes7 || !out5) return PCR_ERR_INVALID;
  return pcr_launch<nearest_bev_kernel>(dim3((N + 255) / 256), dim3(256), 0, pcr_s(stream), boxes7, out5, N);
}

PCR_EXPORT int pcr_bev_frames_f32(const float *boxes5, float *frames, int N, pcr_stream_t stream) {
  if (N < 0) return PCR_ERR_INVALID;
  if (N == 0) return PCR_OK;
  if (!boxes5 || !frames) return PCR_ERR_INVALID;
  return pcr_launch<bev_frames_kernel>(dim3((N + 255) / 256), dim3(256), 0, pcr_s(stream), boxes5, frames, N);
}

PCR_EXPORT int pcr_iou_bev_f32(const float *a, const float *b, float *out, int A, int B, int kind,
                               pcr_stream_t stream) {
  if (A < 0 || A > PCR_IOU_MAX_BOXES || B < 0 || B > PCR_IOU_MAX_BOXES) return PCR_ERR_INVALID;
  if (kind != PCR_IOU_AXIS && kind != PCR_IOU_ROTATED && kind != PCR_IOU_OVERLAP) return PCR_ERR_INVALID;
  if (A == 0 || B == 0) return PCR_OK;
  if (!a || !b || !out) return PCR_ERR_INVALID;
  const dim3 grid((B + kWave - 1) / kWave, A), block(kWave);
  hipStream_t st = pcr_s(stream);
  if (kind == PCR_IOU_AXIS) return pcr_launch<iou_bev_kernel<PCR_IOU_AXIS>>(grid, block, 0, st, a, b, out, A, B);
  if (kind == PCR_IOU_ROTATED) return pcr_launch<iou_bev_kernel<PCR_IOU_ROTATED>>(grid, block, 0, st, a, b, out, A, B);
  return pcr_launch<iou_bev_kernel<PCR_IOU_OVERLAP>>(grid, block, 0, st, a, b, out, A, B);
}

PCR_EXPORT int pcr_nms_ok(int N) { return N >= 0 && N <= PCR_NMS_MAX; }

PCR_EXPORT int pcr_nms_ws_bytes(int N) {
  if (!pcr_nms_ok(N)) return 0;
  const int nb = (N + kWave - 1) / kWave;
  return (int)(nms_table_bytes(N) + kNmsFlags * sizeof(int) + (size_t)N * nb * sizeof(unsigned long long));
}

PCR_EXPORT int pcr_nms_f32(const float *boxes, const float *scores, const float *thresh, int *order, int *keep,
                           int *count, int *info, void *ws, int N, int kind, int pre_max, pcr_stream_t stream) {
  if (!pcr_nms_ok(N)) return PCR_ERR_INVALID;
  if (kind != PCR_IOU_AXIS && kind != PCR_IOU_ROTATED) return PCR_ERR_INVALID;
  if (N == 0) return PCR_OK;
  if (!boxes || !scores || !thresh || !order || !keep || !count || !info || !ws) return PCR_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(ws) & 15) return PCR_ERR_INVALID;
  const int n = pre_max > 0 && pre_max < N ? pre_max : N;     // the ranks that take part
  const int nb = (n + kWave - 1) / kWave, nflags = (N + kRankThreads - 1) / kRankThreads;
  float *table = static_cast<float *>(ws);
  int *flags = reinterpret_cast<int *>(static_cast<char *>(ws) + nms_table_bytes(N));
  unsigned long long *mask = reinterpret_cast<unsigned long long *>(flags + kNmsFlags);
  hipStream_t st = pcr_s(stream);
  int rc = pcr_launch<nms_rank_kernel>(dim3(nflags), dim3(kRankThreads), 0, st, boxes, scores, order, table, flags, N, n,
                                       kind);
  if (rc != PCR_OK) return rc;
  rc = kind == PCR_IOU_AXIS
           ? pcr_launch<nms_mask_kernel<PCR_IOU_AXIS>>(dim3(nb, nb), dim3(kWave), 0, st, (const float *)table, thresh, mask,
                                                       n, nb)
           : pcr_launch<nms_mask_kernel<PCR_IOU_ROTATED>>(dim3(nb, nb), dim3(kWave), 0, st, (const float *)table, thresh,
                                                          mask, n, nb);
  if (rc != PCR_OK) return rc;
  return pcr_launch_lds<nms_sweep_kernel>(dim3(1), dim3(kWave), kSweepLdsBytes, st, (const unsigned long long *)mask, (const int *)order,
                                      (const int *)flags, nflags, keep, count, info, N, n, nb);
}

PCR_EXPORT int pcr_track_nms_f32(const float *boxes5, const int *classes, const float *scores, const float *thresh,
                                 int *suppressed, int N, pcr_stream_t stream) {
  if (!pcr_nms_ok(N)) return PCR_ERR_INVALID;
  if (N == 0) return PCR_OK;
  if (!boxes5 || !classes || !scores || !thresh || !suppressed) return PCR_ERR_INVALID;
  return pcr_launch<track_nms_kernel>(dim3((N + kRankThreads - 1) / kRankThreads), dim3(kRankThreads), 0, pcr_s(stream),
                                      boxes5, classes, scores, thresh, suppressed, N);
}
