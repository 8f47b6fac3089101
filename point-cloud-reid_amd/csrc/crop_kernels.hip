// Points in boxes and per-box object crops of a LiDAR sweep (include/pcr.h, section A2).
//
// Membership restates mmdet3d/ops/roiaware_pool3d/src/points_in_boxes_cuda.cu:24-49 with the widths that file has: the
// z centre and the half extents are double expressions of float values, the rotation is float.  The file is built with
// -ffp-contract=off (pcr_amd/build.py) and keeps every product in a statement of its own, so a point's membership and its
// box-frame coordinates are the same bits in every kernel below and in the CPU restatement (tests/crops_ref.py).
#include "pcr_common.h"

namespace {

constexpr int kCropThreads = 1024;       // one workgroup per box: 16 waves share the sweep
constexpr int kCropScratch = 64;         // LDS words in front of the count table (per-wave scan totals)
constexpr int kPibTile = 256;            // boxes staged per tile by the two membership kernels
constexpr int kPibPoints = 64;           // points staged per workgroup by points_in_boxes_batch

// (cos, sin) of rot = rz + pi/2 -- the ONLY trigonometry of this file; pcr_box_frames_f32 writes what it returns.
__device__ __forceinline__ void pcr_box_frame(float rz, float &cosa, float &sina) {
  const float rot = (float)((double)rz + 1.57079632679489661923);
  cosa = cosf(rot);
  sina = sinf(rot);
}

struct CropBox {
  float cx, cy, cz, cosa, sina;
  double hl, nhl, hw, nhw, hh;           // l/2, -l/2, w/2, -w/2, h/2 as the .cu evaluates them (double)
};

__device__ __forceinline__ CropBox make_box(float cx, float cy, float cz, float cosa, float sina, float w, float l,
                                            float h) {
  CropBox b;
  b.cx = cx, b.cy = cy, b.cz = cz, b.cosa = cosa, b.sina = sina;
  b.hl = (double)l / 2.0, b.nhl = (double)(-l) / 2.0;
  b.hw = (double)w / 2.0, b.nhw = (double)(-w) / 2.0;
  b.hh = (double)h / 2.0;
  return b;
}

// box = [x, y, z, w, l, h, rz]; z is the bottom face unless z_is_centre
__device__ __forceinline__ float box_cz(const float *box, int z_is_centre) {
  return z_is_centre ? box[2] : (float)((double)box[2] + (double)box[5] / 2.0);
}

__device__ __forceinline__ CropBox load_box(const float *box, int z_is_centre) {
  float c, s;
  pcr_box_frame(box[6], c, s);
  return make_box(box[0], box[1], box_cz(box, z_is_centre), c, s, box[3], box[4], box[5]);
}

// both z faces inside, the x / y faces outside; lx, ly: the point in the box frame
__device__ __forceinline__ bool in_box(const CropBox &b, float x, float y, float z, float &lx, float &ly) {
  const float sx = x - b.cx, sy = y - b.cy;
  const float a0 = sx * b.cosa;
  const float a1 = sy * (-b.sina);
  lx = a0 + a1;
  const float b0 = sx * b.sina;
  const float b1 = sy * b.cosa;
  ly = b0 + b1;
  if ((double)fabsf(z - b.cz) > b.hh) return false;
  return ((double)lx > b.nhl) & ((double)lx < b.hl) & ((double)ly > b.nhw) & ((double)ly < b.hw);
}

// the counter-based generator of pcr.h: the word of slot s of box m under seed
__device__ __forceinline__ uint32_t crop_word(unsigned long long seed, uint32_t m, uint32_t s) {
  uint32_t h = pcr_mix32((uint32_t)seed ^ 0x9e3779b9u);
  h = pcr_mix32(h ^ (uint32_t)(seed >> 32));
  h = pcr_mix32(h ^ m);
  return pcr_mix32(h ^ s);
}

__global__ void box_frames_kernel(const float *__restrict__ boxes, float *__restrict__ frames, int T) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= T) return;
  float c, s;
  pcr_box_frame(boxes[7 * (size_t)k + 6], c, s);
  frames[2 * (size_t)k] = c;
  frames[2 * (size_t)k + 1] = s;
}

// (B,P,3), (B,T,7) -> (B,P,T) 0 / 1.  A thread owns one box (registers) and walks the workgroup's 64 points (LDS
// broadcast reads); consecutive threads write consecutive boxes of a point's row.
__global__ __launch_bounds__(kPibTile) void points_in_boxes_batch_kernel(const float *__restrict__ pts,
                                                                         const float *__restrict__ boxes,
                                                                         int *__restrict__ out, int P, int T) {
  __shared__ float sp[kPibPoints * 3];
  const int b = blockIdx.z, p0 = blockIdx.x * kPibPoints, k = blockIdx.y * kPibTile + threadIdx.x;
  const int np = min(kPibPoints, P - p0);
  if ((int)threadIdx.x < np * 3) sp[threadIdx.x] = pts[((size_t)b * P + p0) * 3 + threadIdx.x];
  __syncthreads();
  if (k >= T) return;
  const CropBox bx = load_box(boxes + ((size_t)b * T + k) * 7, 0);
  int *o = out + ((size_t)b * P + p0) * T + k;
  for (int i = 0; i < np; ++i) {
    float lx, ly;
    o[(size_t)i * T] = in_box(bx, sp[3 * i], sp[3 * i + 1], sp[3 * i + 2], lx, ly) ? 1 : 0;
  }
}

// (B,P,3), (B,T,7) -> (B,P): the lowest box index that holds the point, -1 for none.  A thread owns one point; the
// boxes pass through LDS in tiles of 256 (8 floats a box: centre, frame, sizes).
__global__ __launch_bounds__(kPibTile) void points_in_boxes_kernel(const float *__restrict__ pts,
                                                                   const float *__restrict__ boxes,
                                                                   int *__restrict__ out, int P, int T) {
  __shared__ float sb[kPibTile * 8];
  const int b = blockIdx.y, p = blockIdx.x * kPibTile + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  if (p < P) {
    const float *q = pts + ((size_t)b * P + p) * 3;
    x = q[0], y = q[1], z = q[2];
  }
  int found = -1;
  for (int k0 = 0; k0 < T; k0 += kPibTile) {
    const int nb = min(kPibTile, T - k0);
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const float *bp = boxes + ((size_t)b * T + k0 + threadIdx.x) * 7;
      float c, s;
      pcr_box_frame(bp[6], c, s);
      float *d = sb + 8 * threadIdx.x;
      d[0] = bp[0], d[1] = bp[1], d[2] = box_cz(bp, 0), d[3] = c, d[4] = s, d[5] = bp[3], d[6] = bp[4], d[7] = bp[5];
    }
    __syncthreads();
    if (found < 0) {
      for (int k = 0; k < nb; ++k) {
        const float *d = sb + 8 * k;
        const CropBox bx = make_box(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
        float lx, ly;
        if (in_box(bx, x, y, z, lx, ly)) {
          found = k0 + k;
          break;
        }
      }
    }
  }
  if (p < P) out[(size_t)b * P + p] = found;
}

__device__ __forceinline__ bool crop_test(const CropBox &bx, const float *__restrict__ pts, int stride, int P, int p,
                                          int frame, float &ox, float &oy, float &oz) {
  ox = oy = oz = 0.f;
  if (p >= P) return false;
  const float *q = pts + (size_t)p * stride;
  const float x = q[0], y = q[1], z = q[2];
  float lx, ly;
  const bool in = in_box(bx, x, y, z, lx, ly);
  if (frame == PCR_CROP_FRAME_SENSOR) {
    ox = x, oy = y, oz = z;
  } else if (frame == PCR_CROP_FRAME_CENTRED) {
    ox = x - bx.cx, oy = y - bx.cy, oz = z - bx.cz;
  } else {
    ox = lx, oy = ly, oz = z - bx.cz;
  }
  return in;
}

// One workgroup per box.  Pass 1: every wave tests 64-point chunks of the sweep and leaves the chunk's in-box count in
// LDS; the counts are scanned in place (exclusive).  Pass 2: slot s wants the in-box point of rank j; a binary search over
// the scanned counts names its chunk, the wave tests that chunk again and the lane whose rank inside the chunk's ballot
// is j - base hands its coordinates over.  No list, no atomics, nothing that depends on scheduling.
__global__ __launch_bounds__(kCropThreads) void crop_boxes_kernel(const float *__restrict__ pts, int stride,
                                                                  const float *__restrict__ boxes,
                                                                  const uint32_t *__restrict__ rnd,
                                                                  const unsigned long long *__restrict__ seed,
                                                                  float *__restrict__ clouds, int *__restrict__ lengths,
                                                                  int P, int n, int frame, int rule, int z_is_centre) {
  extern __shared__ uint32_t crop_lds[];
  uint32_t *wsum = crop_lds;
  uint32_t *tab = crop_lds + kCropScratch;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  constexpr int nw = kCropThreads / kWave;
  const int nchunks = (P + kWave - 1) / kWave;
  const CropBox bx = load_box(boxes + 7 * (size_t)m, z_is_centre);

  for (int c = wave; c < nchunks; c += nw) {
    float ox, oy, oz;
    const bool in = crop_test(bx, pts, stride, P, c * kWave + lane, frame, ox, oy, oz);
    const unsigned long long bal = __ballot(in);
    if (lane == 0) tab[c] = (uint32_t)__popcll(bal);
  }
  __syncthreads();

  // exclusive scan of tab[0 .. nchunks): a contiguous segment per thread, a wave scan of the segment sums, the 16 wave totals
  const int per = (nchunks + kCropThreads - 1) / kCropThreads;
  const int lo = min(tid * per, nchunks), hi = min(lo + per, nchunks);
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += tab[i];
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += t;
  }
  if (lane == kWave - 1) wsum[wave] = incl;
  __syncthreads();
  uint32_t woff = 0, len = 0;
#pragma unroll
  for (int w = 0; w < nw; ++w) {
    const uint32_t t = wsum[w];
    woff += w < wave ? t : 0u;
    len += t;
  }
  uint32_t run = woff + incl - sum;
  for (int i = lo; i < hi; ++i) {
    const uint32_t t = tab[i];
    tab[i] = run;
    run += t;
  }
  __syncthreads();
  if (tid == 0) lengths[m] = (int)len;

  float *out = clouds + (size_t)m * n * 3;
  int mode;                                 // 0 zeros, 1 drawn, 2 the in-box points in order
  if (rule == PCR_CROP_RULE_DATASET) mode = len <= 2u ? 0 : (len == (uint32_t)n ? 2 : 1);
  else mode = len == 0u ? 0 : 1;
  if (mode == 0) {
    for (int i = tid; i < 3 * n; i += kCropThreads) out[i] = 0.f;
    return;
  }
  const unsigned long long sd = seed ? seed[0] : 0ull;
  const int SL = min(kWave, max(1, (n + nw - 1) / nw));      // slots a wave takes per round
  for (int base = wave * SL; base < n; base += nw * SL) {
    const int cnt = min(SL, n - base);
    const int s = base + lane;
    const bool own = lane < cnt;
    uint32_t j = 0;
    if (own) {
      if (mode == 2) j = (uint32_t)s;
      else {
        const uint32_t u = rnd ? rnd[(size_t)m * n + s] : crop_word(sd, (uint32_t)m, (uint32_t)s);
        j = (uint32_t)(((unsigned long long)u * len) >> 32);
      }
    }
    int clo = 0, chi = nchunks - 1;         // the largest chunk whose scanned count is <= j (its own count is > 0 then)
    while (clo < chi) {
      const int mid = (clo + chi + 1) >> 1;
      if (tab[mid] <= j) clo = mid;
      else chi = mid - 1;
    }
    const uint32_t r = j - tab[clo];
    float mx = 0.f, my = 0.f, mz = 0.f;
    for (int i = 0; i < cnt; ++i) {
      const int ci = __shfl(clo, i, kWave);
      const uint32_t ri = __shfl(r, i, kWave);
      float ox, oy, oz;
      const bool in = crop_test(bx, pts, stride, P, ci * kWave + lane, frame, ox, oy, oz);
      const unsigned long long bal = __ballot(in);
      const uint32_t rank = pcr_lanes_below(bal);
      const unsigned long long hit = __ballot(in && rank == ri);
      const int src = hit ? __ffsll((long long)hit) - 1 : 0;
      const float vx = __shfl(ox, src, kWave), vy = __shfl(oy, src, kWave), vz = __shfl(oz, src, kWave);
      if (lane == i) mx = vx, my = vy, mz = vz;
    }
    if (own) {
      float *o = out + 3 * (size_t)s;
      o[0] = mx, o[1] = my, o[2] = mz;
    }
  }
}

size_t crop_lds_bytes(int P) { return ((size_t)((P + kWave - 1) / kWave) + kCropScratch) * sizeof(uint32_t); }

static_assert(((PCR_CROP_MAX_POINTS + kWave - 1) / kWave + kCropScratch) * sizeof(uint32_t) == (size_t)kMaxDynLds,
              "PCR_CROP_MAX_POINTS is what the count table leaves of the LDS");

}  // namespace

PCR_EXPORT int pcr_box_frames_f32(const float *boxes, float *frames, int T, pcr_stream_t stream) {
  if (T < 0) return PCR_ERR_INVALID;
  if (T == 0) return PCR_OK;
  if (!boxes || !frames) return PCR_ERR_INVALID;
  return pcr_launch<box_frames_kernel>(dim3((T + 255) / 256), dim3(256), 0, pcr_s(stream), boxes, frames, T);
}

PCR_EXPORT int pcr_points_in_boxes_batch_f32(const float *points, const float *boxes, int *out, int B, int P, int T,
                                             pcr_stream_t stream) {
  if (B < 0 || P < 0 || T < 0 || B > 65535) return PCR_ERR_INVALID;
  if (B == 0 || P == 0 || T == 0) return PCR_OK;
  if (!points || !boxes || !out) return PCR_ERR_INVALID;
  const int gy = (T + kPibTile - 1) / kPibTile;
  if (gy > 65535) return PCR_ERR_INVALID;
  return pcr_launch<points_in_boxes_batch_kernel>(dim3((P + kPibPoints - 1) / kPibPoints, gy, B), dim3(kPibTile), 0,
                                                  pcr_s(stream), points, boxes, out, P, T);
}

PCR_EXPORT int pcr_points_in_boxes_f32(const float *points, const float *boxes, int *out, int B, int P, int T,
                                       pcr_stream_t stream) {
  if (B < 0 || P < 0 || T < 0 || B > 65535) return PCR_ERR_INVALID;
  if (B == 0 || P == 0) return PCR_OK;
  if (!points || !out || (T > 0 && !boxes)) return PCR_ERR_INVALID;
  return pcr_launch<points_in_boxes_kernel>(dim3((P + kPibTile - 1) / kPibTile, B), dim3(kPibTile), 0, pcr_s(stream),
                                            points, boxes, out, P, T);
}

PCR_EXPORT int pcr_crop_boxes_ok(int P, int M, int n, int stride) {
  // P: the scanned count table (one word per 64 points) and its scratch words must fit the 160 KiB of LDS a workgroup
  // may take on gfx950
  if (P < 0 || P > PCR_CROP_MAX_POINTS) return 0;
  if (M < 0 || M > PCR_CROP_MAX_BOXES) return 0;
  if (n < 1 || n > PCR_CROP_MAX_SAMPLES) return 0;
  if (stride < 3 || stride > PCR_CROP_MAX_STRIDE) return 0;
  return 1;
}

PCR_EXPORT int pcr_crop_boxes_f32(const float *points, int stride, const float *boxes, const int *rand,
                                  const long long *seed, float *clouds, int *lengths, int P, int M, int n, int frame,
                                  int rule, int z_is_centre, pcr_stream_t stream) {
  if (!pcr_crop_boxes_ok(P, M, n, stride)) return PCR_ERR_INVALID;
  if (frame < PCR_CROP_FRAME_SENSOR || frame > PCR_CROP_FRAME_BOX) return PCR_ERR_INVALID;
  if (rule != PCR_CROP_RULE_TRACKER && rule != PCR_CROP_RULE_DATASET) return PCR_ERR_INVALID;
  if (M == 0) return PCR_OK;
  if (!boxes || !clouds || !lengths || (P > 0 && !points)) return PCR_ERR_INVALID;
  return pcr_launch_lds<crop_boxes_kernel>(dim3(M), dim3(kCropThreads), crop_lds_bytes(P), pcr_s(stream), points, stride,
                                           boxes, reinterpret_cast<const uint32_t *>(rand),
                                           reinterpret_cast<const unsigned long long *>(seed), clouds, lengths, P, n,
                                           frame, rule, z_is_centre != 0);
}
