// The device-resident crop store (include/pcr.h, section A6): subsamplePC over packed crops, and the training pair rule.
//
// Integer work only: a gather copies the stored floats bit for bit, the pair rule walks int32 tables.  Every sample is
// W(seed, stream, key, k) of pcr.h, or the caller's word in its place; tests/store_ref.py restates both launches.
#include "pcr_common.h"

namespace {

constexpr int kGatherWaves = 4;          // clouds per workgroup: one wave each
constexpr int kPairThreads = 64;         // items per workgroup: one thread each
constexpr uint32_t kStreamPairs = 1u, kStreamGather = 2u;

// (the word's prefix h and pick are pcr_common.h's pcr_word_prefix / pcr_pick: W = pcr_mix32(h ^ k))

// One wave per cloud.  The lanes walk the cloud's 3n output floats, so every store of the wave is 64 consecutive words;
// the three lanes of a slot derive the same word and read the three neighbouring floats of the same stored point.
__global__ __launch_bounds__(kGatherWaves *kWave) void store_gather_kernel(
    const float *__restrict__ points, const long long *__restrict__ offsets, int R, const int *__restrict__ rows,
    const int *__restrict__ keys, const uint32_t *__restrict__ rnd, const unsigned long long *__restrict__ seed,
    float *__restrict__ clouds, int *__restrict__ sizes, int *__restrict__ info, int B, int n) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const long long bl = (long long)blockIdx.x * kGatherWaves + wave;
  if (bl >= B) return;
  const int b = (int)bl;
  const int row = rows[b];
  long long off = 0;
  uint32_t len = 0;
  bool bad = row >= R;
  if (!bad && row >= 0) {
    // a row is read only between offsets[0] and offsets[R], whatever the table holds
    const long long o0 = offsets[row], o1 = offsets[row + 1];
    if (o0 < offsets[0] || o1 < o0 || o1 > offsets[R] || o1 - o0 > 0x7fffffffLL) bad = true;
    else off = o0, len = (uint32_t)(o1 - o0);
  }
  if (lane == 0) {
    sizes[b] = (int)len;
    if (bad) atomicOr(info, PCR_STORE_INFO_ROW);
  }
  float *out = clouds + (size_t)b * n * 3;
  const int nf = 3 * n;
  if (len <= 2u) {
    for (int f = lane; f < nf; f += kWave) out[f] = 0.f;
    return;
  }
  const float *src = points + 3 * (size_t)off;
  if (len == (uint32_t)n) {
    for (int f = lane; f < nf; f += kWave) out[f] = src[f];
    return;
  }
  const uint32_t h = pcr_word_prefix(seed ? seed[0] : 0ull, kStreamGather, keys ? (uint32_t)keys[b] : (uint32_t)b);
  const uint32_t *r = rnd ? rnd + (size_t)b * n : nullptr;
  for (int f = lane; f < nf; f += kWave) {
    const int s = f / 3, c = f - 3 * s;
    const uint32_t u = r ? r[s] : pcr_mix32(h ^ (uint32_t)s);
    out[f] = src[3 * (size_t)pcr_pick(u, len) + c];
  }
}

// the k-th draw of an item: the caller's word, or W(seed, 1, key, k)
struct Draws {
  const uint32_t *r;
  uint32_t h, k;
  __device__ __forceinline__ uint32_t next() {
    const uint32_t w = r ? r[k] : pcr_mix32(h ^ k);
    ++k;
    return w;
  }
};

// _class_list_density / _frame_even: from bucket `from` down to 0, then from 0 up, the first bucket of the CSR row `o`
// that holds at least `need` entries; -1 for none
__device__ __forceinline__ int store_walk(const int *__restrict__ o, int from, int need) {
  for (int q = from; q >= 0; --q)
    if (o[q + 1] - o[q] >= need) return q;
  for (int q = 0; q < PCR_STORE_BUCKETS; ++q)
    if (o[q + 1] - o[q] >= need) return q;
  return -1;
}

// TrainPairs.__getitem__, one item per thread
__global__ __launch_bounds__(kPairThreads) void store_train_pairs_kernel(
    pcr_store_tables t, const int *__restrict__ items, const int *__restrict__ keys, const uint32_t *__restrict__ rnd,
    const unsigned long long *__restrict__ seed, int *__restrict__ rows, int *__restrict__ labels, int *__restrict__ ids,
    int *__restrict__ info, int B) {
  const int b = blockIdx.x * kPairThreads + threadIdx.x;
  if (b >= B) return;
  constexpr int NB = PCR_STORE_BUCKETS;
  const int O = t.num_objects, C = t.num_classes;
  int r1 = -1, r2 = -1, l1 = -1, l2 = -1, i1 = -1, i2 = -1, flags = 0;
  const int o = items[b];
  int c = -1, nb = 0, n = 0;
  if (o >= 0 && o < O) {
    c = t.obj_cls[o];
    nb = t.nums_off[o];
    n = t.nums_off[o + 1] - nb;
  }
  if (c < 0 || c >= C || n < 2) {
    flags = PCR_STORE_INFO_ITEM;
  } else {
    Draws d;
    d.r = rnd ? rnd + (size_t)b * PCR_STORE_PAIR_WORDS : nullptr;
    d.h = pcr_word_prefix(seed ? seed[0] : 0ull, kStreamPairs, (uint32_t)keys[b]);
    d.k = 0;
    l1 = c;
    i1 = t.obj_id[o];
    if (d.next() >> 31) {
      const uint32_t ia = pcr_pick(d.next(), (uint32_t)n);
      const uint32_t j = pcr_pick(d.next(), (uint32_t)(n - 1));
      const uint32_t ib = j + (j >= ia ? 1u : 0u);
      r1 = t.nums_rows[nb + ia];
      r2 = t.nums_rows[nb + ib];
      l2 = c;
      i2 = i1;
    } else {
      r1 = t.nums_rows[nb + pcr_pick(d.next(), (uint32_t)n)];
      // the bucket of the r-th observation in bucket order: the host's draw from the object's own distribution
      const int r = (int)pcr_pick(d.next(), (uint32_t)n);
      const int *bo = t.bucket_off + (size_t)o * NB;
      int dens = 0;
      while (dens < NB - 1 && bo[dens + 1] - bo[0] <= r) ++dens;
      const bool use_tp = (d.next() >> 31) != 0;
      const int *po = t.pool_off + ((size_t)(use_tp ? 0 : 1) * C + c) * NB;
      const int db = store_walk(po, dens, 2);
      int other = -1;
      if (db >= 0) {
        const int cb = po[db], cl = po[db + 1] - cb;
        for (int a = 0; a < PCR_STORE_PAIR_ATTEMPTS; ++a) {
          const int cand = t.pool_objs[cb + pcr_pick(d.next(), (uint32_t)cl)];
          if (cand != o) {
            other = cand;
            break;
          }
        }
        if (other < 0) {
          flags |= PCR_STORE_INFO_RETRY;
          for (int q = 0; q < cl && other < 0; ++q)
            if (t.pool_objs[cb + q] != o) other = t.pool_objs[cb + q];
        }
      }
      int fb = -1;
      const int *oo = nullptr;
      if (other >= 0 && other < O) {
        oo = t.bucket_off + (size_t)other * NB;
        fb = store_walk(oo, db, 1);
      }
      if (fb < 0) {
        flags |= PCR_STORE_INFO_ITEM;      // (a table CropStore refuses to build)
        r1 = l1 = i1 = -1;
      } else {
        r2 = t.bucket_rows[oo[fb] + pcr_pick(d.next(), (uint32_t)(oo[fb + 1] - oo[fb]))];
        l2 = use_tp ? c : c + C;
        i2 = t.obj_fp[other] ? -1 : t.obj_id[other];
      }
    }
  }
  rows[2 * (size_t)b] = r1, rows[2 * (size_t)b + 1] = r2;
  labels[2 * (size_t)b] = l1, labels[2 * (size_t)b + 1] = l2;
  ids[2 * (size_t)b] = i1, ids[2 * (size_t)b + 1] = i2;
  if (flags) atomicOr(info, flags);
}

}  // namespace

PCR_EXPORT int pcr_store_gather_f32(const float *points, const long long *offsets, int R, const int *rows, const int *keys,
                                    const int *rand, const long long *seed, float *clouds, int *sizes, int *info, int B,
                                    int n, pcr_stream_t stream) {
  if (R < 0 || B < 0 || n < 1 || n > PCR_STORE_MAX_SAMPLES) return PCR_ERR_INVALID;
  if (B == 0) return PCR_OK;
  if (!points || !offsets || !rows || !clouds || !sizes || !info) return PCR_ERR_INVALID;
  return pcr_launch<store_gather_kernel>(dim3((B + kGatherWaves - 1) / kGatherWaves), dim3(kGatherWaves * kWave), 0,
                                         pcr_s(stream), points, offsets, R, rows, keys,
                                         reinterpret_cast<const uint32_t *>(rand),
                                         reinterpret_cast<const unsigned long long *>(seed), clouds, sizes, info, B, n);
}

PCR_EXPORT int pcr_store_train_pairs_i32(const pcr_store_tables *tables, const int *items, const int *keys, const int *rand,
                                         const long long *seed, int *rows, int *labels, int *ids, int *info, int B,
                                         pcr_stream_t stream) {
  if (!tables || B < 0) return PCR_ERR_INVALID;
  const pcr_store_tables &t = *tables;
  if (t.num_objects < 0 || t.num_classes < 1) return PCR_ERR_INVALID;
  if (B == 0) return PCR_OK;
  if (!t.obj_cls || !t.obj_fp || !t.obj_id || !t.nums_off || !t.nums_rows || !t.bucket_off || !t.bucket_rows ||
      !t.pool_off || !t.pool_objs)
    return PCR_ERR_INVALID;
  if (!items || !keys || !rows || !labels || !ids || !info) return PCR_ERR_INVALID;
  return pcr_launch<store_train_pairs_kernel>(dim3((B + kPairThreads - 1) / kPairThreads), dim3(kPairThreads), 0,
                                              pcr_s(stream), t, items, keys, reinterpret_cast<const uint32_t *>(rand),
                                              reinterpret_cast<const unsigned long long *>(seed), rows, labels, ids, info,
                                              B);
}
