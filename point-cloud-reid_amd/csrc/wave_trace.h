// The cycle-stamp recorder of the diagnostic builds (-DPCR_SA_TRACE_BUILD): a lane's view of its record in a device buffer,
// and the host routine that appends a launch's records to a text file (tools/trace_*.py read it).
#pragma once
#include <stdio.h>

#include <vector>

#include "pcr_common.h"

// A record is HEAD header words, then RECS rows of MARKS stamps, and the buffer holds CAP records; the kernel names the lane
// that stamps (`on`), its record, and how many rows to let pass first.  In a build without PCR_SA_TRACE_BUILD every member
// is empty, and a kernel starts its recorder as
//   WaveTrace<..> trace;  if constexpr (kTraceBuild) trace.begin(on, buffer, record, skip);
// so that the arguments are not even evaluated there: the kernel's code is what it is without the recorder.  (An unused
// `lane == 0 && ...` is not free: its compares are merged with the kernel's own and move them.)
#ifdef PCR_SA_TRACE_BUILD
constexpr bool kTraceBuild = true;
#else
constexpr bool kTraceBuild = false;
#endif
// SKIPS: begin() may be told to let rows pass (only then is the row counter ever negative and tested for it).
template <int HEAD, int RECS, int MARKS, int CAP, bool SKIPS = false>
struct WaveTrace {
  static constexpr int kHead = HEAD, kStamps = RECS * MARKS, kWords = HEAD + RECS * MARKS, kCap = CAP;
#ifdef PCR_SA_TRACE_BUILD
  unsigned long long *rec = nullptr;
  int it = 0;
  bool on = false;
  __device__ __forceinline__ void begin(bool on_, unsigned long long *buf, size_t record, int skip = 0) {
    rec = buf + record * kWords, it = -skip, on = on_;
  }
  __device__ __forceinline__ bool live() const { return on && (!SKIPS || it >= 0) && it < RECS; }
  __device__ __forceinline__ void mark(int m) const {                 // stamp m of the current row := the shader clock
    if (live()) rec[HEAD + it * MARKS + m] = __builtin_readcyclecounter();
  }
  __device__ __forceinline__ void mark_realtime(int m) const {        // ... := the constant 100 MHz counter
    if (live()) rec[HEAD + it * MARKS + m] = __builtin_amdgcn_s_memrealtime();
  }
  __device__ __forceinline__ unsigned long long *row() const {        // the current row for a callee (wave_trace_stamp), or null
    return live() ? rec + HEAD + it * MARKS : nullptr;
  }
  __device__ __forceinline__ void next() { it++; }
#else
  __device__ __forceinline__ void begin(bool, unsigned long long *, size_t, int = 0) {}
  __device__ __forceinline__ void mark(int) const {}
  __device__ __forceinline__ void mark_realtime(int) const {}
  __device__ __forceinline__ unsigned long long *row() const { return nullptr; }
  __device__ __forceinline__ void next() {}
#endif
};
__device__ __forceinline__ void wave_trace_stamp(unsigned long long *row, int m) {
#ifdef PCR_SA_TRACE_BUILD
  if (row) row[m] = __builtin_readcyclecounter();
#else
  (void)row, (void)m;
#endif
}

// Host, diagnostics only: synchronises and appends the first `nrec` records of the buffer behind `symbol` to `path`:
// "launch <n> " + the caller's header line, then per record "wg <i>[ hwid <w0> xcc <w1>] <stamps ...>".  Launches
// 1 .. PCR_SA_TRACE_SKIP of the process are passed over (they run cold), the eight after them are written.
template <class TR, class... Head>
static void wave_trace_dump(const char *path, const void *symbol, int nrec, const char *head_fmt, Head... head) {
  static int launches = 0;
  static const int skip = pcr_tune_int("PCR_SA_TRACE_SKIP");
  launches++;
  if (launches <= skip || launches > skip + 8) return;   // a few launches are enough
  static std::vector<unsigned long long> host((size_t)TR::kCap * TR::kWords);
  if (hipDeviceSynchronize() != hipSuccess) return;
  if (hipMemcpyFromSymbol(host.data(), symbol, host.size() * sizeof(unsigned long long)) != hipSuccess) return;
  FILE *f = fopen(path, "a");
  if (!f) return;
  fprintf(f, "launch %d ", launches);
  fprintf(f, head_fmt, head...);
  for (int w = 0; w < (nrec < TR::kCap ? nrec : TR::kCap); w++) {
    const unsigned long long *t = host.data() + (size_t)w * TR::kWords;
    fprintf(f, "wg %d", w);
    if constexpr (TR::kHead == 2) fprintf(f, " hwid %llu xcc %llu", t[0], t[1]);
    for (int i = 0; i < TR::kStamps; i++) fprintf(f, " %llu", t[TR::kHead + i]);
    fprintf(f, "\n");
  }
  fclose(f);
}
