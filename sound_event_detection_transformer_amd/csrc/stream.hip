// stream.hip - live streams: every one of S streams owns a ring of ring_samples float32 in one [S, ring_samples] device tensor
//   * stream_append_kernel   chunks that arrived, staged as one flat float32 vector, into the streams' rings (wrapping)
//   * stream_cut_kernel      the windows that became due out of the rings into the detector's (B, window) input, zero-padded
// The reference reads whole files and has no counterpart; DESIGN.md section 4 ("Live streams") holds the definition.
// One launch serves all streams; the jobs are small int32 tables the host uploads (four words a job).
// Access width: window starts and write positions are arbitrary sample indices, so a row is only 4-byte aligned relative to the
// ring and the two sides of a copy rarely agree on anything wider.  Both kernels therefore move DWORDS, one per lane and step
// (a wave's 64 consecutive dwords coalesce into full cache lines on either side); no 16-byte path, plain vector loads and stores
// only.  The volume is small beside the step it feeds: a window of 10 s at 16 kHz is 640 KB.
// The entry points check every job on the host copy of the table; the kernels check again and skip a job that is out of range, so
// nothing is read or written out of bounds whatever the device table holds.
#include <vector>

#include "common.h"

namespace sedt {

#define SEDT_RING_THREADS 256
#define SEDT_RING_MAX_BLOCKS 64    // blocks per job / row: a grid-stride loop covers the rest
enum { SEDT_APPEND_STREAM, SEDT_APPEND_POS, SEDT_APPEND_SRC, SEDT_APPEND_N, SEDT_RING_JOB_WORDS };
enum { SEDT_CUT_STREAM, SEDT_CUT_POS, SEDT_CUT_LEN, SEDT_CUT_ROW };

// blockIdx.y = job {stream, ring write position, source offset, n}
__global__ __launch_bounds__(SEDT_RING_THREADS) void stream_append_kernel(const float* __restrict__ src, long src_len,
                                                                          const int32_t* __restrict__ jobs, float* __restrict__ ring,
                                                                          int S, int ring_samples) {
  const int32_t* job = jobs + (long)blockIdx.y * SEDT_RING_JOB_WORDS;
  const int s = job[SEDT_APPEND_STREAM], pos = job[SEDT_APPEND_POS], off = job[SEDT_APPEND_SRC], n = job[SEDT_APPEND_N];
  if (s < 0 || s >= S || pos < 0 || pos >= ring_samples || n < 0 || n > ring_samples || off < 0 || (long)off + n > src_len) return;
  float* dst = ring + (long)s * ring_samples;
  for (int i = blockIdx.x * SEDT_RING_THREADS + threadIdx.x; i < n; i += gridDim.x * SEDT_RING_THREADS) {
    int p = pos + i;                                                    // pos < ring and i < n <= ring: one subtraction wraps
    if (p >= ring_samples) p -= ring_samples;
    dst[p] = src[(long)off + i];
  }
}

// blockIdx.y = row of wave [B, window]; its job {stream, ring read position, length, row} is looked up in the table (at most B jobs)
__global__ __launch_bounds__(SEDT_RING_THREADS) void stream_cut_kernel(const float* __restrict__ ring, int S, int ring_samples,
                                                                       const int32_t* __restrict__ jobs, int n_jobs,
                                                                       float* __restrict__ wave, int window) {
  const int b = blockIdx.y;
  int s = -1, pos = 0, len = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const int32_t* job = jobs + (long)j * SEDT_RING_JOB_WORDS;
    if (job[SEDT_CUT_ROW] == b) {
      s = job[SEDT_CUT_STREAM]; pos = job[SEDT_CUT_POS]; len = job[SEDT_CUT_LEN];
      break;
    }
  }
  if (s < 0 || s >= S || pos < 0 || pos >= ring_samples || len < 0 || len > window || len > ring_samples) len = 0, s = 0, pos = 0;
  const float* from = ring + (long)s * ring_samples;
  float* dst = wave + (long)b * window;
  for (int i = blockIdx.x * SEDT_RING_THREADS + threadIdx.x; i < window; i += gridDim.x * SEDT_RING_THREADS) {
    float v = 0.f;                                                      // past the length, and a row without a job: zeros
    if (i < len) {
      int p = pos + i;
      if (p >= ring_samples) p -= ring_samples;
      v = from[p];
    }
    dst[i] = v;
  }
}

static inline unsigned ring_blocks(long n) {
  const long b = (n + SEDT_RING_THREADS - 1) / SEDT_RING_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > SEDT_RING_MAX_BLOCKS ? SEDT_RING_MAX_BLOCKS : b));
}

}  // namespace sedt

extern "C" int sedt_stream_append(const float* src, int64_t src_len, const int32_t* jobs_host, const int32_t* jobs, int n_jobs, float* ring,
                                  int S, int ring_samples, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(S >= 1 && ring_samples >= 1 && n_jobs >= 0 && n_jobs <= 65535 && src_len >= 0,
               "stream_append: S=%d ring_samples=%d n_jobs=%d (0 .. 65535) src_len=%lld", S, ring_samples, n_jobs, (long long)src_len);
  if (n_jobs == 0) return 0;
  SEDT_REQUIRE(src && jobs_host && jobs && ring, "stream_append: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(ring) & 3) == 0,
               "stream_append: the samples are 4-byte aligned");
  int most = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const int32_t* job = jobs_host + (long)j * SEDT_RING_JOB_WORDS;
    const int s = job[SEDT_APPEND_STREAM], pos = job[SEDT_APPEND_POS], off = job[SEDT_APPEND_SRC], n = job[SEDT_APPEND_N];
    SEDT_REQUIRE(s >= 0 && s < S, "stream_append: job %d: stream %d outside 0 .. %d", j, s, S - 1);
    SEDT_REQUIRE(pos >= 0 && pos < ring_samples, "stream_append: job %d: write position %d outside the ring of %d samples", j, pos,
                 ring_samples);
    SEDT_REQUIRE(n >= 0 && n <= ring_samples, "stream_append: job %d: %d samples, the ring holds %d", j, n, ring_samples);
    SEDT_REQUIRE(off >= 0 && (int64_t)off + n <= src_len, "stream_append: job %d: samples %d .. %lld outside the staged %lld", j, off,
                 (long long)off + n, (long long)src_len);
    most = n > most ? n : most;
  }
  hipLaunchKernelGGL(stream_append_kernel, dim3(ring_blocks(most), n_jobs), dim3(SEDT_RING_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), src, (long)src_len, jobs, ring, S, ring_samples);
  return check_launch("stream_append");
}

extern "C" int sedt_stream_cut(const float* ring, int S, int ring_samples, const int32_t* jobs_host, const int32_t* jobs, int n_jobs,
                               float* wave, int B, int window, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(S >= 1 && B >= 1 && B <= 65535 && n_jobs >= 0 && n_jobs <= B, "stream_cut: S=%d B=%d (1 .. 65535) n_jobs=%d (0 .. B)", S, B,
               n_jobs);
  SEDT_REQUIRE(window >= 1 && window <= ring_samples, "stream_cut: window=%d ring_samples=%d (1 <= window <= ring_samples)", window,
               ring_samples);
  SEDT_REQUIRE(ring && wave && (n_jobs == 0 || (jobs_host && jobs)), "stream_cut: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(wave) & 3) == 0 && (reinterpret_cast<uintptr_t>(ring) & 3) == 0,
               "stream_cut: the samples are 4-byte aligned");
  std::vector<char> taken(B, 0);
  for (int j = 0; j < n_jobs; ++j) {
    const int32_t* job = jobs_host + (long)j * SEDT_RING_JOB_WORDS;
    const int s = job[SEDT_CUT_STREAM], pos = job[SEDT_CUT_POS], len = job[SEDT_CUT_LEN], row = job[SEDT_CUT_ROW];
    SEDT_REQUIRE(s >= 0 && s < S, "stream_cut: job %d: stream %d outside 0 .. %d", j, s, S - 1);
    SEDT_REQUIRE(pos >= 0 && pos < ring_samples, "stream_cut: job %d: read position %d outside the ring of %d samples", j, pos, ring_samples);
    SEDT_REQUIRE(len >= 0 && len <= window, "stream_cut: job %d: length %d outside 0 .. window %d", j, len, window);
    SEDT_REQUIRE(row >= 0 && row < B, "stream_cut: job %d: row %d outside 0 .. %d", j, row, B - 1);
    SEDT_REQUIRE(!taken[row], "stream_cut: job %d: row %d has a job already", j, row);
    taken[row] = 1;
  }
  hipLaunchKernelGGL(stream_cut_kernel, dim3(ring_blocks(window), B), dim3(SEDT_RING_THREADS), 0, reinterpret_cast<hipStream_t>(stream), ring,
                     S, ring_samples, jobs, n_jobs, wave, window);
  return check_launch("stream_cut");
}
