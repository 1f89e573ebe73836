// loudness.hip - ITU-R BS.1770 loudness of the sources of a sound bank, measured on the device
// (utilities/loudness.py; DESIGN.md section 4, "Loudness (BS.1770) on the device"; tests/loudness_ref.py restates it in float64)
//   * loudness_kernel        one workgroup of 256 per source: the K-weighting cascade (two biquads, transposed direct form II, float64)
//                            run in parallel over the 100 ms hops, the hop energies to `work`, then the gated mean of the 400 ms blocks
//   * scale_sources_kernel   x * gain[s] in place over every source (sedt_scale_sources: the second half of a normalisation)
// The reference has no counterpart: its corpora were mixed offline by a generator that normalises to LUFS.
// The cascade, the rounds, the blocks and the gates are the device functions of loudness_dev.h, which relevel.hip shares: what
// follows defines them.
//
// Filter.  Stage k has b0 b1 b2 a1 a2 = coef[5 k .. 5 k + 4] (a0 = 1 dropped); per sample v, from zero state:
//   o = b0 v + s0;  s0 = b1 v - a1 o + s1;  s1 = b2 v - a2 o;  the shelf stage feeds the high-pass stage.  All in float64 on the float32
//   samples widened; products and sums may be contracted into FMAs.
// Hops.  H = hop samples; segment h of a source of n samples is [h H, min((h + 1) H, n)) - only the last can be partial.  The cascade is
//   linear, so its four state words at the start of segment h + 1 are  hop_map . (state at the start of h) + (the state the segment
//   leaves when it is filtered from zero state); hop_map [4][4] row-major is the cascade's state after H zero-input samples from the
//   four unit states (column k from unit state k; states ordered shelf s0 s1, high-pass s0 s1).  A round takes 256 segments, thread t
//   segment 256 r + t: pass A filters it from zero state and leaves the end state in LDS; thread 0 walks the 256 end states into
//   start states (carrying the last into the next round); pass B filters again from the true start state and writes
//   e_h = sum of y * y, in sample order, to work[base + h].  base = the sum over the earlier sources of (len / H + 1): every workgroup
//   sums it for itself (integers, a fixed tree).  A source whose range does not fit into work_len is not measured: zbar NaN, counts -1.
// Blocks and gates, by the workgroup after its last round: n >= 4 H: J = n / H - 3 blocks, z_j = (e_j + e_j+1 + e_j+2 + e_j+3) / (4 H)
//   (a trailing partial hop is not used); n < 4 H ("short", outside the standard): J = 1, z_0 = (e_0 + e_1 + ..) / n over all its samples
//   (0 for n = 0).  Pass 1: sum and count of z_j > z_abs; pass 2: of z_j > z_abs and z_j > 0.1 * (that sum / that count).  Thread t adds
//   blocks t, t + 256, ... in that order, then a fixed LDS tree - no floating-point atomics, two calls give the same bits.
//   zbar = sum / count of pass 2 (0 when none passes); NaN when a hop energy is not finite (a NaN or infinite sample).
// Memory.  A lane walks its own segment, 16 bytes per load (the next vector is requested before the current one is filtered): a
//   64-byte line is fetched for one lane and used up by its next four loads, so the pass relies on the cache, not on LDS tiles - the
//   float64 recurrence (12 multiply-adds per sample, each stage's state a dependent chain), not the loads, sets the time: DESIGN
//   quotes the measurement.
#include "common.h"
#include "loudness_dev.h"

#include <math.h>

namespace sedt {

__device__ __forceinline__ long loud_clamped_len(const int64_t* src_off, const int64_t* src_len, long flat_len, int s, long& off) {
  off = min(max((long)src_off[s], 0L), flat_len);
  return min(max((long)src_len[s], 0L), flat_len - off);
}

__global__ __launch_bounds__(SEDT_LOUD_THREADS) void loudness_kernel(
    const float* __restrict__ flat, long flat_len, const int64_t* __restrict__ src_off, const int64_t* __restrict__ src_len,
    const double* __restrict__ coef, const double* __restrict__ hop_map, int hop, double z_abs, double* __restrict__ work, long work_len,
    double* __restrict__ zbar, int32_t* __restrict__ counts) {
  __shared__ LoudLds lds;
  const int tid = threadIdx.x, s = blockIdx.x;
  long off;
  const long len = loud_clamped_len(src_off, src_len, flat_len, s, off);
  const float* __restrict__ p = flat + off;
  // ---- this source's place in `work`: the earlier sources hold len / hop + 1 doubles each
  {
    long mine = 0;
    for (int q = tid; q < s; q += SEDT_LOUD_THREADS) {
      long o;
      mine += loud_clamped_len(src_off, src_len, flat_len, q, o) / hop + 1;
    }
    lds.sum[tid] = 0.0;
    lds.cnt[tid] = mine;
    loud_tree(lds, tid);
  }
  const long base = lds.cnt[0];
  __syncthreads();                                              // (cnt[0] is read: the trees below reuse it)
  if (base + len / hop + 1 > work_len) {                        // the same for the whole workgroup; nothing of `work` is touched
    if (tid == 0) {
      zbar[s] = __longlong_as_double(0x7ff8000000000000LL);
      for (int i = 0; i < 4; ++i) counts[4 * s + i] = -1;
    }
    return;
  }
  const LoudResult r = loud_measure(lds, p, len, coef, hop_map, hop, z_abs, work + base, tid);    // (loudness_dev.h)
  if (tid == 0) {
    zbar[s] = r.zbar;
    counts[4 * s] = (int32_t)min(r.J, 0x7fffffffL);
    counts[4 * s + 1] = (int32_t)min(r.n_abs, 0x7fffffffL);
    counts[4 * s + 2] = (int32_t)min(r.n_rel, 0x7fffffffL);
    counts[4 * s + 3] = r.is_short ? 1 : 0;
  }
}

#define SEDT_SCALE_MAXY 128             // workgroups per source at most
#define SEDT_SCALE_PER_WG 8192          // samples per workgroup aimed at when the grid is sized

// workgroups (s, 0 .. gridDim.y - 1) share source s: the scalar head up to the first 16-byte boundary and the tail behind the last
// whole vector belong to workgroup 0, the vectors go round the workgroups.  One float32 multiplication per sample.
__global__ __launch_bounds__(SEDT_LOUD_THREADS) void scale_sources_kernel(float* __restrict__ flat, long flat_len,
                                                                          const int64_t* __restrict__ src_off,
                                                                          const int64_t* __restrict__ src_len,
                                                                          const float* __restrict__ gain) {
  const int tid = threadIdx.x, s = blockIdx.x;
  const float g = gain[s];
  if (g == 1.0f) return;                                        // x * 1 is x: nothing to write
  long off;
  const long len = loud_clamped_len(src_off, src_len, flat_len, s, off);
  float* __restrict__ d = flat + off;
  const long head = min((long)((4 - (int)((reinterpret_cast<uintptr_t>(d) >> 2) & 3)) & 3), len);
  const long nvec = (len - head) >> 2;
  const long tail = head + 4 * nvec;
  if (blockIdx.y == 0) {
    if (tid < head) d[tid] = d[tid] * g;
    if (tid < len - tail) d[tail + tid] = d[tail + tid] * g;
  }
  const long stride = (long)gridDim.y * SEDT_LOUD_THREADS;
  for (long v = (long)blockIdx.y * SEDT_LOUD_THREADS + tid; v < nvec; v += stride) {
    loud_f4* q = reinterpret_cast<loud_f4*>(d + head + 4 * v);
    const loud_f4 x = *q;
    *q = loud_f4{x[0] * g, x[1] * g, x[2] * g, x[3] * g};
  }
}

}  // namespace sedt

extern "C" int sedt_loudness(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                             const double* coef, const double* hop_map, int hop, double z_abs, double* work, int64_t work_len,
                             double* zbar, int32_t* counts, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_src >= 1 && flat_len >= 0 && hop >= 1, "loudness: n_src=%d flat_len=%lld hop=%d (1 <= n_src, 0 <= flat_len, 1 <= hop)",
               n_src, (long long)flat_len, hop);
  SEDT_REQUIRE(z_abs >= 0.0, "loudness: z_abs=%g is not a number >= 0", z_abs);
  SEDT_REQUIRE(work_len >= (int64_t)n_src,
               "loudness: work_len=%lld is too small: every source takes src_len / hop + 1 doubles, %d sources at least %d",
               (long long)work_len, n_src, n_src);
  SEDT_REQUIRE(flat && src_off && src_len && coef && hop_map && work && zbar && counts, "loudness: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(src_off) & 7) == 0 && (reinterpret_cast<uintptr_t>(src_len) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(coef) & 7) == 0 && (reinterpret_cast<uintptr_t>(hop_map) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(work) & 7) == 0 && (reinterpret_cast<uintptr_t>(zbar) & 7) == 0,
               "loudness: the waveforms and counts are 4-byte aligned, the tables and every float64 buffer 8-byte aligned");
  hipLaunchKernelGGL(loudness_kernel, dim3((unsigned)n_src), dim3(SEDT_LOUD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), flat,
                     (long)flat_len, src_off, src_len, coef, hop_map, hop, z_abs, work, (long)work_len, zbar, counts);
  return check_launch("loudness");
}

extern "C" int sedt_scale_sources(float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                                  const float* gain, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_src >= 1 && flat_len >= 0, "scale_sources: n_src=%d flat_len=%lld (1 <= n_src, 0 <= flat_len)", n_src,
               (long long)flat_len);
  SEDT_REQUIRE(flat && src_off && src_len && gain, "scale_sources: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 3) == 0 && (reinterpret_cast<uintptr_t>(gain) & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(src_off) & 7) == 0 && (reinterpret_cast<uintptr_t>(src_len) & 7) == 0,
               "scale_sources: the waveforms and gains are 4-byte aligned, the tables 8-byte aligned");
  const int64_t per = (flat_len / n_src + SEDT_SCALE_PER_WG - 1) / SEDT_SCALE_PER_WG;
  const unsigned gy = (unsigned)(per < 1 ? 1 : (per > SEDT_SCALE_MAXY ? SEDT_SCALE_MAXY : per));
  hipLaunchKernelGGL(scale_sources_kernel, dim3((unsigned)n_src, gy), dim3(SEDT_LOUD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     flat, (long)flat_len, src_off, src_len, gain);
  return check_launch("scale_sources");
}
