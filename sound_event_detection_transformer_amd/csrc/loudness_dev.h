// loudness_dev.h - the device half of the BS.1770 measurement that loudness.hip (every source of a bank) and relevel.hip (every region
// of a job list) share: the K-weighting cascade, the parallel hops, the blocks and the gates.  The helpers were moved out of
// loudness.hip unchanged; loud_measure is the body of its kernel from the rounds to the gated mean, so that both entry points run the
// same operations in the same order and give the same bits on the same samples.  loudness.hip's header holds the definition.
#pragma once
#include "common.h"

#include <math.h>

namespace sedt {

#define SEDT_LOUD_THREADS 256

struct __attribute__((packed, aligned(4))) LoudF4 { float v[4]; };      // four floats behind a pointer that is only 4-byte aligned
typedef __attribute__((ext_vector_type(4))) float loud_f4;

__device__ __forceinline__ loud_f4 loud_load4(const float* p) {
  const LoudF4 u = *reinterpret_cast<const LoudF4*>(p);
  return loud_f4{u.v[0], u.v[1], u.v[2], u.v[3]};
}

struct LoudCoef { double c[10]; };

// one sample through both stages; returns the K-weighted sample
__device__ __forceinline__ double loud_step(const LoudCoef& k, double v, double* s) {
  const double o1 = k.c[0] * v + s[0];
  s[0] = k.c[1] * v - k.c[3] * o1 + s[1];
  s[1] = k.c[2] * v - k.c[4] * o1;
  const double o2 = k.c[5] * o1 + s[2];
  s[2] = k.c[6] * o1 - k.c[8] * o2 + s[3];
  s[3] = k.c[7] * o1 - k.c[9] * o2;
  return o2;
}

// samples p[0 .. len - 1] from state s (updated); returns the sum of y * y in sample order
__device__ __forceinline__ double loud_segment(const LoudCoef& k, const float* __restrict__ p, int len, double* s) {
  double e = 0.0;
  const int nvec = len >> 2;
  if (nvec > 0) {
    loud_f4 cur = loud_load4(p);
    for (int v = 0; v < nvec; ++v) {
      const loud_f4 nxt = v + 1 < nvec ? loud_load4(p + 4 * (v + 1)) : cur;       // (never past the segment)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double y = loud_step(k, (double)cur[i], s);
        e = e + y * y;
      }
      cur = nxt;
    }
  }
  for (int i = 4 * nvec; i < len; ++i) {
    const double y = loud_step(k, (double)p[i], s);
    e = e + y * y;
  }
  return e;
}

struct LoudLds {
  double st[SEDT_LOUD_THREADS][4];      // pass A: the end state of segment t from zero state; after the walk: its true start state
  double carry[4];                      // the state at the start of the next round's first segment
  double sum[SEDT_LOUD_THREADS];
  long cnt[SEDT_LOUD_THREADS];
};

// fixed trees over the workgroup: sum[] and cnt[] hold one value per thread on entry, the totals in [0] on return
__device__ __forceinline__ void loud_tree(LoudLds& lds, int tid) {
  __syncthreads();
  for (int h = SEDT_LOUD_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      lds.sum[tid] = lds.sum[tid] + lds.sum[tid + h];
      lds.cnt[tid] = lds.cnt[tid] + lds.cnt[tid + h];
    }
    __syncthreads();
  }
}

// what loud_measure leaves in every thread of the workgroup
struct LoudResult {
  double zbar;                          // the gated mean of the blocks, 0 when none passes; NaN when a hop energy is not finite
  long J, n_abs, n_rel;                 // blocks; those over the absolute gate; those over both
  bool is_short;
};

// the measurement of p[0 .. len) by one workgroup of SEDT_LOUD_THREADS, all of whose threads call it: the rounds of 256 hops with
// the carried state, the hop energies to e_hop[0 .. len / hop] (the caller has checked that they fit), the blocks and both gates
__device__ __forceinline__ LoudResult loud_measure(LoudLds& lds, const float* __restrict__ p, long len, const double* __restrict__ coef,
                                                   const double* __restrict__ hop_map, int hop, double z_abs, double* __restrict__ e_hop,
                                                   int tid) {
  const long full = len / hop;                                  // full hops
  const long nseg = (len + hop - 1) / hop;                      // segments: the full hops and a trailing partial one (<= full + 1)
  LoudCoef k;
#pragma unroll
  for (int i = 0; i < 10; ++i) k.c[i] = coef[i];
  if (tid < 4) lds.carry[tid] = 0.0;
  bool bad = false;
  // ---- the rounds
  for (long h0 = 0; h0 < nseg; h0 += SEDT_LOUD_THREADS) {
    const long h = h0 + tid;
    const bool active = h < nseg;
    const int n = active ? (int)min((long)hop, len - h * hop) : 0;
    double st[4] = {0.0, 0.0, 0.0, 0.0};
    if (active && h + 1 < nseg) loud_segment(k, p + h * hop, n, st);        // pass A (the source's last segment has no successor)
#pragma unroll
    for (int i = 0; i < 4; ++i) lds.st[tid][i] = st[i];
    __syncthreads();
    if (tid == 0) {                                             // end states from zero -> true start states, in segment order
      double m[16], c[4];
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] = hop_map[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = lds.carry[i];
      const int live = (int)min((long)SEDT_LOUD_THREADS, nseg - h0);
      for (int t = 0; t < live; ++t) {
        double z[4], nx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          z[i] = lds.st[t][i];
          lds.st[t][i] = c[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) nx[i] = (((m[4 * i] * c[0] + m[4 * i + 1] * c[1]) + m[4 * i + 2] * c[2]) + m[4 * i + 3] * c[3]) + z[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = nx[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) lds.carry[i] = c[i];
    }
    __syncthreads();
    if (active) {                                               // pass B
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = lds.st[tid][i];
      const double e = loud_segment(k, p + h * hop, n, st);
      e_hop[h] = e;
      bad = bad || !(fabs(e) <= 1.7976931348623157e308);
    }
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);           // (also: every e_hop of this workgroup is visible to all its threads)
  // ---- blocks and gates
  const bool is_short = len < 4L * hop;
  const long J = is_short ? 1 : full - 3;
  auto z_of = [&](long j) -> double {
    if (is_short) {
      double a = 0.0;
      for (long h = 0; h < nseg; ++h) a = a + e_hop[h];
      return len > 0 ? a / (double)len : 0.0;
    }
    return (((e_hop[j] + e_hop[j + 1]) + e_hop[j + 2]) + e_hop[j + 3]) / (double)(4L * hop);
  };
  double a = 0.0;
  long c = 0;
  for (long j = tid; j < J; j += SEDT_LOUD_THREADS) {
    const double z = z_of(j);
    if (z > z_abs) {
      a = a + z;
      ++c;
    }
  }
  lds.sum[tid] = a;
  lds.cnt[tid] = c;
  loud_tree(lds, tid);
  const long n_abs = lds.cnt[0];
  const double thr = n_abs > 0 ? 0.1 * (lds.sum[0] / (double)n_abs) : 0.0;
  __syncthreads();
  a = 0.0;
  c = 0;
  for (long j = tid; j < J; j += SEDT_LOUD_THREADS) {
    const double z = z_of(j);
    if (z > z_abs && z > thr) {
      a = a + z;
      ++c;
    }
  }
  lds.sum[tid] = a;
  lds.cnt[tid] = c;
  loud_tree(lds, tid);
  const long n_rel = lds.cnt[0];
  const double mean = n_rel > 0 ? lds.sum[0] / (double)n_rel : 0.0;
  return LoudResult{any_bad ? __longlong_as_double(0x7ff8000000000000LL) : mean, J, n_abs, n_rel, is_short};
}

}  // namespace sedt
