// recpsds.hip - the PSDS confusion counts of recordings of any length: the stitched event lists of stitch_events_kernel (stitch.hip)
// against the recordings' annotations, per (threshold, recording, class) - lists in, counts out
//   * recording_psds_counts_kernel   counts [K][C][C + 1] += {true positives on the diagonal, cross triggers, the world column}
//                                    one wave per (recording, class, threshold)
// The reference scores 10 s dataset clips only and has no counterpart; the counts are those of psds.hip (utilities/psds.py holds the
// definition) with "clip" read as "recording" and "record order" read as "onset order", without a limit on the events of a list.
// DESIGN.md section 4 ("PSDS on recordings") holds the definition and tests/recording_psds_ref.py restates it in NumPy.
//
// Scope: per fusion strategy, threshold k, recording r with rec_idx[r] inside the table.  Float64, plain subtract / divide / compare,
// no contraction, comparisons >=; inter(d, g) = min(off_d, off_g) - max(on_d, on_g) counts only where it is > 0; every term is one
// division added to a running sum.
//   detections  of class c: the first min(count, cap) slots of out[k][r][c], as stitch wrote them: ascending by onset and disjoint.  One
//               whose off - on is not > 0 takes part in nothing.
//   references  of class c': the table's list of (rec_idx[r], c'), ascending by onset, any number of them, and they may overlap.  One
//               whose end - on is not > 0 takes part in nothing.
//   DTC         p_d = sum of inter(d, g) / dur_d over the references g of d's class, in table order; d passes when p_d >= dtc.
//   GTC         v_g = sum of inter(d, g) / dur_g over the detections of g's class that passed, in onset order; v_g >= gtc:
//               counts[c][c] += 1.
//   CTTC        for every d that failed the DTC and every other class c': sum of inter(d, g) / dur_d over the references of c' >= cttc:
//               counts[class(d)][c'] += 1; independently (min(off_d, rec_dur[r]) - max(on_d, 0)) / dur_d >= cttc: counts[class(d)][C]
//               += 1, the world column.
//   no limit    a term with inter <= 0 adds nothing, so only the items that can overlap are walked, in the stated order:
//               - the references that overlap a detection: all of them have on_g < off_d, and none before the first j whose PREFIX
//                 MAXIMUM of `end` (ref_pmax, the host's running maximum over the list) is > on_d can reach d.  Binary search for that
//                 j, then scan while ref_on[j] < off_d.  A reference spanning the recording makes every scan of its class start
//                 at it: that costs time, not correctness.
//               - the detections that overlap a reference: they are disjoint, so max(on_d, off_d) ascends with the onset; binary
//                 search for the first d with max(on_d, off_d) > on_g, then scan while on_d < off_g.
//   pass bits   phase 1 (lane = detection, chunks of 64) leaves one ballot word per chunk in pass [K][R][C][ceil(cap / 64)]; phase 2
//               (lane = reference, chunks of 64) reads them back.  The wave that writes a word is the only one that reads it.
//   status      [K][R] int32, zeroed before the launch: 1 the stitch status of (k, r) is non-zero or some count[k][r][c] > cap; 4 a list
//               holds a non-finite time, is not ascending by onset, or estimates overlap (an onset before the previous offset).  1
//               before 4.  With a status raised the counters may hold partial sums of that recording.
// count is clamped to 0 .. cap before it indexes anything, a rec_idx outside the table is skipped, the CSR offsets are clamped to the
// table and every scan ends at its list's end: nothing is read or written out of bounds, whatever the lists hold.  Counters are
// int64, integer atomics only: results do not depend on launch order.
#include <cmath>

#include "common.h"
#include "recording_lists.h"

#pragma clang fp contract(off)     // inter / dur added to a running sum: the plain float64 operations of the definition

namespace sedt {

// sum over the references j0 .. j1 (table order) of inter(d, g) / dur, d = (on, off), dur = off - on > 0
__device__ __forceinline__ double rp_reference_sum(const double* __restrict__ ref_on, const double* __restrict__ ref_end,
                                                   const double* __restrict__ ref_pmax, int j0, int j1, double on, double off, double dur) {
  int lo = j0, hi = j1;                                               // the first j whose prefix maximum of `end` is > on
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ref_pmax[mid] > on) hi = mid; else lo = mid + 1;
  }
  double sum = 0.0;
  for (int j = lo; j < j1; ++j) {
    const double g_on = ref_on[j];
    if (!(g_on < off)) break;                                         // ascending by onset: nothing behind it overlaps d
    const double g_end = ref_end[j];
    if (!(g_end - g_on > 0.0)) continue;                              // a zero-length reference takes part in nothing
    const double inter = fmin(off, g_end) - fmax(on, g_on);
    if (inter > 0.0) sum = sum + inter / dur;
  }
  return sum;
}

// block = 64 threads = one wave, blockIdx.x = recording * C + class, blockIdx.y = threshold; counts: this fusion strategy's
// [K][C][C + 1]; pass [K][R][C][n_pass] with n_pass = ceil(cap / 64); status [K][R] zeroed before the launch
__global__ __launch_bounds__(64) void recording_psds_counts_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ out,
                                                                   const int32_t* __restrict__ stitch_status,
                                                                   const int32_t* __restrict__ rec_idx, const int32_t* __restrict__ ref_off,
                                                                   const double* __restrict__ ref_on, const double* __restrict__ ref_end,
                                                                   const double* __restrict__ ref_pmax, const double* __restrict__ rec_dur,
                                                                   int N, int E, int R, int C, int cap, int n_pass, double dtc, double gtc,
                                                                   double cttc, unsigned long long* pass,
                                                                   unsigned long long* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ unsigned int col[64];                                    // this wave's additions to row c of counts: C + 1 <= 64 columns
  const int r = blockIdx.x / C, c = blockIdx.x % C, kt = blockIdx.y, lane = threadIdx.x;
  const int ri = rec_idx[r];
  if (ri < 0 || ri >= N) return;                                      // not in the reference: adds nothing anywhere
  const long kr = (long)kt * R + r;
  const int32_t* cnt = count + kr * C;
  if (rm_incomplete(stitch_status, cnt, kr, C, cap, lane)) {
    if (lane == 0 && c == 0) atomicMax(&status[kr], SEDT_RM_INCOMPLETE);   // every class of (k, r) sees it and counts nothing
    return;
  }
  const int n_det = min(max(cnt[c], 0), cap);
  const double* det = reinterpret_cast<const double*>(out + (kr * C + c) * (long)cap * SEDT_EVENT_WORDS);
  int j0, j1;
  rm_ref_range(ref_off, ri, C, c, E, j0, j1);
  if (!rm_lists_ok(det, n_det, ref_on, ref_end, j0, j1, lane, true)) {
    if (lane == 0) atomicMax(&status[kr], SEDT_RM_UNORDERED);
    return;
  }
  col[lane] = 0u;
  __syncthreads();
  const double D = rec_dur[r];
  unsigned long long* my_pass = pass + (kr * C + c) * (long)n_pass;

  // ---- phase 1: lane = detection.  DTC; on failure the CTTC sums over the other classes' lists and the world term
  for (int base = 0; base < n_det; base += 64) {
    const int i = base + lane;
    double on = 0.0, off = 0.0;
    if (i < n_det) {
      on = det[SEDT_EVENT_DOUBLES * (long)i];
      off = det[SEDT_EVENT_DOUBLES * (long)i + 1];
    }
    const double dur = off - on;
    const bool live = i < n_det && dur > 0.0;                         // a zero-length detection takes part in nothing
    const bool passed = live && rp_reference_sum(ref_on, ref_end, ref_pmax, j0, j1, on, off, dur) >= dtc;
    const unsigned long long word = __ballot(passed);
    if (lane == 0) __hip_atomic_store(my_pass + (base >> 6), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool failed = live && !passed;
    if (__ballot(failed) == 0ull) continue;
    for (int o = 0; o < C; ++o) {                                     // wave-uniform: the list of class o is the same for every lane
      if (o == c) continue;
      int o0, o1;
      rm_ref_range(ref_off, ri, C, o, E, o0, o1);
      if (o0 == o1) continue;
      if (failed && rp_reference_sum(ref_on, ref_end, ref_pmax, o0, o1, on, off, dur) >= cttc) atomicAdd(&col[o], 1u);
    }
    if (failed && (fmin(off, D) - fmax(on, 0.0)) / dur >= cttc) atomicAdd(&col[C], 1u);
  }
  // the words above were stored by lane 0 and are read by every lane: stores drained and ordered before the loads below
  __threadfence();
  __syncthreads();

  // ---- phase 2: lane = reference.  GTC over the detections that passed, in onset order
  unsigned int tp = 0u;                                               // wave-uniform
  for (int base = j0; base < j1; base += 64) {
    const int j = base + lane;
    bool hit = false;
    if (j < j1) {
      const double g_on = ref_on[j], g_end = ref_end[j], g_dur = g_end - g_on;
      if (g_dur > 0.0) {
        int lo = 0, hi = n_det;                                       // the first d with max(on_d, off_d) > on_g
        while (lo < hi) {
          const int mid = lo + ((hi - lo) >> 1);
          if (fmax(det[SEDT_EVENT_DOUBLES * (long)mid], det[SEDT_EVENT_DOUBLES * (long)mid + 1]) > g_on) hi = mid; else lo = mid + 1;
        }
        double v = 0.0;
        for (int i = lo; i < n_det; ++i) {
          const double on = det[SEDT_EVENT_DOUBLES * (long)i];
          if (!(on < g_end)) break;                                   // ascending by onset: nothing behind it overlaps g
          const unsigned long long word = __hip_atomic_load(my_pass + (i >> 6), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (!((word >> (i & 63)) & 1ull)) continue;
          const double inter = fmin(det[SEDT_EVENT_DOUBLES * (long)i + 1], g_end) - fmax(on, g_on);
          if (inter > 0.0) v = v + inter / g_dur;
        }
        hit = v >= gtc;
      }
    }
    tp += (unsigned int)__popcll(__ballot(hit));
  }
  if (lane == 0) col[c] = tp;                                         // column c is the diagonal: no cross trigger lands on it
  __syncthreads();
  if (lane <= C && col[lane]) atomicAdd(counts + ((long)kt * C + c) * (C + 1) + lane, (unsigned long long)col[lane]);
}

}  // namespace sedt

extern "C" int sedt_recording_psds_counts(const int32_t* count, const int32_t* out, const int32_t* stitch_status, const int32_t* rec_idx,
                                          const int32_t* ref_off, const double* ref_on, const double* ref_end, const double* ref_pmax,
                                          const double* rec_dur, int n_ref_rec, int n_ref_events, int K, int R, int C, int cap,
                                          int n_fusion, int fusion, double dtc, double gtc, double cttc, uint64_t* pass, int64_t* counts,
                                          int32_t* status, void* stream) {
  using namespace sedt;
  if (recording_args_ok("recording_psds_counts", count, out, stitch_status, rec_idx, ref_off, ref_on, ref_end, n_ref_rec, n_ref_events, K,
                        R, C, cap, n_fusion, fusion, status))
    return 1;
  SEDT_REQUIRE(dtc == dtc && gtc == gtc && cttc == cttc, "recording_psds_counts: a tolerance criterion is NaN (dtc %g gtc %g cttc %g)", dtc,
               gtc, cttc);
  if (R == 0) return 0;
  SEDT_REQUIRE(rec_dur && pass && counts, "recording_psds_counts: null pointer");
  SEDT_REQUIRE(n_ref_events == 0 || ref_pmax, "recording_psds_counts: the prefix maximum of the reference ends is missing");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(pass) & 7) == 0, "recording_psds_counts: pass is not 8-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)K * R, s) != hipSuccess) return check_launch("recording_psds_counts (status)");
  const int n_pass = (int)(((long)cap + 63) / 64);
  hipLaunchKernelGGL(recording_psds_counts_kernel, dim3((unsigned)(R * C), K), dim3(64), 0, s, count, out, stitch_status, rec_idx, ref_off,
                     ref_on, ref_end, ref_pmax, rec_dur, n_ref_rec, n_ref_events, R, C, cap, n_pass, dtc, gtc, cttc,
                     reinterpret_cast<unsigned long long*>(pass),
                     reinterpret_cast<unsigned long long*>(counts) + (long)fusion * K * C * (C + 1), status);
  return check_launch("recording_psds_counts");
}
