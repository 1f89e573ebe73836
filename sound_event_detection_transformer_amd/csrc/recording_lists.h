// recording_lists.h - what the kernels that read stitched event lists against a recording's annotations share (recmetrics.hip,
// recpsds.hip): the status values, the completeness test of (threshold, recording), the clamped CSR range of (recording, class), the
// check of the premise "finite and ascending by onset", and the host-side argument checks.
#pragma once
#include <cmath>

#include "common.h"
#include "event_records.h"

namespace sedt {

#define SEDT_RM_INCOMPLETE 1
#define SEDT_RM_BLOCK 2
#define SEDT_RM_UNORDERED 4

__device__ __forceinline__ bool rm_finite(double x) { return fabs(x) < INFINITY; }      // false for NaN

// lists of (k, r): true when the stitch raised a status or a class holds more events than `out` does (wave-uniform; lane = class)
__device__ __forceinline__ bool rm_incomplete(const int32_t* stitch_status, const int32_t* cnt, long kr, int C, int cap, int lane) {
  const bool over = lane < C && cnt[lane] > cap;
  return stitch_status[kr] != 0 || __ballot(over) != 0ull;
}

// the CSR range of (reference recording ri, class c), clamped to 0 .. E
__device__ __forceinline__ void rm_ref_range(const int32_t* ref_off, int ri, int C, int c, int E, int& j0, int& j1) {
  j0 = min(max(ref_off[(long)ri * C + c], 0), E);
  j1 = min(max(ref_off[(long)ri * C + c + 1], j0), E);
}

// every lane of the wave: true when the n events at `ev` (stitched events read as doubles: onset, offset) / the references j0 .. j1 are finite and
// ascending by onset; with `disjoint` the events may not overlap either (no onset before the previous offset)
__device__ __forceinline__ bool rm_lists_ok(const double* ev, int n, const double* ref_on, const double* ref_end, int j0, int j1, int lane,
                                            bool disjoint = false) {
  bool bad = false;
  for (int i = lane; i < n; i += 64) {
    const double* e = ev + SEDT_EVENT_DOUBLES * (long)i;                    // e[-SEDT_EVENT_DOUBLES ..]: the event before it
    const double on = e[0], off = e[1];
    bad = bad || !rm_finite(on) || !rm_finite(off) || (i > 0 && !(on >= e[-SEDT_EVENT_DOUBLES]));
    if (disjoint) bad = bad || (i > 0 && !(on >= e[1 - SEDT_EVENT_DOUBLES]));
  }
  for (int j = j0 + lane; j < j1; j += 64) {
    const double on = ref_on[j];
    bad = bad || !rm_finite(on) || !rm_finite(ref_end[j]) || (j > j0 && !(on >= ref_on[j - 1]));
  }
  return __ballot(bad) == 0ull;
}

static inline int recording_args_ok(const char* what, const void* count, const void* out, const void* stitch_status, const void* rec_idx,
                                    const void* ref_off, const void* ref_on, const void* ref_end, int n_ref_rec, int n_ref_events, int K,
                                    int R, int C, int cap, int n_fusion, int fusion, const void* status) {
  SEDT_REQUIRE(C >= 1 && C <= SEDT_MAX_CLASSES, "%s: C=%d (1 .. %d)", what, C, SEDT_MAX_CLASSES);
  SEDT_REQUIRE(K >= 1 && K <= SEDT_MAX_THRESHOLDS, "%s: %d thresholds (1 .. %d)", what, K, SEDT_MAX_THRESHOLDS);
  SEDT_REQUIRE(R >= 0 && cap >= 1, "%s: R=%d (>= 0) cap=%d (>= 1)", what, R, cap);
  SEDT_REQUIRE((double)R * C <= 2147483647.0, "%s: R=%d x C=%d waves per threshold exceed the grid", what, R, C);
  SEDT_REQUIRE(n_ref_rec >= 0 && n_ref_events >= 0, "%s: reference table of %d recordings, %d events", what, n_ref_rec, n_ref_events);
  SEDT_REQUIRE(n_fusion >= 1 && fusion >= 0 && fusion < n_fusion, "%s: fusion %d of %d", what, fusion, n_fusion);
  if (R == 0) return 0;
  SEDT_REQUIRE(count && out && stitch_status && rec_idx && status, "%s: null pointer", what);
  SEDT_REQUIRE(n_ref_rec == 0 || ref_off, "%s: reference table missing", what);
  SEDT_REQUIRE(n_ref_events == 0 || (ref_on && ref_end), "%s: reference events missing", what);
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "%s: out is not 8-byte aligned", what);
  return 0;
}

}  // namespace sedt
