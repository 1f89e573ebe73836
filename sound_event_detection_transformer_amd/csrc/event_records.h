// event_records.h - the two event layouts the scoring kernels meet at, the limits they share and the small pieces each of them
// repeated: decode.hip writes the records; sweep.hip, psds.hip and stitch.hip read them; stitch.hip writes the stitched lists that
// recmetrics.hip and recpsds.hip read (recording_lists.h); metrics.hip decodes for itself under the same limits (event_match.h).
#pragma once
#include "common.h"

namespace sedt {

// ---- limits: one lane of a wave per query, per class and per reference event of a clip; one grid row per threshold
#define SEDT_MAX_QUERIES 64        // queries per clip = event slots of a record (one bit of a hit-graph row each)
#define SEDT_MAX_CLASSES 63        // classes (one lane, one BFS queue row each)
#define SEDT_MAX_REF_EVENTS 64     // reference events per clip (utilities/scoring.py: MAX_REF_EVENTS)
#define SEDT_MAX_THRESHOLDS 1024   // thresholds per launch (gridDim.y; ops.py: DECODE_MAX_THRESHOLDS)

// ---- the decode record of one (threshold, clip), records [K][B][1 + SEDT_REC_SLOT * Q] 32-bit words: {n, then Q slots of {class
// int32, onset f32, offset f32, score f32, query int32}}; the slots at or past n hold {-1, 0, 0, 0, -1}
#define SEDT_REC_SLOT 5
enum { SEDT_REC_CLASS, SEDT_REC_ONSET, SEDT_REC_OFFSET, SEDT_REC_SCORE, SEDT_REC_QUERY };

template <typename T>                                  // the record of (threshold kt, row b) of records [K][rows][..]
__device__ __forceinline__ T* record_at(T* records, int kt, int rows, int b, int Q) {
  return records + ((long)kt * rows + b) * (1 + SEDT_REC_SLOT * Q);
}
template <typename T>                                  // slot i of a record
__device__ __forceinline__ T* record_slot(T* rec, int i) {
  return rec + 1 + SEDT_REC_SLOT * i;
}

// ---- the stitched event, out [K][R][C][cap][SEDT_EVENT_WORDS] 32-bit words: {onset f64, offset f64, score f32, n_merged, window,
// query int32}, 8-byte aligned: as doubles, event i's onset and offset are [SEDT_EVENT_DOUBLES * i] and the one behind it
#define SEDT_EVENT_WORDS 8
#define SEDT_EVENT_DOUBLES (SEDT_EVENT_WORDS / 2)
enum { SEDT_EVENT_SCORE = 4, SEDT_EVENT_MERGED, SEDT_EVENT_WINDOW, SEDT_EVENT_QUERY };      // the words behind the two doubles

// ---- the two count blocks: integer atomics only, and a zero is not added.  cell[0 .. 3) += {a, b, c}: {tp, n_ref, n_sys}, {S, D, I}
__device__ __forceinline__ void add_counts3(unsigned long long* cell, long a, long b, long c) {
  if (a) atomicAdd(cell, (unsigned long long)a);
  if (b) atomicAdd(cell + 1, (unsigned long long)b);
  if (c) atomicAdd(cell + 2, (unsigned long long)c);
}
// cell[0 .. 3) += the presence outcome {tp, fp, fn} of one (clip or recording, class): in the reference / among the estimates
__device__ __forceinline__ void add_presence(unsigned long long* cell, bool ref_has, bool sys_has) {
  if (ref_has && sys_has) atomicAdd(cell, 1ull);
  if (!ref_has && sys_has) atomicAdd(cell + 1, 1ull);
  if (ref_has && !sys_has) atomicAdd(cell + 2, 1ull);
}

// ---- the argument checks of the three clip-level entry points (recording_lists.h: recording_args_ok is the counterpart); K = 1 for
// an entry point without a grid; `table`: whether every table pointer the kernel reads is there
static inline int clip_args_ok(const char* what, int B, int Q, int C, int K, int n_clips, bool table, int max_ref, int n_fusion,
                               int fusion) {
  SEDT_REQUIRE(B >= 0 && Q >= 1 && Q <= SEDT_MAX_QUERIES && C >= 1 && C <= SEDT_MAX_CLASSES, "%s: B=%d Q=%d (<=%d) C=%d (<=%d)", what, B, Q,
               SEDT_MAX_QUERIES, C, SEDT_MAX_CLASSES);
  SEDT_REQUIRE(K >= 1 && K <= SEDT_MAX_THRESHOLDS, "%s: %d thresholds (1 .. %d)", what, K, SEDT_MAX_THRESHOLDS);
  SEDT_REQUIRE(n_clips >= 0 && (n_clips == 0 || table), "%s: reference table missing", what);
  SEDT_REQUIRE(max_ref >= 0 && max_ref <= SEDT_MAX_REF_EVENTS, "%s: a clip has %d reference events (<= %d)", what, max_ref,
               SEDT_MAX_REF_EVENTS);
  SEDT_REQUIRE(n_fusion >= 1 && fusion >= 0 && fusion < n_fusion, "%s: fusion %d of %d", what, fusion, n_fusion);
  return 0;
}

}  // namespace sedt
