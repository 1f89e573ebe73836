// decode.hip - the predictions themselves on the device: reference engine.get_sedt_predictions' per-clip decode, written out
//   * decode_events_kernel   BoxEncoder.decode_strong (utilities/BoxEncoder.py:179-226) + the clip to [0, max_len] (engine.py:287),
//                            at one threshold or a whole grid of them, as event records in the reference's output order
// One wave per (clip, threshold).  Everything runs in f32 on PostProcess's f32 values, exactly as the reference's numpy / torch
// scalars do.  Each wave owns its record and writes all of it with plain stores: no atomics, nothing depends on launch order, and a
// replay never shows rows of an earlier batch.  The keep / sort / overlap pass repeats event_metrics_kernel's (metrics.hip) on
// purpose - that kernel orders by class index and writes nothing out; tests/test_decode_events_gpu.py pins the two to each other.
#include <cmath>

#include "common.h"
#include "event_records.h"

#pragma clang fp contract(off)     // offset - onset >= min_duration is the plain f32 subtract and compare of the reference

namespace sedt {

// block = 64 threads = one wave, blockIdx.x = clip of the batch, blockIdx.y = threshold of the grid.
//   out [K][B][1 + 5 Q] 32-bit words: the records of event_records.h
__global__ __launch_bounds__(64) void decode_events_kernel(const float* __restrict__ scores, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ boxes, const float* __restrict__ thresholds,
                                                           int class_wise, int B, int Q, int C, float min_dur, float max_len,
                                                           int del_overlap, int32_t* __restrict__ out) {
  __shared__ float s_on[SEDT_MAX_QUERIES], s_end[SEDT_MAX_QUERIES], s_score[SEDT_MAX_QUERIES];
  __shared__ int s_lab[SEDT_MAX_QUERIES], s_surv[SEDT_MAX_QUERIES], s_order[SEDT_MAX_QUERIES];
  const int b = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  // read on every launch: a captured graph follows an edited grid.  thresholds [K] (class_wise 0: one per operating point) or [K][C]
  // (one per operating point and class, looked up by the query's label once that is known to be a class)
  const float uniform = class_wise ? 0.f : thresholds[kt];

  // ---- decode_strong: keep (BoxEncoder.py:190-196 / :202-205)
  float on = 0.f, end = 0.f, sc = -INFINITY;
  int lab = -1;
  bool keep = false;
  if (lane < Q) {
    const long r = (long)b * Q + lane;
    sc = scores[r];
    const int64_t l = labels[r];
    on = boxes[2 * r];
    end = boxes[2 * r + 1];
    const bool is_class = l >= 0 && l < C;                             // tested before the lookup: any other label reads nothing
    const float threshold = !class_wise ? uniform : is_class ? thresholds[(long)kt * C + l] : INFINITY;
    const bool pass = del_overlap ? (sc >= threshold) : (sc > threshold);
    keep = pass && (end - on) >= min_dur && is_class;
    lab = keep ? (int)l : -1;
  }
  // ---- order: with del_overlap (class by its first kept query - the reference's dict insertion order -, onset, query), else query.
  // `first` names the class of a kept query: the lowest kept query with its label
  int first = lane;
  for (int j = 0; j < Q; ++j) {
    const int lj = __shfl(lab, j, 64);                                // -1 where query j is not kept
    if (keep && lj == lab && j < first) first = j;
  }
  int pos = 0, start = 0, n_c = 0;                                    // output position before the deletions; run of the class
  for (int j = 0; j < Q; ++j) {
    const int kj = __shfl((int)keep, j, 64), fj = __shfl(first, j, 64);
    const float oj = __shfl(on, j, 64);
    const bool before = del_overlap ? (fj < first || (fj == first && (oj < on || (oj == on && j < lane)))) : j < lane;
    pos += (kj && before) ? 1 : 0;
    start += (kj && fj < first) ? 1 : 0;
    n_c += (kj && fj == first) ? 1 : 0;
  }
  s_on[lane] = on; s_end[lane] = end; s_score[lane] = sc; s_lab[lane] = lab;
  s_surv[lane] = keep;
  if (keep) s_order[pos] = lane;                                      // a permutation of [0, kept): the keys are distinct
  __syncthreads();

  // ---- sequential same-class overlap removal in onset order (BoxEncoder.py:212-223), by the class's first kept query: an event
  // starting before the end of the last one still standing removes it when its score is strictly higher, else is removed itself
  if (del_overlap && keep && first == lane && n_c > 1) {
    int top = s_order[start];
    for (int k = 1; k < n_c; ++k) {
      const int q = s_order[start + k];
      if (s_on[q] < s_end[top]) {
        if (s_score[q] > s_score[top]) {
          s_surv[top] = 0;
          top = q;
        } else {
          s_surv[q] = 0;
        }
      } else {
        top = q;
      }
    }
  }
  __syncthreads();

  // ---- compact the survivors in order (lane = position before the deletions) and write the record
  const unsigned long long kept = __ballot(keep);
  const int n_kept = __popcll(kept);
  const int q = lane < n_kept ? s_order[lane] : 0;
  const bool surv = lane < n_kept && s_surv[q];
  const unsigned long long alive = __ballot(surv);
  const int n = __popcll(alive);
  int32_t* rec = record_at(out, kt, B, b, Q);
  if (lane == 0) rec[0] = n;
  if (surv) {
    float o = s_on[q], e = s_end[q];
    if (max_len < INFINITY) {                                          // engine.py:287; +inf: the decode as decode_strong returns it
      o = fminf(fmaxf(o, 0.f), max_len);
      e = fminf(fmaxf(e, 0.f), max_len);
    }
    int32_t* s = record_slot(rec, __popcll(alive & ((1ull << lane) - 1ull)));
    s[SEDT_REC_CLASS] = s_lab[q];
    s[SEDT_REC_ONSET] = __float_as_int(o);
    s[SEDT_REC_OFFSET] = __float_as_int(e);
    s[SEDT_REC_SCORE] = __float_as_int(s_score[q]);
    s[SEDT_REC_QUERY] = q;
  }
  if (lane >= n && lane < Q) {
    int32_t* s = record_slot(rec, lane);
    s[SEDT_REC_CLASS] = -1; s[SEDT_REC_ONSET] = 0; s[SEDT_REC_OFFSET] = 0; s[SEDT_REC_SCORE] = 0; s[SEDT_REC_QUERY] = -1;
  }
}

}  // namespace sedt

namespace sedt {

int decode_events_launch(const char* what, const float* scores, const int64_t* labels, const float* boxes, const float* thresholds,
                         int class_wise, int B, int Q, int C, int K, float min_duration, double max_len, int del_overlap, int32_t* out,
                         void* stream) {
  SEDT_REQUIRE(scores && labels && boxes && thresholds && out, "%s: null pointer", what);
  SEDT_REQUIRE(B >= 0 && Q >= 1 && Q <= SEDT_MAX_QUERIES && C >= 1 && C <= SEDT_MAX_CLASSES, "%s: B=%d Q=%d (<=%d) C=%d (<=%d)", what, B, Q,
               SEDT_MAX_QUERIES, C, SEDT_MAX_CLASSES);
  SEDT_REQUIRE(K >= 1 && K <= SEDT_MAX_THRESHOLDS, "%s: %d thresholds (1 .. %d)", what, K, SEDT_MAX_THRESHOLDS);
  SEDT_REQUIRE(max_len >= 0.0 && (double)(float)max_len == max_len,
               "%s: max_len %.17g is not a non-negative number float32 represents exactly (+inf: no clip)", what, max_len);
  if (B == 0) return 0;
  hipLaunchKernelGGL(decode_events_kernel, dim3(B, K), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), scores, labels, boxes,
                     thresholds, class_wise, B, Q, C, min_duration, (float)max_len, del_overlap, out);
  return check_launch(what);
}

}  // namespace sedt

extern "C" int sedt_decode_events(const float* scores, const int64_t* labels, const float* boxes, const float* thresholds, int B, int Q,
                                  int C, int K, float min_duration, double max_len, int del_overlap, int32_t* out, void* stream) {
  return sedt::decode_events_launch("decode_events", scores, labels, boxes, thresholds, 0, B, Q, C, K, min_duration, max_len, del_overlap,
                                    out, stream);
}

extern "C" int sedt_decode_events_classwise(const float* scores, const int64_t* labels, const float* boxes, const float* thresholds,
                                            int B, int Q, int C, int K, float min_duration, double max_len, int del_overlap, int32_t* out,
                                            void* stream) {
  return sedt::decode_events_launch("decode_events_classwise", scores, labels, boxes, thresholds, 1, B, Q, C, K, min_duration, max_len,
                                    del_overlap, out, stream);
}
