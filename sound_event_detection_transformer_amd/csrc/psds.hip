// psds.hip - the per-operating-point confusion counts of the polyphonic sound detection score (Bilen et al., ICASSP 2020; psds_eval's
// PSDSEval restated, utilities/psds.py holds the definition) from the event records decode_events_kernel (decode.hip) wrote
//   * psds_update_kernel   records [K][B][1 + 5 Q] + the clip's reference events -> counts [K][C][C + 1] += {true positives on the
//                          diagonal, cross triggers off it, false positives in the last (world) column}
// One wave per (clip, threshold).  The decode is not repeated: the two kernels meet at the packed record.  All arithmetic is float64 on
// the record's f32 values widened; every term is a plain division added to a running sum in a fixed order (reference events in table
// order, detections in record order), so a sum that lands exactly on a threshold does so here and on the host alike.  Counts land in
// int64 counters through integer atomics only: a replay is bit-reproducible and independent of the order the clips arrive in.
#include "common.h"
#include "event_records.h"

#pragma clang fp contract(off)     // inter / dur added to a running sum: no fused multiply-add may stand in for the division's tail

namespace sedt {

// the part of detection [on, off] inside reference event j, as a fraction of `dur`, added to `sum` when it is positive
__device__ inline double add_overlap(double sum, double on, double off, double r_on, double r_end, double dur) {
  const double inter = fmin(off, r_end) - fmax(on, r_on);
  return inter > 0.0 ? sum + inter / dur : sum;
}

// block = 64 threads = one wave, blockIdx.x = clip of the batch, blockIdx.y = threshold of the grid; counts: this fusion strategy's
// [K][C][C + 1]
__global__ __launch_bounds__(64) void psds_update_kernel(const int32_t* __restrict__ records, const int32_t* __restrict__ clip_idx,
                                                         const int32_t* __restrict__ ref_present, const int32_t* __restrict__ ref_off,
                                                         const int32_t* __restrict__ ref_cls, const double* __restrict__ ref_on,
                                                         const double* __restrict__ ref_end, const double* __restrict__ ref_dur,
                                                         int n_clips, int B, int Q, int C, double dtc, double gtc, double cttc,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ int r_cls[SEDT_MAX_REF_EVENTS], d_cls[SEDT_MAX_QUERIES];            // -1: takes part in nothing / did not pass the DTC
  __shared__ double r_on[SEDT_MAX_REF_EVENTS], r_end[SEDT_MAX_REF_EVENTS], d_on[SEDT_MAX_QUERIES], d_end[SEDT_MAX_QUERIES];
  const int b = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  const int clip = clip_idx[b];
  if (clip < 0 || clip >= n_clips || (ref_present && !ref_present[clip])) return;      // outside the table: block-uniform
  const int32_t* rec = record_at(records, kt, B, b, Q);
  const int n = rec[0];
  if (n < 0 || n > Q) return;                                           // not a count decode_events writes: block-uniform
  const int e0 = ref_off[clip];
  const int ne = min(max(ref_off[clip + 1] - e0, 0), SEDT_MAX_REF_EVENTS);     // sedt_psds_update bounds max_ref on the host
  const double clip_len = ref_dur[clip];
  unsigned long long* row0 = counts + (long)kt * C * (C + 1);

  // ---- stage the clip's reference events; one with a class outside 0 .. C - 1 or a duration <= 0 takes part in nothing
  {
    int c = -1;
    double on = 0.0, end = 0.0;
    if (lane < ne) {
      c = ref_cls[e0 + lane];
      on = ref_on[e0 + lane];
      end = ref_end[e0 + lane];
      if (c < 0 || c >= C || !(end - on > 0.0)) c = -1;
    }
    r_cls[lane] = c; r_on[lane] = on; r_end[lane] = end;
  }
  __syncthreads();
  unsigned long long in_clip = 0ull;                                    // classes with a reference event in this clip
  for (int j = 0; j < ne; ++j)
    if (r_cls[j] >= 0) in_clip |= 1ull << r_cls[j];

  // ---- phase 1, lane = detection slot: DTC against the references of its own class; a detection that fails it may cross-trigger
  // every other class and may be a false positive
  int cls = -1;
  double on = 0.0, off = 0.0, dur = 0.0;
  if (lane < n) {
    const int32_t* s = record_slot(rec, lane);
    cls = s[SEDT_REC_CLASS];
    on = (double)__int_as_float(s[SEDT_REC_ONSET]);
    off = (double)__int_as_float(s[SEDT_REC_OFFSET]);
    dur = off - on;
    if (cls < 0 || cls >= C || !(dur > 0.0)) cls = -1;                  // never an index
  }
  bool pass = false;
  if (cls >= 0) {
    double p = 0.0;
    for (int j = 0; j < ne; ++j)
      if (r_cls[j] == cls) p = add_overlap(p, on, off, r_on[j], r_end[j], dur);
    pass = p >= dtc;
  }
  d_cls[lane] = pass ? cls : -1; d_on[lane] = on; d_end[lane] = off;
  if (cls >= 0 && !pass) {
    unsigned long long* row = row0 + (long)cls * (C + 1);
    for (int c = 0; c < C; ++c) {
      if (c == cls) continue;
      double x = 0.0;
      if ((in_clip >> c) & 1ull)
        for (int j = 0; j < ne; ++j)
          if (r_cls[j] == c) x = add_overlap(x, on, off, r_on[j], r_end[j], dur);
      if (x >= cttc) atomicAdd(row + c, 1ull);
    }
    const double world = (fmin(off, clip_len) - fmax(on, 0.0)) / dur;   // the detection inside [0, D_k]: psds_eval's "world" label
    if (world >= cttc) atomicAdd(row + C, 1ull);
  }
  __syncthreads();

  // ---- phase 2, lane = reference event: GTC over the detections of its class that passed the DTC, in record order
  const int g = r_cls[lane];
  if (g >= 0) {
    const double g_on = r_on[lane], g_end = r_end[lane], g_dur = g_end - g_on;
    double v = 0.0;
    for (int d = 0; d < n; ++d)
      if (d_cls[d] == g) v = add_overlap(v, d_on[d], d_end[d], g_on, g_end, g_dur);
    if (v >= gtc) atomicAdd(row0 + (long)g * (C + 1) + g, 1ull);
  }
}

}  // namespace sedt

extern "C" int sedt_psds_update(const int32_t* records, const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off,
                                const int32_t* ref_cls, const double* ref_on, const double* ref_end, const double* ref_dur, int n_clips,
                                int max_ref, int B, int Q, int C, int K, int n_fusion, int fusion, double dtc, double gtc, double cttc,
                                int64_t* counts, void* stream) {
  using namespace sedt;
  if (clip_args_ok("psds_update", B, Q, C, K, n_clips, ref_cls && ref_on && ref_end && ref_dur, max_ref, n_fusion, fusion)) return 1;
  SEDT_REQUIRE(dtc == dtc && gtc == gtc && cttc == cttc, "psds_update: a tolerance criterion is NaN (dtc %g gtc %g cttc %g)", dtc, gtc, cttc);
  if (B == 0) return 0;
  SEDT_REQUIRE(records && clip_idx && ref_off && counts, "psds_update: null pointer");
  unsigned long long* mine = reinterpret_cast<unsigned long long*>(counts) + (long)fusion * K * C * (C + 1);
  hipLaunchKernelGGL(psds_update_kernel, dim3(B, K), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), records, clip_idx, ref_present,
                     ref_off, ref_cls, ref_on, ref_end, ref_dur, n_clips, B, Q, C, dtc, gtc, cttc, mine);
  return check_launch("psds_update");
}
