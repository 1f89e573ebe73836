// sweep.hip - the operating points of a validation set: sed_eval's event-based and the clip-level counts of event_metrics_kernel
// (metrics.hip) at EVERY threshold of the decoder's grid, from the event records decode_events_kernel (decode.hip) wrote
//   * event_sweep_kernel   records [K][B][1 + 5 Q] + the clip's reference events -> ev [K][C][3] += {tp, n_ref, n_sys},
//                          tag [K][C][3] += {tp, fp, fn}
// One wave per (clip, threshold).  The decode is not repeated: the kernels meet at the packed record, whose times are already clipped
// to [0, max_len].  The hit test runs in float64 on the record's f32 times widened, the matching is event_match.h's - the code
// event_metrics_kernel runs, so at threshold k the counts are what that kernel counts at grid[k].  Decode and matching are both class
// by class: under class-wise thresholds the counts of class c are those of the uniform threshold of class c.  Counts land in int64
// counters through integer atomics only: a replay is bit-reproducible and independent of the order the clips arrive in.
#include "common.h"
#include "event_match.h"

#pragma clang fp contract(off)     // the float64 collar tests must be the plain sub / mul / compare sed_eval evaluates

namespace sedt {

// block = 64 threads = one wave, blockIdx.x = clip of the batch, blockIdx.y = threshold of the grid; ev / tag: this fusion strategy's
// [K][C][3]
__global__ __launch_bounds__(64) void event_sweep_kernel(const int32_t* __restrict__ records, const int32_t* __restrict__ clip_idx,
                                                         const int32_t* __restrict__ ref_present, const int32_t* __restrict__ ref_off,
                                                         const int32_t* __restrict__ ref_cls, const double* __restrict__ ref_on,
                                                         const double* __restrict__ ref_end, int n_clips, int B, int Q, int C,
                                                         double t_collar, double pct, int optimal, unsigned long long* __restrict__ ev,
                                                         unsigned long long* __restrict__ tag) {
  __shared__ int d_cls[SEDT_MAX_QUERIES];                               // -1: not a live slot of a class 0 .. C - 1
  __shared__ int r_cls[SEDT_MAX_REF_EVENTS];
  __shared__ double r_on[SEDT_MAX_REF_EVENTS], r_end[SEDT_MAX_REF_EVENTS];
  __shared__ unsigned long long adj[SEDT_MAX_REF_EVENTS];                  // adj[j] bit q: slot q hits reference j
  __shared__ int match_est[SEDT_MAX_QUERIES], from_ref[SEDT_MAX_QUERIES], match_ref[SEDT_MAX_REF_EVENTS];
  __shared__ unsigned char queue[SEDT_MAX_CLASSES][SEDT_MAX_REF_EVENTS];       // BFS queue of class c (refs of one class, one clip)
  const int b = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  const int32_t* rec = record_at(records, kt, B, b, Q);
  const int n = rec[0];
  if (n < 0 || n > Q) return;                                        // not a count decode_events writes: block-uniform
  int clip = clip_idx[b];
  if (clip < 0 || clip >= n_clips || (ref_present && !ref_present[clip])) clip = -1;   // not in the reference: clip level only
  int e0 = 0, ne = 0;
  if (clip >= 0) {
    e0 = ref_off[clip];
    ne = min(max(ref_off[clip + 1] - e0, 0), SEDT_MAX_REF_EVENTS);          // sedt_event_sweep_update bounds max_ref on the host
  }

  // ---- stage: lane = slot of the record, lane = reference event
  int cls = -1;
  double on = 0.0, end = 0.0;
  if (lane < n) {
    const int32_t* s = record_slot(rec, lane);
    cls = s[SEDT_REC_CLASS];
    on = (double)__int_as_float(s[SEDT_REC_ONSET]);
    end = (double)__int_as_float(s[SEDT_REC_OFFSET]);
    if (cls < 0 || cls >= C) cls = -1;                               // never an index, not counted
  }
  d_cls[lane] = cls;
  match_est[lane] = -1;
  match_ref[lane] = -1;
  if (lane < ne) {
    r_cls[lane] = ref_cls[e0 + lane];
    r_on[lane] = ref_on[e0 + lane];
    r_end[lane] = ref_end[e0 + lane];
  }
  __syncthreads();
  event_hit_graph(adj, r_cls, r_on, r_end, ne, cls >= 0, cls, on, end, t_collar, pct, lane);
  __syncthreads();

  // ---- per class (lane c): the estimates are the record's slots of class c in record order (order == nullptr: index order)
  const int c = lane;
  if (c >= C) return;
  long n_ref = 0, n_sys = 0;
  for (int d = 0; d < n; ++d) n_sys += d_cls[d] == c;
  const long tp = event_class_match(c, ne, r_cls, adj, match_est, from_ref, match_ref, queue[c], optimal, nullptr, 0, n_ref);
  const long cell = ((long)kt * C + c) * 3;
  if (clip >= 0) add_counts3(ev + cell, tp, n_ref, n_sys);
  // ---- clip level: class present among the record's events / among the reference events; every clip counts
  add_presence(tag + cell, n_ref > 0, n_sys > 0);
}

}  // namespace sedt

extern "C" int sedt_event_sweep_update(const int32_t* records, const int32_t* clip_idx, const int32_t* ref_present,
                                       const int32_t* ref_off, const int32_t* ref_cls, const double* ref_on, const double* ref_end,
                                       int n_clips, int max_ref, int B, int Q, int C, int K, int n_fusion, int fusion, double t_collar,
                                       double pct, int optimal, int64_t* ev_counts, int64_t* tag_counts, void* stream) {
  using namespace sedt;
  if (clip_args_ok("event_sweep_update", B, Q, C, K, n_clips, ref_cls && ref_on && ref_end, max_ref, n_fusion, fusion)) return 1;
  if (B == 0) return 0;
  SEDT_REQUIRE(records && clip_idx && ref_off && ev_counts && tag_counts, "event_sweep_update: null pointer");
  const long mine = (long)fusion * K * C * 3;
  hipLaunchKernelGGL(event_sweep_kernel, dim3(B, K), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), records, clip_idx, ref_present,
                     ref_off, ref_cls, ref_on, ref_end, n_clips, B, Q, C, t_collar, pct, optimal,
                     reinterpret_cast<unsigned long long*>(ev_counts) + mine, reinterpret_cast<unsigned long long*>(tag_counts) + mine);
  return check_launch("event_sweep_update");
}
