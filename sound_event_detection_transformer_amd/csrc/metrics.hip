// metrics.hip - validation scores on the device: the per-clip part of reference engine.get_sedt_predictions + utilities/metrics.py
//   * event_metrics_kernel   BoxEncoder.decode_strong (utilities/BoxEncoder.py:179-226) + the clip to [0, max_len] (engine.py:287)
//                            + sed_eval EventBasedMetrics counts (metrics.py:43-80: t_collar, percentage_of_length, onset and offset)
//                            + clip-level tag counts of the decoded events and of the audio-tag head (metrics.py:281-322)
//                            + (SEG) sed_eval SegmentBasedMetrics counts (metrics.py:83-116): class-wise and per-segment S / D / I
// One wave per clip.  The decode runs in f32 on PostProcess's f32 values, exactly as the reference's numpy / torch scalars do; the
// matching conditions run in float64 on those values, as sed_eval compares Python floats.  Counts land in int64 counters through
// integer atomics only: every result is independent of the order the clips arrive in.
#include <cfloat>

#include "common.h"
#include "event_match.h"

#pragma clang fp contract(off)     // the float64 collar tests must be the plain sub / mul / compare sed_eval evaluates

namespace sedt {

#define SEDT_EM_MAXSEG 1024        // segments per clip of the segment-based counts (10 s at 10 ms)
#define SEDT_EM_SEGW (SEDT_EM_MAXSEG / 64)   // 64-bit words of one class's segment row

// segments floor(on / r) <= k < ceil(off / r) of one event into its class's bit row (W words): float64 divisions, as sed_eval's
// event_list_to_event_roll computes `onset * 1 / time_resolution`; an empty range sets nothing, events of one class OR together
__device__ inline void seg_raster(unsigned long long* row, double on, double off, double r, int W) {
  const double nb = 64.0 * W;       // the host bounds every ceil(off / r) by the roll length: the clamps only keep LDS in range
  const int k0 = (int)fmin(fmax(floor(on / r), 0.0), nb), k1 = (int)fmin(fmax(ceil(off / r), 0.0), nb);
  if (k0 >= k1) return;
  for (int w = k0 >> 6; 64 * w < k1; ++w) {
    const int lo = max(k0 - 64 * w, 0), hi = min(k1 - 64 * w, 64);
    const unsigned long long m = (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
    atomicOr(row + w, m);                                           // ds_or_b64
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// block = 64 threads = one wave, blockIdx.x = clip of the batch.
//   ev  [n_fusion][C][3] += {tp, n_ref, n_sys}       (only clips that are in the reference: clip_idx >= 0)
//   tag [n_fusion + 1][C][3] += {tp, fp, fn}         (every clip: reference clips and clips without any reference row alike)
// SEG: the segment-based counts at resolution seg_res over seg_words words of 64 segments (reference clips only):
//   seg [n_fusion][C][3] += {tp, n_ref, n_sys}       (segments where the class is active in both / in the reference / in the estimates)
//   sdi [n_fusion][3]    += {S, D, I}                (per segment over the classes: substitutions, deletions, insertions)
template <bool SEG>
__global__ __launch_bounds__(64) void event_metrics_kernel(const float* __restrict__ scores, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ boxes, const int64_t* __restrict__ at_tags,
                                                           const int32_t* __restrict__ clip_idx, const int32_t* __restrict__ ref_present,
                                                           const int32_t* __restrict__ ref_off,
                                                           const int32_t* __restrict__ ref_cls, const double* __restrict__ ref_on,
                                                           const double* __restrict__ ref_end, int n_clips, int Q, int C, int n_fusion,
                                                           int fusion, float threshold, float min_dur, double max_len, double t_collar,
                                                           double pct, int del_overlap, int optimal, unsigned long long* __restrict__ ev,
                                                           unsigned long long* __restrict__ tag, double seg_res, int seg_words,
                                                           unsigned long long* __restrict__ seg, unsigned long long* __restrict__ sdi) {
  __shared__ float s_on[SEDT_MAX_QUERIES], s_end[SEDT_MAX_QUERIES], s_score[SEDT_MAX_QUERIES];
  __shared__ int s_lab[SEDT_MAX_QUERIES], s_keep[SEDT_MAX_QUERIES], s_surv[SEDT_MAX_QUERIES], s_order[SEDT_MAX_QUERIES];
  __shared__ int r_cls[SEDT_MAX_REF_EVENTS];
  __shared__ double r_on[SEDT_MAX_REF_EVENTS], r_end[SEDT_MAX_REF_EVENTS];
  __shared__ unsigned long long adj[SEDT_MAX_REF_EVENTS];                  // adj[j] bit q: estimate q hits reference j
  __shared__ int match_est[SEDT_MAX_QUERIES], from_ref[SEDT_MAX_QUERIES], match_ref[SEDT_MAX_REF_EVENTS];
  __shared__ unsigned char queue[SEDT_MAX_CLASSES][SEDT_MAX_REF_EVENTS];       // BFS queue of class c (refs of one class, one clip)
  const int b = blockIdx.x, lane = threadIdx.x;
  int clip = clip_idx[b];
  if (clip >= n_clips || (clip >= 0 && ref_present && !ref_present[clip])) clip = -1;   // not in the reference (the host validates)
  int e0 = 0, ne = 0;
  if (clip >= 0) {
    e0 = ref_off[clip];
    ne = min(ref_off[clip + 1] - e0, SEDT_MAX_REF_EVENTS);                  // sedt_event_metrics_update checks the table on the host
  }

  // ---- decode_strong: keep, then order by (class, onset, query) with del_overlap / (class, query) without
  float on = 0.f, end = 0.f, sc = -INFINITY;
  int lab = 0;
  bool keep = false;
  if (lane < Q) {
    const long r = (long)b * Q + lane;
    sc = scores[r];
    lab = (int)labels[r];
    on = boxes[2 * r];
    end = boxes[2 * r + 1];
    const bool pass = del_overlap ? (sc >= threshold) : (sc > threshold);   // BoxEncoder.py:203 / :190
    keep = pass && (end - on) >= min_dur && lab >= 0 && lab < C;
  }
  int pos = 0;
  for (int j = 0; j < Q; ++j) {
    const int kj = __shfl((int)keep, j, 64), lj = __shfl(lab, j, 64);
    const float oj = __shfl(on, j, 64);
    const bool before = lj < lab || (lj == lab && (del_overlap ? (oj < on || (oj == on && j < lane)) : j < lane));
    pos += (kj && before) ? 1 : 0;
  }
  if (lane < SEDT_MAX_QUERIES) {
    s_on[lane] = on; s_end[lane] = end; s_score[lane] = sc; s_lab[lane] = lab;
    s_keep[lane] = keep; s_surv[lane] = keep;
    match_est[lane] = -1;
  }
  if (keep) s_order[pos] = lane;
  for (int j = lane; j < ne; j += 64) {
    r_cls[j] = ref_cls[e0 + j];
    r_on[j] = ref_on[e0 + j];
    r_end[j] = ref_end[e0 + j];
    match_ref[j] = -1;
  }
  __syncthreads();

  // per class (lane c): its run [start, start + n) of s_order
  const int c = lane;
  int start = 0, n_c = 0;
  if (c < C)
    for (int j = 0; j < Q; ++j)
      if (s_keep[j]) {
        start += s_lab[j] < c;
        n_c += s_lab[j] == c;
      }
  // ---- sequential same-class overlap removal in onset order (BoxEncoder.py:212-223): an event overlapping the last one still
  // standing removes it when its score is strictly higher, else is removed itself
  if (del_overlap && c < C && n_c > 1) {
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
  // ---- hit graph: same class, |on_r - on_e| <= collar, |off_r - off_e| <= max(collar, pct * (off_r - on_r)), in float64 on the
  // estimates clipped to [0, max_len] (engine.py:287)
  const bool surv = lane < Q && s_surv[lane];
  const double my_on = fmin(fmax((double)on, 0.0), max_len), my_end = fmin(fmax((double)end, 0.0), max_len);
  event_hit_graph(adj, r_cls, r_on, r_end, ne, surv, lab, my_on, my_end, t_collar, pct, lane);
  __syncthreads();

  // ---- per class: tp = maximum-cardinality matching (augmenting paths, breadth first) or sed_eval's greedy pass (event_match.h)
  long tp = 0, n_ref = 0, n_sys = 0;
  if (c < C) {
    for (int k = 0; k < n_c; ++k) n_sys += s_surv[s_order[start + k]];
    tp = event_class_match(c, ne, r_cls, adj, match_est, from_ref, match_ref, queue[c], optimal, s_order + start, n_c, n_ref);
    if (clip >= 0) add_counts3(ev + ((long)fusion * C + c) * 3, tp, n_ref, n_sys);
    // ---- clip level: class present among the decoded events / among the reference events / among the audio tags
    add_presence(tag + ((long)fusion * C + c) * 3, n_ref > 0, n_sys > 0);
    if (at_tags) add_presence(tag + ((long)n_fusion * C + c) * 3, n_ref > 0, at_tags[(long)b * C + c] != 0);
  }

  // ---- segment-based counts (sed_eval SegmentBasedMetrics): the clipped survivors (the values the hit test used) and the clip's
  // reference events as per-class bit rows, roll_*[c * W + w] bit b = segment 64 w + b; the roll lengths and their padding only add
  // true negatives, which are not counted
  if constexpr (SEG) {
    if (clip < 0) return;                                          // block-uniform: only reference clips are evaluated
    __shared__ unsigned long long roll_ref[SEDT_MAX_CLASSES * SEDT_EM_SEGW], roll_sys[SEDT_MAX_CLASSES * SEDT_EM_SEGW];
    const int W = seg_words;
    for (int i = lane; i < C * W; i += 64) {
      roll_ref[i] = 0ull;
      roll_sys[i] = 0ull;
    }
    __syncthreads();
    if (surv) seg_raster(roll_sys + lab * W, my_on, my_end, seg_res, W);
    if (lane < ne) seg_raster(roll_ref + r_cls[lane] * W, r_on[lane], r_end[lane], seg_res, W);
    __syncthreads();
    // class-wise (lane = class): segments active in both, in the reference, in the estimates
    int s_tp = 0, s_ref = 0, s_sys = 0;
    if (c < C) {
      for (int w = 0; w < W; ++w) {
        const unsigned long long a = roll_ref[c * W + w], s = roll_sys[c * W + w];
        s_tp += __popcll(a & s);
        s_ref += __popcll(a);
        s_sys += __popcll(s);
      }
      add_counts3(seg + ((long)fusion * C + c) * 3, s_tp, s_ref, s_sys);
    }
    // per segment (lane = bit of the word), over the classes active anywhere in the clip (the others add nothing):
    // S += min(Nref, Nsys) - Ntp, D += max(0, Nref - Nsys), I += max(0, Nsys - Nref)
    const unsigned long long act = __ballot(c < C && (s_ref | s_sys) != 0);
    int n_sub = 0, n_del = 0, n_ins = 0;
    for (int w = 0; w < W; ++w) {
      int nref = 0, nsys = 0, ntp = 0;
      for (unsigned long long m = act; m; m &= m - 1ull) {
        const int k = (__ffsll((long long)m) - 1) * W + w;
        const int a = (int)(roll_ref[k] >> lane) & 1, s = (int)(roll_sys[k] >> lane) & 1;
        nref += a;
        nsys += s;
        ntp += a & s;
      }
      n_sub += min(nref, nsys) - ntp;
      n_del += max(0, nref - nsys);
      n_ins += max(0, nsys - nref);
    }
    for (int o = 32; o > 0; o >>= 1) {
      n_sub += __shfl_xor(n_sub, o, 64);
      n_del += __shfl_xor(n_del, o, 64);
      n_ins += __shfl_xor(n_ins, o, 64);
    }
    if (lane == 0) add_counts3(sdi + (long)fusion * 3, n_sub, n_del, n_ins);
  }
}

template <bool SEG>
int event_metrics_launch(const char* what, const float* scores, const int64_t* labels, const float* boxes, const int64_t* at_tags,
                         const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off, const int32_t* ref_cls,
                         const double* ref_on, const double* ref_end, int n_clips, int max_ref, int B, int Q, int C, int n_fusion,
                         int fusion, float threshold, float min_duration, double max_len, double t_collar, double pct, int del_overlap,
                         int optimal, int64_t* ev_counts, int64_t* tag_counts, double seg_res, int seg_words, int64_t* seg_counts,
                         int64_t* sdi_counts, void* stream) {
  SEDT_REQUIRE(scores && labels && boxes && clip_idx && ref_off && ev_counts && tag_counts, "event_metrics_update: null pointer");
  // one threshold: K = 1
  if (clip_args_ok("event_metrics_update", B, Q, C, 1, n_clips, ref_cls && ref_on && ref_end, max_ref, n_fusion, fusion)) return 1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(event_metrics_kernel<SEG>, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), scores, labels, boxes,
                     at_tags, clip_idx, ref_present, ref_off, ref_cls, ref_on, ref_end, n_clips, Q, C, n_fusion, fusion, threshold,
                     min_duration, max_len, t_collar, pct, del_overlap, optimal, reinterpret_cast<unsigned long long*>(ev_counts),
                     reinterpret_cast<unsigned long long*>(tag_counts), seg_res, seg_words,
                     reinterpret_cast<unsigned long long*>(seg_counts), reinterpret_cast<unsigned long long*>(sdi_counts));
  return check_launch(what);
}

}  // namespace sedt

extern "C" int sedt_event_metrics_update(const float* scores, const int64_t* labels, const float* boxes, const int64_t* at_tags,
                                         const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off,
                                         const int32_t* ref_cls, const double* ref_on,
                                         const double* ref_end, int n_clips, int max_ref, int B, int Q, int C, int n_fusion, int fusion,
                                         float threshold, float min_duration, double max_len, double t_collar, double pct,
                                         int del_overlap, int optimal, int64_t* ev_counts, int64_t* tag_counts, void* stream) {
  return sedt::event_metrics_launch<false>("event_metrics_update", scores, labels, boxes, at_tags, clip_idx, ref_present, ref_off,
                                           ref_cls, ref_on, ref_end, n_clips, max_ref, B, Q, C, n_fusion, fusion, threshold,
                                           min_duration, max_len, t_collar, pct, del_overlap, optimal, ev_counts, tag_counts, 0.0, 0,
                                           nullptr, nullptr, stream);
}

extern "C" int sedt_event_segment_metrics_update(const float* scores, const int64_t* labels, const float* boxes, const int64_t* at_tags,
                                                 const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off,
                                                 const int32_t* ref_cls, const double* ref_on, const double* ref_end, int n_clips,
                                                 int max_ref, int B, int Q, int C, int n_fusion, int fusion, float threshold,
                                                 float min_duration, double max_len, double t_collar, double pct, int del_overlap,
                                                 int optimal, int64_t* ev_counts, int64_t* tag_counts, double time_resolution,
                                                 int n_seg_words, int64_t* seg_counts, int64_t* sdi_counts, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(seg_counts && sdi_counts, "event_segment_metrics_update: null pointer");
  SEDT_REQUIRE(time_resolution > 0.0 && time_resolution <= DBL_MAX, "event_segment_metrics_update: time_resolution %g", time_resolution);
  SEDT_REQUIRE(n_seg_words >= 1 && n_seg_words <= SEDT_EM_SEGW,
               "event_segment_metrics_update: %d segment words (1 .. %d: at most %d segments per clip)", n_seg_words, SEDT_EM_SEGW,
               SEDT_EM_MAXSEG);
  return event_metrics_launch<true>("event_segment_metrics_update", scores, labels, boxes, at_tags, clip_idx, ref_present, ref_off,
                                    ref_cls, ref_on, ref_end, n_clips, max_ref, B, Q, C, n_fusion, fusion, threshold, min_duration,
                                    max_len, t_collar, pct, del_overlap, optimal, ev_counts, tag_counts, time_resolution, n_seg_words,
                                    seg_counts, sdi_counts, stream);
}
