// stitch.hip - recordings of any length: the event records of a recording's overlapping windows (decode_events_kernel, decode.hip)
// merged into one event list per (threshold, recording, class)
//   * stitch_events_kernel   an event a window boundary cut in two, or one that two overlapping windows both report, becomes one event
// The reference scores 10 s dataset clips only and has no counterpart; DESIGN.md section 4 ("Recordings of any length") holds the
// definition and tests/recording_ref.py restates it in NumPy.
// One wave per (recording, threshold) sweeps the recording's windows in start order with the OPEN merged events in LDS.  An event of
// window w cannot start before t_w, so a merged event with off + merge_gap < t_w can gain no member once window w is reached: it is
// written out and leaves the set.  What stays open at window w comes from the few earlier windows that still reach t_w (D of them,
// D <= 8 by the Python side's plan check), at most D * Q events of all classes together - a recording of any number of windows runs
// in the same 36 KB of LDS.  Float64 adds and compares on the records' f32 values widened; plain stores, integer LDS operations only:
// the result does not depend on launch order and two launches give the same bytes.
#include <cmath>

#include "common.h"
#include "event_records.h"

#pragma clang fp contract(off)     // t_w + on32, off + merge_gap: the plain float64 add and compare of the definition

namespace sedt {

#define SEDT_ST_OPEN 640           // open merged events + the candidates of the window being added: (8 + 1) * 64 and a chunk to spare

#define SEDT_ST_UNORDERED 1        // status bits: win_start of the recording not ascending (or NaN)
#define SEDT_ST_OVERFLOW 2         //   more than SEDT_ST_OPEN open events + candidates at some window
#define SEDT_ST_EARLY 4            //   a kept candidate starts before its window does (a negative onset in a record)
#define SEDT_ST_TABLE 8            //   win_off[r] .. win_off[r + 1] is not a range inside 0 .. W

// the member of a merged event that gives score, window and query: the highest score; among equal scores the first in (on, w, s)
__device__ __forceinline__ bool st_better(float sa, double oa, int wa, int la, float sb, double ob, int wb, int lb) {
  if (sa != sb) return sa > sb;
  if (oa != ob) return oa < ob;
  if (wa != wb) return wa < wb;
  return la < lb;
}

// block = 64 threads = one wave, blockIdx.x = recording, blockIdx.y = threshold.
__global__ __launch_bounds__(64) void stitch_events_kernel(const int32_t* __restrict__ records, const int32_t* __restrict__ win_off,
                                                           const double* __restrict__ win_start, const double* __restrict__ rec_dur,
                                                           int W, int W_stride, int R, int Q, int C, double gap, int cap,
                                                           int32_t* __restrict__ count, int32_t* __restrict__ out,
                                                           int32_t* __restrict__ status) {
  // the open merged events (all classes, unordered; class -1 = absorbed into another entry, dropped at the next compaction)
  __shared__ double o_on[SEDT_ST_OPEN], o_off[SEDT_ST_OPEN], o_pon[SEDT_ST_OPEN];       // onset, offset, onset of the providing member
  __shared__ float o_score[SEDT_ST_OPEN];
  __shared__ int o_n[SEDT_ST_OPEN], o_win[SEDT_ST_OPEN], o_q[SEDT_ST_OPEN], o_slot[SEDT_ST_OPEN], o_cls[SEDT_ST_OPEN], o_fin[SEDT_ST_OPEN];
  // the kept candidates of the window being added, in slot order
  __shared__ double c_on[SEDT_MAX_QUERIES], c_off[SEDT_MAX_QUERIES];
  __shared__ float c_score[SEDT_MAX_QUERIES];
  __shared__ int c_cls[SEDT_MAX_QUERIES], c_q[SEDT_MAX_QUERIES], c_slot[SEDT_MAX_QUERIES];
  __shared__ int s_cnt[SEDT_MAX_CLASSES + 1];

  const int r = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int32_t* cnt_out = count + ((long)kt * R + r) * C;
  int32_t* out_r = out + ((long)kt * R + r) * C * (long)cap * SEDT_EVENT_WORDS;
  if (lane <= SEDT_MAX_CLASSES) s_cnt[lane] = 0;
  const int w0 = win_off[r], w1 = win_off[r + 1];
  int st = 0;
  if (w0 < 0 || w1 < w0 || w1 > W) st = SEDT_ST_TABLE;
  if (!st) {                                                            // ascending starts: the premise of the sweep
    bool bad = false;
    for (int w = w0 + lane; w < w1; w += 64) {
      const double t = win_start[w];
      bad = bad || !(t == t) || (w > w0 && !(t >= win_start[w - 1]));
    }
    if (__ballot(bad)) st = SEDT_ST_UNORDERED;
  }
  const double dur = st ? 0.0 : rec_dur[r];
  int N = 0;                                                            // entries of the open set (wave-uniform)
  __syncthreads();

  for (int w = w0; w <= w1 && !st; ++w) {
    const bool flush = w == w1;                                         // after the last window: everything still open is final
    const double tw = flush ? 0.0 : win_start[w];

    // ---- the window's kept candidates (one lane per slot)
    int n_kept = 0;
    if (!flush) {
      const int32_t* rec = record_at(records, kt, W_stride, w, Q);
      const int n_w = rec[0];
      bool kept = false;
      double on = 0.0, off = 0.0;
      float sc = 0.f;
      int cls = -1, q = -1;
      if (n_w >= 0 && n_w <= Q && lane < n_w) {                         // a count outside 0 .. Q: the record is skipped whole
        const int32_t* s = record_slot(rec, lane);
        cls = s[SEDT_REC_CLASS];
        const double a = tw + (double)__int_as_float(s[SEDT_REC_ONSET]), b = tw + (double)__int_as_float(s[SEDT_REC_OFFSET]);
        on = a > dur ? dur : a;                                         // min(., rec_dur); a NaN stays one and fails the compare below
        off = b > dur ? dur : b;
        sc = __int_as_float(s[SEDT_REC_SCORE]);
        q = s[SEDT_REC_QUERY];
        kept = cls >= 0 && cls < C && (off - on) > 0.0 && sc == sc;
      }
      if (__ballot(kept && on < tw)) { st = SEDT_ST_EARLY; break; }
      const unsigned long long km = __ballot(kept);
      n_kept = __popcll(km);
      if (kept) {
        const int p = __popcll(km & lt);
        c_on[p] = on; c_off[p] = off; c_score[p] = sc; c_cls[p] = cls; c_q[p] = q; c_slot[p] = lane;
      }
    }

    // ---- final events: off + merge_gap < t_w.  Written at count[class] + their rank by onset among the final ones of the class
    // (merged events of one class are disjoint, so their onsets differ), then taken out of the set
    for (int i = lane; i < N; i += 64) o_fin[i] = o_cls[i] >= 0 && (flush || o_off[i] + gap < tw);
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
      if (!o_fin[i]) continue;
      const int cls = o_cls[i];
      const double on = o_on[i];
      int rank = 0;
      for (int j = 0; j < N; ++j) rank += (o_fin[j] && o_cls[j] == cls && o_on[j] < on) ? 1 : 0;
      const long pos = (long)s_cnt[cls] + rank;
      if (pos < cap) {
        int32_t* e = out_r + ((long)cls * cap + pos) * SEDT_EVENT_WORDS;
        reinterpret_cast<double*>(e)[0] = on;
        reinterpret_cast<double*>(e)[1] = o_off[i];
        e[SEDT_EVENT_SCORE] = __float_as_int(o_score[i]);
        e[SEDT_EVENT_MERGED] = o_n[i];
        e[SEDT_EVENT_WINDOW] = o_win[i];
        e[SEDT_EVENT_QUERY] = o_q[i];
      }
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64)
      if (o_fin[i]) atomicAdd(&s_cnt[o_cls[i]], 1);                      // integer LDS add: the sum does not depend on the order
    __syncthreads();
    int M = 0;                                                          // compaction, in place: chunk by chunk, order kept
    for (int base = 0; base < N; base += 64) {
      const int i = base + lane;
      const bool stay = i < N && o_cls[i] >= 0 && !o_fin[i];
      double a = 0.0, b = 0.0, c = 0.0;
      float sc = 0.f;
      int n = 0, wi = 0, q = 0, sl = 0, cl = 0;
      if (stay) { a = o_on[i]; b = o_off[i]; c = o_pon[i]; sc = o_score[i]; n = o_n[i]; wi = o_win[i]; q = o_q[i]; sl = o_slot[i]; cl = o_cls[i]; }
      const unsigned long long sm = __ballot(stay);
      __syncthreads();
      if (stay) {
        const int d = M + __popcll(sm & lt);                            // d <= i: an entry moves towards the front, inside chunks already read
        o_on[d] = a; o_off[d] = b; o_pon[d] = c; o_score[d] = sc; o_n[d] = n; o_win[d] = wi; o_q[d] = q; o_slot[d] = sl; o_cls[d] = cl;
      }
      M += __popcll(sm);
      __syncthreads();
    }
    N = M;
    if (flush) break;
    if (N + n_kept > SEDT_ST_OPEN) { st = SEDT_ST_OVERFLOW; break; }

    // ---- the candidates join the set one after the other.  A candidate and an open event of its class belong together when each
    // starts no later than the other's offset + merge_gap; the open events of a class are disjoint components, so the candidate and
    // everything it touches become one entry (the first touched, else a new one) and the others are marked absorbed.  Every value
    // below is wave-uniform but `hit`; lane 0 writes.
    const int wr = w - w0;
    for (int c = 0; c < n_kept; ++c) {
      const int cc = c_cls[c];
      double on = c_on[c], off = c_off[c], pon = on;
      float sc = c_score[c];
      int n = 1, wi = wr, q = c_q[c], sl = c_slot[c], first = -1;
      const double reach = off + gap, start = on;                       // the candidate's own: the merged entry grows, its test does not
      for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool hit = i < N && o_cls[i] == cc && start <= o_off[i] + gap && o_on[i] <= reach;
        unsigned long long hm = __ballot(hit);
        while (hm) {
          const int j = base + (int)__ffsll((long long)hm) - 1;
          hm &= hm - 1ull;
          const double jo = o_on[j], je = o_off[j], jp = o_pon[j];
          const float js = o_score[j];
          const int jw = o_win[j], jl = o_slot[j];
          on = jo < on ? jo : on;
          off = je > off ? je : off;
          n += o_n[j];
          if (st_better(js, jp, jw, jl, sc, pon, wi, sl)) { sc = js; pon = jp; wi = jw; sl = jl; q = o_q[j]; }
          if (first < 0) first = j;
          else if (lane == 0) o_cls[j] = -1;
        }
      }
      const int d = first >= 0 ? first : N;
      if (lane == 0) {
        o_on[d] = on; o_off[d] = off; o_pon[d] = pon; o_score[d] = sc; o_n[d] = n; o_win[d] = wi; o_q[d] = q; o_slot[d] = sl; o_cls[d] = cc;
      }
      if (first < 0) ++N;
      __syncthreads();
    }
  }

  // ---- counts and status.  With a status raised the lists are not to be used: their counts read 0
  __syncthreads();
  if (lane < C) cnt_out[lane] = st ? 0 : s_cnt[lane];
  if (lane == 0) status[(long)kt * R + r] = st;
}

}  // namespace sedt

extern "C" int sedt_stitch_events(const int32_t* records, const int32_t* win_off, const double* win_start, const double* rec_dur, int K,
                                  int W, int W_stride, int R, int Q, int C, double merge_gap, int cap, int32_t* count, int32_t* out,
                                  int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(Q >= 1 && Q <= SEDT_MAX_QUERIES && C >= 1 && C <= SEDT_MAX_CLASSES, "stitch_events: Q=%d (1 .. %d) C=%d (1 .. %d)", Q, SEDT_MAX_QUERIES,
               C, SEDT_MAX_CLASSES);
  SEDT_REQUIRE(K >= 1 && K <= SEDT_MAX_THRESHOLDS, "stitch_events: %d thresholds (1 .. %d)", K, SEDT_MAX_THRESHOLDS);
  SEDT_REQUIRE(R >= 0 && W >= 0 && W <= W_stride, "stitch_events: R=%d W=%d W_stride=%d (0 <= W <= W_stride)", R, W, W_stride);
  SEDT_REQUIRE(merge_gap >= 0.0 && merge_gap < INFINITY, "stitch_events: merge_gap %.17g is not a finite number >= 0", merge_gap);
  SEDT_REQUIRE(cap >= 1, "stitch_events: cap=%d (>= 1)", cap);
  SEDT_REQUIRE((double)K * R * C * cap * SEDT_EVENT_WORDS * 4.0 <= 4294967296.0, "stitch_events: an output of K=%d x R=%d x C=%d x cap=%d events "
               "is larger than 4 GiB", K, R, C, cap);
  SEDT_REQUIRE(records && win_off && win_start && rec_dur && count && out && status, "stitch_events: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "stitch_events: out is not 8-byte aligned");
  if (R == 0) return 0;
  hipLaunchKernelGGL(stitch_events_kernel, dim3(R, K), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), records, win_off, win_start,
                     rec_dur, W, W_stride, R, Q, C, merge_gap, cap, count, out, status);
  return check_launch("stitch_events");
}
