// stitch_sweep.h - ONE window of the stitch sweep ("Recordings of any length" and "Live streams"): the body of the
// window loop that stitch_events_kernel runs over all windows of a recording in one launch and stitch_stream_kernel runs once per
// launch with the open set carried in global memory between launches (both in stitch.hip).  Both kernels are built from
// stitch_sweep_step and nothing else touches the open set, so the two cannot drift apart.
//
// Defining property of the stream form.  For any stream, take the windows w = 0 .. n-1 with their (t_w, dur) and feed them one per
// launch with action 1 and a final 2 (or the last one with 3).  The concatenated emissions, grouped by class, are the count, the six
// event words and the status that sedt_stitch_events gives for the same records with win_start = t_w and rec_dur = dur, in the same
// per-class order: within a class, final events leave in onset order.  This holds because at window w the sweep needs only the open
// set - the merged events with off + merge_gap >= t_w - and everything else is already final.
//
// The step, on a set of N entries (wave-uniform) in LDS, for one wave of 64 lanes:
//   1. load      the window's kept candidates, one lane per record slot, clipped to `dur` (skipped when `flush`)
//   2. write out the entries with off + merge_gap < t_w (all of them when `flush`) are final: each is handed to `emit` with its rank
//                among the final ones - by onset inside its class (BY_CLASS false: the offline lists, one per class), or by
//                (class, onset) over all classes (BY_CLASS true: the stream's one list per launch) - and s_cnt[class] counts them
//   3. compact   final and absorbed entries leave the set, order kept
//   4. join      the candidates join the set one after the other, merging with everything of their class they touch
// Returns 0 or the status bit raised (SEDT_ST_EARLY before anything is written, SEDT_ST_OVERFLOW after steps 2 and 3).
#pragma once
#include "common.h"
#include "event_records.h"

#pragma clang fp contract(off)     // t_w + on32, off + merge_gap: the plain float64 add and compare of the definition

namespace sedt {

#define SEDT_ST_OPEN 640           // open merged events + the candidates of the window being added: (8 + 1) * 64 and a chunk to spare

#define SEDT_ST_UNORDERED 1        // status bits: window starts not ascending (or NaN)
#define SEDT_ST_OVERFLOW 2         //   more than SEDT_ST_OPEN open events + candidates at some window
#define SEDT_ST_EARLY 4            //   a kept candidate starts before its window does (a negative onset in a record)
#define SEDT_ST_TABLE 8            //   offline: win_off[r] .. win_off[r + 1] is not a range inside 0 .. W; stream: row outside 0 .. B-1

// the working set of one wave, in LDS
struct StitchSet {
  // the open merged events (all classes, unordered; class -1 = absorbed into another entry, dropped at the next compaction)
  double o_on[SEDT_ST_OPEN], o_off[SEDT_ST_OPEN], o_pon[SEDT_ST_OPEN];       // onset, offset, onset of the providing member
  float o_score[SEDT_ST_OPEN];
  int o_n[SEDT_ST_OPEN], o_win[SEDT_ST_OPEN], o_q[SEDT_ST_OPEN], o_slot[SEDT_ST_OPEN], o_cls[SEDT_ST_OPEN], o_fin[SEDT_ST_OPEN];
  // the kept candidates of the window being added, in slot order
  double c_on[SEDT_MAX_QUERIES], c_off[SEDT_MAX_QUERIES];
  float c_score[SEDT_MAX_QUERIES];
  int c_cls[SEDT_MAX_QUERIES], c_q[SEDT_MAX_QUERIES], c_slot[SEDT_MAX_QUERIES];
  int s_cnt[SEDT_MAX_CLASSES + 1];                                           // final events per class so far
};

// the member of a merged event that gives score, window and query: the highest score; among equal scores the first in (on, w, s)
__device__ __forceinline__ bool st_better(float sa, double oa, int wa, int la, float sb, double ob, int wb, int lb) {
  if (sa != sb) return sa > sb;
  if (oa != ob) return oa < ob;
  if (wa != wb) return wa < wb;
  return la < lb;
}

// rec: the window's record (unused when flush); tw, dur: its start and the duration to clip against; wr: the window word of its
// events; emit(i, cls, on, rank): entry i of the set is final.  All arguments but `lane` are wave-uniform.
template <bool BY_CLASS, typename Emit>
__device__ __forceinline__ int stitch_sweep_step(StitchSet& S, int& N, bool flush, const int32_t* rec, double tw, double dur, int wr, int Q,
                                                 int C, double gap, int lane, Emit emit) {
  const unsigned long long lt = (1ull << lane) - 1ull;

  // ---- the window's kept candidates (one lane per slot)
  int n_kept = 0;
  if (!flush) {
    const int n_w = rec[0];
    bool kept = false;
    double on = 0.0, off = 0.0;
    float sc = 0.f;
    int cls = -1, q = -1;
    if (n_w >= 0 && n_w <= Q && lane < n_w) {                         // a count outside 0 .. Q: the record is skipped whole
      const int32_t* s = record_slot(rec, lane);
      cls = s[SEDT_REC_CLASS];
      const double a = tw + (double)__int_as_float(s[SEDT_REC_ONSET]), b = tw + (double)__int_as_float(s[SEDT_REC_OFFSET]);
      on = a > dur ? dur : a;                                         // min(., dur); a NaN stays one and fails the compare below
      off = b > dur ? dur : b;
      sc = __int_as_float(s[SEDT_REC_SCORE]);
      q = s[SEDT_REC_QUERY];
      kept = cls >= 0 && cls < C && (off - on) > 0.0 && sc == sc;
    }
    if (__ballot(kept && on < tw)) return SEDT_ST_EARLY;
    const unsigned long long km = __ballot(kept);
    n_kept = __popcll(km);
    if (kept) {
      const int p = __popcll(km & lt);
      S.c_on[p] = on; S.c_off[p] = off; S.c_score[p] = sc; S.c_cls[p] = cls; S.c_q[p] = q; S.c_slot[p] = lane;
    }
  }

  // ---- final events: off + merge_gap < t_w.  Handed out with their rank by onset among the final ones of the class (merged events
  // of one class are disjoint, so their onsets differ) - BY_CLASS: behind the final ones of the classes below -, then taken out
  for (int i = lane; i < N; i += 64) S.o_fin[i] = S.o_cls[i] >= 0 && (flush || S.o_off[i] + gap < tw);
  __syncthreads();
  for (int i = lane; i < N; i += 64) {
    if (!S.o_fin[i]) continue;
    const int cls = S.o_cls[i];
    const double on = S.o_on[i];
    int rank = 0;
    for (int j = 0; j < N; ++j)
      rank += (S.o_fin[j] && (S.o_cls[j] == cls ? S.o_on[j] < on : (BY_CLASS && S.o_cls[j] < cls))) ? 1 : 0;
    emit(i, cls, on, rank);
  }
  __syncthreads();
  for (int i = lane; i < N; i += 64)
    if (S.o_fin[i]) atomicAdd(&S.s_cnt[S.o_cls[i]], 1);                // integer LDS add: the sum does not depend on the order
  __syncthreads();
  int M = 0;                                                          // compaction, in place: chunk by chunk, order kept
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    const bool stay = i < N && S.o_cls[i] >= 0 && !S.o_fin[i];
    double a = 0.0, b = 0.0, c = 0.0;
    float sc = 0.f;
    int n = 0, wi = 0, q = 0, sl = 0, cl = 0;
    if (stay) {
      a = S.o_on[i]; b = S.o_off[i]; c = S.o_pon[i]; sc = S.o_score[i]; n = S.o_n[i]; wi = S.o_win[i]; q = S.o_q[i]; sl = S.o_slot[i];
      cl = S.o_cls[i];
    }
    const unsigned long long sm = __ballot(stay);
    __syncthreads();
    if (stay) {
      const int d = M + __popcll(sm & lt);                            // d <= i: an entry moves towards the front, inside chunks already read
      S.o_on[d] = a; S.o_off[d] = b; S.o_pon[d] = c; S.o_score[d] = sc; S.o_n[d] = n; S.o_win[d] = wi; S.o_q[d] = q; S.o_slot[d] = sl;
      S.o_cls[d] = cl;
    }
    M += __popcll(sm);
    __syncthreads();
  }
  N = M;
  if (flush) return 0;
  if (N + n_kept > SEDT_ST_OPEN) return SEDT_ST_OVERFLOW;

  // ---- the candidates join the set one after the other.  A candidate and an open event of its class belong together when each
  // starts no later than the other's offset + merge_gap; the open events of a class are disjoint components, so the candidate and
  // everything it touches become one entry (the first touched, else a new one) and the others are marked absorbed.  Every value
  // below is wave-uniform but `hit`; lane 0 writes.
  for (int c = 0; c < n_kept; ++c) {
    const int cc = S.c_cls[c];
    double on = S.c_on[c], off = S.c_off[c], pon = on;
    float sc = S.c_score[c];
    int n = 1, wi = wr, q = S.c_q[c], sl = S.c_slot[c], first = -1;
    const double reach = off + gap, start = on;                       // the candidate's own: the merged entry grows, its test does not
    for (int base = 0; base < N; base += 64) {
      const int i = base + lane;
      const bool hit = i < N && S.o_cls[i] == cc && start <= S.o_off[i] + gap && S.o_on[i] <= reach;
      unsigned long long hm = __ballot(hit);
      while (hm) {
        const int j = base + (int)__ffsll((long long)hm) - 1;
        hm &= hm - 1ull;
        const double jo = S.o_on[j], je = S.o_off[j], jp = S.o_pon[j];
        const float js = S.o_score[j];
        const int jw = S.o_win[j], jl = S.o_slot[j];
        on = jo < on ? jo : on;
        off = je > off ? je : off;
        n += S.o_n[j];
        if (st_better(js, jp, jw, jl, sc, pon, wi, sl)) { sc = js; pon = jp; wi = jw; sl = jl; q = S.o_q[j]; }
        if (first < 0) first = j;
        else if (lane == 0) S.o_cls[j] = -1;
      }
    }
    const int d = first >= 0 ? first : N;
    if (lane == 0) {
      S.o_on[d] = on; S.o_off[d] = off; S.o_pon[d] = pon; S.o_score[d] = sc; S.o_n[d] = n; S.o_win[d] = wi; S.o_q[d] = q; S.o_slot[d] = sl;
      S.o_cls[d] = cc;
    }
    if (first < 0) ++N;
    __syncthreads();
  }
  return 0;
}

}  // namespace sedt
