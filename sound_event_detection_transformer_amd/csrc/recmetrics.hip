// recmetrics.hip - recordings of any length scored against their annotations: the stitched event lists of stitch_events_kernel
// (stitch.hip) are read where they lie, per (threshold, recording, class), and counted - lists in, counts out
//   * recording_event_counts_kernel     ev [K][C][3] += {tp, n_ref, n_sys}, tag [K][C][3] += {tp, fp, fn}   one wave per (rec., class, thr.)
//   * recording_segment_counts_kernel   seg [K][C][3] += {tp, n_ref, n_sys}, sdi [K][3] += {S, D, I}        one wave per (rec., threshold)
// The reference scores 10 s dataset clips only and has no counterpart; DESIGN.md section 4 ("Scoring recordings") holds the
// definition and tests/recording_metrics_ref.py restates it in NumPy.
//
// Scope: per fusion strategy, threshold k, recording r, class c.  Float64, plain subtract / multiply / divide / compare, no contraction.
//   estimates   the first count[k][r][c] slots of the stitch output out[k][r][c] (onset = the f64 in words 0-1, offset = the f64 in
//               words 2-3), as stitch wrote them: no second clip, no duration filter; ascending by onset and disjoint.
//   references  the recording's annotated events of class c, sorted by the host by (onset, offset, input order); any number of them,
//               and those of one class may overlap.
//   evaluated   only recordings with an entry in the reference: rec_idx[r] = -1 (or outside the table) adds nothing anywhere.  A
//               recording annotated with an empty list is evaluated: its estimates count as n_sys, as false positives and as I.
//   event-based a hit is |on_r - on_e| <= t_collar and |off_r - off_e| <= max(t_collar, pct * (off_r - on_r)) (event_hit_graph);
//               tp = the size of a maximum-cardinality matching of the hit graph of class c over the WHOLE recording, or
//               (optimal == 0) of sed_eval's greedy pass: references in table order, each takes the first estimate in onset order
//               that is still free and that it hits.
//   no limit    a hit needs onsets within t_collar, so the two lists are merged by onset and a BLOCK is closed between two consecutive
//               items a <= b of the merged order with fl(b - a) > t_collar.  No hit crosses such a cut: for p <= a < b <= q the
//               real difference q - p >= b - a, rounding is monotone, so fl(q - p) >= fl(b - a) > t_collar.  The matching (maximum, or
//               greedy in the orders above) is the sum over the blocks.  Blocks are formed while both lists have items left: what
//               remains of one list behind the last block matches nothing and is not walked.  A block holds at most 64 references
//               and 64 estimates (event_match.h); a denser one raises status 2, it is never silently mis-counted.
//   presence    per class "count[k][r][c] > 0" against "class c has a reference event in r": {tp, fp, fn}.
//   segments    at time_resolution rho an event makes its class active in the segments floor(on / rho) <= s < ceil(off / rho), both
//               quotients float64 divisions; events of a class OR together.  Class-wise {tp, n_ref, n_sys}; per segment over the
//               classes S += min(Nref, Nsys) - Ntp, D += max(0, Nref - Nsys), I += max(0, Nsys - Nref).  The recording spans
//               n_words[r] words of 64 segments (the host: ceil(ceil(max(rec_dur[r], largest reference offset) / rho) / 64)); the sweep
//               holds two words per class, whatever the number of segments.
//   status      [K][R] int32 per launch: 0; 1 the stitch status of (k, r) is non-zero or some count[k][r][c] > cap (the lists are not
//               complete); 4 a list is not ascending by onset or holds a non-finite time; 2 a block over capacity - in this order
//               of precedence.  With a status raised the counters may hold partial sums of that recording.
// count is clamped to 0 .. cap before it indexes anything, a rec_idx outside the table is skipped, the CSR offsets are clamped to the
// table: nothing is read or written out of bounds.  Counters are int64, integer atomics only: results do not depend on launch order.
#include <cmath>

#include "common.h"
#include "event_match.h"
#include "recording_lists.h"

#pragma clang fp contract(off)     // on_b - on_a > t_collar, on / rho: the plain float64 operations of the definition

namespace sedt {

#define SEDT_RM_MAXWORDS ((1 << 25) - 1)   // 64-segment words of one recording: segment indices stay inside int32

// block = 64 threads = one wave, blockIdx.x = recording * C + class, blockIdx.y = threshold; ev / tag: this fusion strategy's [K][C][3];
// status [K][R] zeroed before the launch (the classes of a recording raise it with an integer max: 4 before 2)
__global__ __launch_bounds__(64) void recording_event_counts_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ out,
                                                                    const int32_t* __restrict__ stitch_status,
                                                                    const int32_t* __restrict__ rec_idx, const int32_t* __restrict__ ref_off,
                                                                    const double* __restrict__ ref_on, const double* __restrict__ ref_end,
                                                                    int N, int E, int R, int C, int cap, double t_collar, double pct,
                                                                    int optimal, unsigned long long* __restrict__ ev,
                                                                    unsigned long long* __restrict__ tag, int32_t* __restrict__ status) {
  __shared__ double e_on[SEDT_MAX_QUERIES + 1], e_end[SEDT_MAX_QUERIES];      // the next 64 estimates and the onset of the one behind them
  __shared__ double r_on[SEDT_MAX_REF_EVENTS + 1], r_end[SEDT_MAX_REF_EVENTS];      // the next 64 references and the onset of the one behind them
  __shared__ int r_cls[SEDT_MAX_REF_EVENTS];
  __shared__ unsigned long long adj[SEDT_MAX_REF_EVENTS];
  __shared__ int match_est[SEDT_MAX_QUERIES], from_ref[SEDT_MAX_QUERIES], match_ref[SEDT_MAX_REF_EVENTS];
  __shared__ unsigned char queue[SEDT_MAX_REF_EVENTS];

  const int r = blockIdx.x / C, c = blockIdx.x % C, kt = blockIdx.y, lane = threadIdx.x;
  const int ri = rec_idx[r];
  if (ri < 0 || ri >= N) return;                                      // not in the reference: adds nothing anywhere
  const long kr = (long)kt * R + r;
  const int32_t* cnt = count + kr * C;
  if (rm_incomplete(stitch_status, cnt, kr, C, cap, lane)) {
    if (lane == 0 && c == 0) status[kr] = SEDT_RM_INCOMPLETE;          // every class of (k, r) sees it and counts nothing
    return;
  }
  const int n_est = min(max(cnt[c], 0), cap);
  const double* est = reinterpret_cast<const double*>(out + (kr * C + c) * (long)cap * SEDT_EVENT_WORDS);
  int j0, j1;
  rm_ref_range(ref_off, ri, C, c, E, j0, j1);
  if (!rm_lists_ok(est, n_est, ref_on, ref_end, j0, j1, lane)) {
    if (lane == 0) atomicMax(&status[kr], SEDT_RM_UNORDERED);
    return;
  }
  r_cls[lane] = c;

  long tp = 0;                                                        // lane 0's
  int ie = 0, ir = j0, st = 0;
  while (ie < n_est && ir < j1) {                                     // a list at its end: what is left of the other matches nothing
    // ---- stage the next 65 onsets of both lists
    const int we = min(n_est - ie, SEDT_MAX_QUERIES + 1), wr = min(j1 - ir, SEDT_MAX_REF_EVENTS + 1);
    __syncthreads();
    for (int i = lane; i < we; i += 64) {
      e_on[i] = est[SEDT_EVENT_DOUBLES * (long)(ie + i)];
      if (i < SEDT_MAX_QUERIES) e_end[i] = est[SEDT_EVENT_DOUBLES * (long)(ie + i) + 1];
    }
    for (int i = lane; i < wr; i += 64) {
      r_on[i] = ref_on[ir + i];
      if (i < SEDT_MAX_REF_EVENTS) r_end[i] = ref_end[ir + i];
    }
    match_est[lane] = -1;
    match_ref[lane] = -1;
    __syncthreads();
    // ---- the block: items of the merged order until the first onset step above t_collar (every value is wave-uniform)
    int a = 0, b = 0;
    double last = 0.0;
    for (;;) {
      const bool he = a < we, hr = b < wr;
      if (!he && !hr) break;
      const double oe = he ? e_on[a] : 0.0, orf = hr ? r_on[b] : 0.0;
      const bool take_e = he && (!hr || oe <= orf);
      const double x = take_e ? oe : orf;
      if (a + b > 0 && (x - last) > t_collar) break;
      if ((take_e ? a : b) == SEDT_MAX_QUERIES) { st = SEDT_RM_BLOCK; break; }   // a 65th estimate or reference inside one block
      a += take_e ? 1 : 0;
      b += take_e ? 0 : 1;
      last = x;
    }
    if (st) break;
    if (a > 0 && b > 0) {
      event_hit_graph(adj, r_cls, r_on, r_end, b, lane < a, c, lane < a ? e_on[lane] : 0.0, lane < a ? e_end[lane] : 0.0, t_collar, pct,
                      lane);
      __syncthreads();
      if (lane == 0) {
        long n_ref = 0;
        tp += event_class_match(c, b, r_cls, adj, match_est, from_ref, match_ref, queue, optimal, nullptr, 0, n_ref);
      }
    }
    ie += a;
    ir += b;
  }
  if (st) {
    if (lane == 0) atomicMax(&status[kr], st);
    return;
  }
  if (lane == 0) {
    const long n_ref = j1 - j0, n_sys = n_est;
    const long cell = ((long)kt * C + c) * 3;
    add_counts3(ev + cell, tp, n_ref, n_sys);
    add_presence(tag + cell, n_ref > 0, cnt[c] > 0);
  }
}

// segment index of a float64 quotient already floored / ceiled, inside 0 .. S
__device__ __forceinline__ int rm_seg(double q, int S) { return q < 0.0 ? 0 : (q > (double)S ? S : (int)q); }

// one list of one class in the word sweep: the cursor, and the largest end segment of the events already passed (events of one
// class may overlap, so an earlier one can still cover the current word)
struct RmCursor {
  const double* on;                // onset of event i at on[i * stride], offset at end[i * stride]
  const double* end;
  int stride, i, n, reach;
};

// bits of the segments lo .. lo + 63 the list covers; advances the cursor past every event that starts before lo + 64
__device__ __forceinline__ unsigned long long rm_word(RmCursor& u, int lo, double rho, int S) {
  const int hi = lo + 64;
  unsigned long long m = 0ull;
  if (u.reach > lo) m = u.reach >= hi ? ~0ull : (1ull << (u.reach - lo)) - 1ull;
  while (u.i < u.n) {
    const int s0 = rm_seg(floor(u.on[(long)u.i * u.stride] / rho), S);
    if (s0 >= hi) break;
    const int s1 = rm_seg(ceil(u.end[(long)u.i * u.stride] / rho), S);
    ++u.i;
    if (s1 <= s0) continue;                                           // an empty range sets nothing
    u.reach = max(u.reach, s1);
    if (s1 <= lo) continue;
    const int b0 = max(s0, lo) - lo, b1 = min(s1, hi) - lo;           // 0 <= b0 < b1 <= 64
    m |= (b1 >= 64 ? ~0ull : (1ull << b1) - 1ull) & ~((1ull << b0) - 1ull);
  }
  return m;
}

// the first segment at or after lo in which the list can be active again, S when there is none
__device__ __forceinline__ int rm_next(const RmCursor& u, int lo, double rho, int S) {
  if (u.reach > lo) return lo;
  return u.i < u.n ? rm_seg(floor(u.on[(long)u.i * u.stride] / rho), S) : S;
}

// block = 64 threads = one wave, blockIdx.x = recording, blockIdx.y = threshold, lane = class; seg [K][C][3] / sdi [K][3]: this
// fusion strategy's
__global__ __launch_bounds__(64) void recording_segment_counts_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ out,
                                                                      const int32_t* __restrict__ stitch_status,
                                                                      const int32_t* __restrict__ rec_idx,
                                                                      const int32_t* __restrict__ ref_off, const double* __restrict__ ref_on,
                                                                      const double* __restrict__ ref_end, const int32_t* __restrict__ n_words,
                                                                      int N, int E, int R, int C, int cap, double rho,
                                                                      unsigned long long* __restrict__ seg, unsigned long long* __restrict__ sdi,
                                                                      int32_t* __restrict__ status) {
  __shared__ unsigned long long w_est[64], w_ref[64];                 // the current 64 segments of every class
  const int r = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  const long kr = (long)kt * R + r;
  const int ri = rec_idx[r];
  if (ri < 0 || ri >= N) {
    if (lane == 0) status[kr] = 0;
    return;
  }
  const int32_t* cnt = count + kr * C;
  int st = rm_incomplete(stitch_status, cnt, kr, C, cap, lane) ? SEDT_RM_INCOMPLETE : 0;
  for (int c = 0; c < C && !st; ++c) {                                // the premise of the cursors, checked by the whole wave
    int j0, j1;
    rm_ref_range(ref_off, ri, C, c, E, j0, j1);
    const double* est = reinterpret_cast<const double*>(out + (kr * C + c) * (long)cap * SEDT_EVENT_WORDS);
    if (!rm_lists_ok(est, min(max(cnt[c], 0), cap), ref_on, ref_end, j0, j1, lane)) st = SEDT_RM_UNORDERED;
  }
  if (st) {
    if (lane == 0) status[kr] = st;
    return;
  }
  const int nw = min(max(n_words[r], 0), SEDT_RM_MAXWORDS), S = nw * 64;
  RmCursor ue = {nullptr, nullptr, SEDT_EVENT_DOUBLES, 0, 0, 0}, ur = {nullptr, nullptr, 1, 0, 0, 0};
  if (lane < C) {
    int j0, j1;
    rm_ref_range(ref_off, ri, C, lane, E, j0, j1);
    const double* est = reinterpret_cast<const double*>(out + (kr * C + lane) * (long)cap * SEDT_EVENT_WORDS);
    ue.on = est; ue.end = est + 1; ue.n = min(max(cnt[lane], 0), cap);
    ur.on = ref_on + j0; ur.end = ref_end + j0; ur.n = j1 - j0;
  }
  long c_tp = 0, c_ref = 0, c_sys = 0;                                // lane = class
  long n_s = 0, n_d = 0, n_i = 0;                                     // lane = segment of the word
  for (int w = 0; w < nw;) {
    const int lo = w * 64;
    const unsigned long long me = rm_word(ue, lo, rho, S), mr = rm_word(ur, lo, rho, S);
    if (__ballot((me | mr) != 0ull) == 0ull) {                        // nothing active: on to the word of the next event
      int nxt = min(rm_next(ue, lo + 64, rho, S), rm_next(ur, lo + 64, rho, S));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) nxt = min(nxt, __shfl_xor(nxt, o, 64));
      w = max(w + 1, nxt / 64);
      continue;
    }
    c_tp += __popcll(me & mr);
    c_ref += __popcll(mr);
    c_sys += __popcll(me);
    __syncthreads();
    w_est[lane] = me;
    w_ref[lane] = mr;
    __syncthreads();
    int s_tp = 0, s_ref = 0, s_sys = 0;                               // lane = segment lo + lane: the classes active in it
    for (int c = 0; c < C; ++c) {
      const int be = (int)((w_est[c] >> lane) & 1ull), br = (int)((w_ref[c] >> lane) & 1ull);
      s_tp += be & br;
      s_ref += br;
      s_sys += be;
    }
    n_s += min(s_ref, s_sys) - s_tp;
    n_d += max(0, s_ref - s_sys);
    n_i += max(0, s_sys - s_ref);
    ++w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_s += __shfl_xor(n_s, o, 64);
    n_d += __shfl_xor(n_d, o, 64);
    n_i += __shfl_xor(n_i, o, 64);
  }
  if (lane < C) add_counts3(seg + ((long)kt * C + lane) * 3, c_tp, c_ref, c_sys);
  if (lane == 0) {
    add_counts3(sdi + (long)kt * 3, n_s, n_d, n_i);
    status[kr] = 0;
  }
}

}  // namespace sedt

extern "C" int sedt_recording_event_counts(const int32_t* count, const int32_t* out, const int32_t* stitch_status, const int32_t* rec_idx,
                                           const int32_t* ref_off, const double* ref_on, const double* ref_end, int n_ref_rec,
                                           int n_ref_events, int K, int R, int C, int cap, int n_fusion, int fusion, double t_collar,
                                           double pct, int optimal, int64_t* ev_counts, int64_t* tag_counts, int32_t* status, void* stream) {
  using namespace sedt;
  if (recording_args_ok("recording_event_counts", count, out, stitch_status, rec_idx, ref_off, ref_on, ref_end, n_ref_rec, n_ref_events, K,
                        R, C, cap, n_fusion, fusion, status))
    return 1;
  SEDT_REQUIRE(t_collar >= 0.0 && t_collar < INFINITY && pct == pct, "recording_event_counts: t_collar %.17g is not a finite number >= 0 "
               "(or percentage_of_length is NaN)", t_collar);
  if (R == 0) return 0;
  SEDT_REQUIRE(ev_counts && tag_counts, "recording_event_counts: null pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)K * R, s) != hipSuccess) return check_launch("recording_event_counts (status)");
  const long mine = (long)fusion * K * C * 3;
  hipLaunchKernelGGL(recording_event_counts_kernel, dim3((unsigned)(R * C), K), dim3(64), 0, s, count, out, stitch_status, rec_idx, ref_off,
                     ref_on, ref_end, n_ref_rec, n_ref_events, R, C, cap, t_collar, pct, optimal,
                     reinterpret_cast<unsigned long long*>(ev_counts) + mine, reinterpret_cast<unsigned long long*>(tag_counts) + mine, status);
  return check_launch("recording_event_counts");
}

extern "C" int sedt_recording_segment_counts(const int32_t* count, const int32_t* out, const int32_t* stitch_status, const int32_t* rec_idx,
                                             const int32_t* ref_off, const double* ref_on, const double* ref_end, const int32_t* n_words,
                                             int n_ref_rec, int n_ref_events, int K, int R, int C, int cap, int n_fusion, int fusion,
                                             double time_resolution, int64_t* seg_counts, int64_t* sdi_counts, int32_t* status,
                                             void* stream) {
  using namespace sedt;
  if (recording_args_ok("recording_segment_counts", count, out, stitch_status, rec_idx, ref_off, ref_on, ref_end, n_ref_rec, n_ref_events,
                        K, R, C, cap, n_fusion, fusion, status))
    return 1;
  SEDT_REQUIRE(time_resolution > 0.0 && time_resolution < INFINITY, "recording_segment_counts: time_resolution %.17g is not a positive "
               "number of seconds", time_resolution);
  if (R == 0) return 0;
  SEDT_REQUIRE(n_words && seg_counts && sdi_counts, "recording_segment_counts: null pointer");
  hipLaunchKernelGGL(recording_segment_counts_kernel, dim3(R, K), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), count, out,
                     stitch_status, rec_idx, ref_off, ref_on, ref_end, n_words, n_ref_rec, n_ref_events, R, C, cap, time_resolution,
                     reinterpret_cast<unsigned long long*>(seg_counts) + (long)fusion * K * C * 3,
                     reinterpret_cast<unsigned long long*>(sdi_counts) + (long)fusion * K * 3, status);
  return check_launch("recording_segment_counts");
}
