// stitch.hip - recordings of any length: the event records of a recording's overlapping windows (decode_events_kernel, decode.hip)
// merged into one event list per (threshold, recording, class)
//   * stitch_events_kernel   an event a window boundary cut in two, or one that two overlapping windows both report, becomes one event
//   * stitch_stream_kernel   the same sweep one window per launch for S live streams, the open set kept in global memory between launches
//   * stream_reset_kernel    chosen streams start again at time 0
// The reference scores 10 s dataset clips only and has no counterpart; DESIGN.md section 4 ("Recordings of any length", "Live
// streams") holds the definition and tests/recording_ref.py / tests/stream_ref.py restate it in NumPy.
// One wave per (recording, threshold) sweeps the recording's windows in start order with the OPEN merged events in LDS.  An event of
// window w cannot start before t_w, so a merged event with off + merge_gap < t_w can gain no member once window w is reached: it is
// written out and leaves the set.  What stays open at window w comes from the few earlier windows that still reach t_w (D of them,
// D <= 8 by the Python side's plan check), at most D * Q events of all classes together - a recording of any number of windows runs
// in the same 36 KB of LDS.  Float64 adds and compares on the records' f32 values widened; plain stores, integer LDS operations only:
// the result does not depend on launch order and two launches give the same bytes.
// The body of the window loop is stitch_sweep_step (stitch_sweep.h); both kernels are built from it.
#include <cmath>

#include "common.h"
#include "event_records.h"
#include "stitch_sweep.h"

#pragma clang fp contract(off)     // t_w + on32, off + merge_gap: the plain float64 add and compare of the definition

namespace sedt {

// block = 64 threads = one wave, blockIdx.x = recording, blockIdx.y = threshold.
__global__ __launch_bounds__(64) void stitch_events_kernel(const int32_t* __restrict__ records, const int32_t* __restrict__ win_off,
                                                           const double* __restrict__ win_start, const double* __restrict__ rec_dur,
                                                           int W, int W_stride, int R, int Q, int C, double gap, int cap,
                                                           int32_t* __restrict__ count, int32_t* __restrict__ out,
                                                           int32_t* __restrict__ status) {
  __shared__ StitchSet S;

  const int r = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  int32_t* cnt_out = count + ((long)kt * R + r) * C;
  int32_t* out_r = out + ((long)kt * R + r) * C * (long)cap * SEDT_EVENT_WORDS;
  if (lane <= SEDT_MAX_CLASSES) S.s_cnt[lane] = 0;
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

  // a final event is written at count[class] + its rank by onset among the final ones of the class
  auto emit = [&](int i, int cls, double on, int rank) {
    const long pos = (long)S.s_cnt[cls] + rank;
    if (pos < cap) {
      int32_t* e = out_r + ((long)cls * cap + pos) * SEDT_EVENT_WORDS;
      reinterpret_cast<double*>(e)[0] = on;
      reinterpret_cast<double*>(e)[1] = S.o_off[i];
      e[SEDT_EVENT_SCORE] = __float_as_int(S.o_score[i]);
      e[SEDT_EVENT_MERGED] = S.o_n[i];
      e[SEDT_EVENT_WINDOW] = S.o_win[i];
      e[SEDT_EVENT_QUERY] = S.o_q[i];
    }
  };
  for (int w = w0; w <= w1 && !st; ++w) {
    const bool flush = w == w1;                                         // after the last window: everything still open is final
    st = stitch_sweep_step<false>(S, N, flush, flush ? records : record_at(records, kt, W_stride, w, Q), flush ? 0.0 : win_start[w], dur,
                                  w - w0, Q, C, gap, lane, emit);
  }

  // ---- counts and status.  With a status raised the lists are not to be used: their counts read 0
  __syncthreads();
  if (lane < C) cnt_out[lane] = st ? 0 : S.s_cnt[lane];
  if (lane == 0) status[(long)kt * R + r] = st;
}

// ---- live streams.  The state of one (threshold, stream), SEDT_SS_WORDS 32-bit words in global memory, 8-byte aligned:
//   header  {N, status, windows_seen, pad, last t_w (f64, words 4-5), count[c] at word SEDT_SS_COUNT + c: the events of class c emitted so far}
//   fields  of the SEDT_ST_OPEN entries of the open set, array by array in StitchSet's order (o_fin is scratch and not kept)
// All zeros is a fresh stream.  Only the first N entries of every array are read and written.
#define SEDT_SS_COUNT 6
#define SEDT_SS_HDR 72
#define SEDT_SS_WORDS (SEDT_SS_HDR + 12 * SEDT_ST_OPEN)
#define SEDT_EMIT_WORDS 10         // {onset f64, offset f64, score f32, n_merged, window, query, class, pad}
enum { SEDT_EMIT_CLASS = 8, SEDT_EMIT_PAD };

__device__ __forceinline__ int wave_sum(int v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// block = 64 threads = one wave, blockIdx.x = stream, blockIdx.y = threshold.
__global__ __launch_bounds__(64) void stitch_stream_kernel(const int32_t* __restrict__ records, const int32_t* __restrict__ action,
                                                           const int32_t* __restrict__ row, const double* __restrict__ t_w,
                                                           const double* __restrict__ dur, const int32_t* __restrict__ win_index,
                                                           int NS, int B, int Q, int C, double gap, int emit_cap,
                                                           int32_t* __restrict__ state, int32_t* __restrict__ emit,
                                                           int32_t* __restrict__ emit_count, int32_t* __restrict__ status) {
  __shared__ StitchSet S;

  const int s = blockIdx.x, kt = blockIdx.y, lane = threadIdx.x;
  const int act = action[s];
  if (act < 1 || act > 3) return;                                       // 0: this stream has no window in this launch
  const long ks = (long)kt * NS + s;
  int32_t* hdr = state + ks * SEDT_SS_WORDS;
  int st = hdr[1];
  if (st) {                                                             // sticky: the stream emits nothing more, its status is reported
    if (lane == 0) status[ks] = st;
    return;
  }
  int N = hdr[0];
  N = N < 0 ? 0 : (N > SEDT_ST_OPEN ? SEDT_ST_OPEN : N);
  const int seen = hdr[2];
  const double last = reinterpret_cast<const double*>(hdr)[2];
  double* g_on = reinterpret_cast<double*>(hdr + SEDT_SS_HDR);
  double* g_off = g_on + SEDT_ST_OPEN;
  double* g_pon = g_off + SEDT_ST_OPEN;
  int32_t* g_score = reinterpret_cast<int32_t*>(g_pon + SEDT_ST_OPEN);
  int32_t *g_n = g_score + SEDT_ST_OPEN, *g_win = g_n + SEDT_ST_OPEN, *g_q = g_win + SEDT_ST_OPEN, *g_slot = g_q + SEDT_ST_OPEN,
          *g_cls = g_slot + SEDT_ST_OPEN;
  if (lane <= SEDT_MAX_CLASSES) S.s_cnt[lane] = lane < C ? hdr[SEDT_SS_COUNT + lane] : 0;
  for (int i = lane; i < N; i += 64) {
    S.o_on[i] = g_on[i]; S.o_off[i] = g_off[i]; S.o_pon[i] = g_pon[i]; S.o_score[i] = __int_as_float(g_score[i]); S.o_n[i] = g_n[i];
    S.o_win[i] = g_win[i]; S.o_q[i] = g_q[i]; S.o_slot[i] = g_slot[i]; S.o_cls[i] = g_cls[i];
  }
  __syncthreads();
  const int cnt0 = lane < C ? S.s_cnt[lane] : 0;
  const int e0 = emit_count[ks];
  int32_t* emit_s = emit + ks * (long)emit_cap * SEDT_EMIT_WORDS;
  int base = e0;                                                        // where this step's final events go: rank by (class, onset) behind it

  auto out = [&](int i, int cls, double on, int rank) {
    const long pos = (long)base + rank;
    if (pos >= 0 && pos < emit_cap) {
      int32_t* e = emit_s + pos * SEDT_EMIT_WORDS;
      reinterpret_cast<double*>(e)[0] = on;
      reinterpret_cast<double*>(e)[1] = S.o_off[i];
      e[SEDT_EVENT_SCORE] = __float_as_int(S.o_score[i]);
      e[SEDT_EVENT_MERGED] = S.o_n[i];
      e[SEDT_EVENT_WINDOW] = S.o_win[i];
      e[SEDT_EVENT_QUERY] = S.o_q[i];
      e[SEDT_EMIT_CLASS] = cls;
      e[SEDT_EMIT_PAD] = 0;
    }
  };
  const double tw = (act & 1) ? t_w[s] : 0.0;
  if (act & 1) {
    const int r = row[s];
    if (r < 0 || r >= B) st = SEDT_ST_TABLE;
    else if (!(tw == tw) || (seen > 0 && !(tw >= last))) st = SEDT_ST_UNORDERED;
    else st = stitch_sweep_step<true>(S, N, false, record_at(records, kt, B, r, Q), tw, dur[s], win_index[s], Q, C, gap, lane, out);
  }
  if (!st && (act & 2)) {
    __syncthreads();
    base = e0 + wave_sum(lane < C ? S.s_cnt[lane] - cnt0 : 0);          // behind what the window's own step wrote (action 3)
    stitch_sweep_step<true>(S, N, true, records, 0.0, 0.0, 0, Q, C, gap, lane, out);
  }

  __syncthreads();
  if (st) {                                                             // raised now: the state stays as it was but for the status word,
    if (lane == 0) { hdr[1] = st; status[ks] = st; }                    // emit_count does not move (slots behind it may have been written)
    return;
  }
  const int total = wave_sum(lane < C ? S.s_cnt[lane] - cnt0 : 0);
  if (lane < C) hdr[SEDT_SS_COUNT + lane] = S.s_cnt[lane];
  for (int i = lane; i < N; i += 64) {
    g_on[i] = S.o_on[i]; g_off[i] = S.o_off[i]; g_pon[i] = S.o_pon[i]; g_score[i] = __float_as_int(S.o_score[i]); g_n[i] = S.o_n[i];
    g_win[i] = S.o_win[i]; g_q[i] = S.o_q[i]; g_slot[i] = S.o_slot[i]; g_cls[i] = S.o_cls[i];
  }
  if (lane == 0) {
    hdr[0] = N;
    if (act & 1) {
      hdr[2] = seen + 1;
      reinterpret_cast<double*>(hdr)[2] = tw;
    }
    emit_count[ks] = e0 + total;
    status[ks] = 0;
  }
}

// one thread per header word of (threshold, stream): the chosen streams' headers and status words read zero afterwards
__global__ void stream_reset_kernel(int32_t* __restrict__ state, const int32_t* __restrict__ which, long n, int NS,
                                    int32_t* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long ks = i / SEDT_SS_HDR;
  const int word = (int)(i - ks * SEDT_SS_HDR);
  if (which && !which[ks % NS]) return;
  state[ks * SEDT_SS_WORDS + word] = 0;
  if (word == 0) status[ks] = 0;
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

extern "C" int64_t sedt_stitch_stream_state_bytes(int K, int S) {
  return (int64_t)(K > 0 ? K : 0) * (S > 0 ? S : 0) * SEDT_SS_WORDS * 4;
}

extern "C" int sedt_stitch_stream(const int32_t* records, const int32_t* action, const int32_t* row, const double* t_w, const double* dur,
                                  const int32_t* win_index, int K, int S, int B, int Q, int C, double merge_gap, int emit_cap,
                                  int32_t* state, int64_t state_bytes, int32_t* emit, int32_t* emit_count, int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(Q >= 1 && Q <= SEDT_MAX_QUERIES && C >= 1 && C <= SEDT_MAX_CLASSES, "stitch_stream: Q=%d (1 .. %d) C=%d (1 .. %d)", Q, SEDT_MAX_QUERIES,
               C, SEDT_MAX_CLASSES);
  SEDT_REQUIRE(K >= 1 && K <= SEDT_MAX_THRESHOLDS, "stitch_stream: %d thresholds (1 .. %d)", K, SEDT_MAX_THRESHOLDS);
  SEDT_REQUIRE(S >= 1 && S <= 65535 && B >= 1, "stitch_stream: S=%d (1 .. 65535) B=%d (>= 1)", S, B);
  SEDT_REQUIRE(merge_gap >= 0.0 && merge_gap < INFINITY, "stitch_stream: merge_gap %.17g is not a finite number >= 0", merge_gap);
  SEDT_REQUIRE(emit_cap >= 1, "stitch_stream: emit_cap=%d (>= 1)", emit_cap);
  SEDT_REQUIRE((double)K * S * emit_cap * SEDT_EMIT_WORDS * 4.0 <= 4294967296.0, "stitch_stream: an emit buffer of K=%d x S=%d x emit_cap=%d "
               "events is larger than 4 GiB", K, S, emit_cap);
  SEDT_REQUIRE(records && action && row && t_w && dur && win_index && state && emit && emit_count && status, "stitch_stream: null pointer");
  SEDT_REQUIRE(state_bytes >= sedt_stitch_stream_state_bytes(K, S), "stitch_stream: a state of %lld bytes, K=%d x S=%d streams take %lld",
               (long long)state_bytes, K, S, (long long)sedt_stitch_stream_state_bytes(K, S));
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(emit) & 7) == 0 && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
               "stitch_stream: emit and state are not 8-byte aligned");
  hipLaunchKernelGGL(stitch_stream_kernel, dim3(S, K), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), records, action, row, t_w, dur,
                     win_index, S, B, Q, C, merge_gap, emit_cap, state, emit, emit_count, status);
  return check_launch("stitch_stream");
}

extern "C" int sedt_stream_reset(int32_t* state, int64_t state_bytes, const int32_t* which, int K, int S, int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(K >= 1 && K <= SEDT_MAX_THRESHOLDS && S >= 1 && S <= 65535, "stream_reset: K=%d (1 .. %d) S=%d (1 .. 65535)", K,
               SEDT_MAX_THRESHOLDS, S);
  SEDT_REQUIRE(state && status, "stream_reset: null pointer");
  SEDT_REQUIRE(state_bytes >= sedt_stitch_stream_state_bytes(K, S), "stream_reset: a state of %lld bytes, K=%d x S=%d streams take %lld",
               (long long)state_bytes, K, S, (long long)sedt_stitch_stream_state_bytes(K, S));
  const long n = (long)K * S * SEDT_SS_HDR;
  hipLaunchKernelGGL(stream_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), state,
                     which, n, S, status);
  return check_launch("stream_reset");
}
