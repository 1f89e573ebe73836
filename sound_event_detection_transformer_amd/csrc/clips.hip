// clips.hip - training batches cut from annotated recordings that live on the device: ONE launch writes the batch's windows and the
// windows' target tables (utilities/recording_clips.py; DESIGN.md section 4, "Training on recordings")
//   * cut_clips_kernel   workgroups 0 .. B * chunks - 1 copy SEDT_CLIPS_CHUNK samples of one row each; the last workgroup owns the targets
// The reference cuts its 10 s clips and encodes their strong labels on the host (data_utils/DataLoad.py, BoxEncoder.encode_strong_df);
// tests/recording_clips_ref.py restates the definition below in NumPy.
//
// Wave part: row b of wave [B][window] is samples start[b] .. start[b] + window - 1 of recording rec[b] of the flat vector, bit for bit;
//   positions past the recording's end are written as zero.  start is any sample index, so the source is only 4-byte aligned: a chunk
//   is split on the DESTINATION's 16-byte boundaries (scalar head and tail, 16-byte stores in between) and the body's loads are 16 bytes
//   wide where the source address allows it, four single loads where it does not.
// Target part: float64, plain subtract / multiply / divide / compare, no contraction.  W = window / sr, t0 = start[b] / sr, t1 = t0 + W.
//   For every event (class c, on, end) of the recording in table order (the host sorts a recording's events by (onset, offset, input
//   order)): a = max(on, t0) - t0, z = min(end, t1) - t0; it is kept iff z - a > 0 and z - a >= min_event_seconds, and becomes label c
//   (int64) and box (float32(((a + z) * 0.5) / W), float32((z - a) / W)).  Nothing is merged.  Two binary searches bound the scan: the
//   first event whose prefix maximum of the offsets exceeds t0 (no event before it ends after t0) and the first onset >= t1.
//   status [B] int32: 0; 1 more than max_targets events survive (the first max_targets in table order are written); 2 the pick is not
//   inside the table (rec outside 0 .. n_rec - 1 or start < 0: a row of zeros, no events).
// Blob: the layout of TargetTables(batch=B, ns=B, n_lab=B, max_targets=M, with_ratio=False): int32 lab_off [B + 1] | box_off [B + 1] | B | B,
//   then at byte 8 B + 16 lab_cat int64 [B M], then box_cat float32 [B M][2]; the offsets are exclusive scans over the clips and, every
//   clip being strong, box_off == lab_off.  Only the live entries are written.
// Every index is clamped before it is used: a recording's [offset, offset + length) to the flat vector, its event range to the table.
#include "common.h"

#pragma clang fp contract(off)     // (a + z) * 0.5, z - a: the plain float64 operations of the definition

namespace sedt {

#define SEDT_CLIPS_THREADS 256
#define SEDT_CLIPS_PER_THREAD (SEDT_CLIPS_MAXB / SEDT_CLIPS_THREADS)

struct __attribute__((packed, aligned(4))) ClipF4 { float v[4]; };      // four floats behind a pointer that is only 4-byte aligned

struct ClipSrc {
  const float* p;     // first sample of the window (never dereferenced at or past n)
  long n;             // samples of the window that exist: 0 .. window
};

// the window of pick b inside the flat vector, or {., 0} for a pick outside the table
__device__ __forceinline__ ClipSrc clip_source(const float* flat, long flat_len, const int64_t* rec_off, const int64_t* rec_len, int n_rec,
                                               const int32_t* pick_rec, const int64_t* pick_start, int b, long window) {
  const int r = pick_rec[b];
  const long start = pick_start[b];
  if (r < 0 || r >= n_rec || start < 0) return {flat, 0};
  const long off = min(max((long)rec_off[r], 0L), flat_len);
  const long len = min(max((long)rec_len[r], 0L), flat_len - off);
  const long n = min(max(len - start, 0L), window);
  return {n > 0 ? flat + off + start : flat, n};
}

typedef __attribute__((ext_vector_type(4))) float clip_f4;

// the 16-byte body of a chunk: nvec vectors from element `body` on, stores aligned; WIDE: the source is 16-byte aligned there too
template <bool WIDE>
__device__ __forceinline__ void cut_wave_body(const ClipSrc s, float* __restrict__ d, long body, int nvec, int tid) {
  for (int v = tid; v < nvec; v += SEDT_CLIPS_THREADS) {
    const long i = body + 4L * v;
    clip_f4 o;
    if (i + 4 <= s.n) {
      if (WIDE) {
        o = *reinterpret_cast<const clip_f4*>(s.p + i);
      } else {
        const ClipF4 u = *reinterpret_cast<const ClipF4*>(s.p + i);
        o = clip_f4{u.v[0], u.v[1], u.v[2], u.v[3]};
      }
    } else {
      o = clip_f4{i < s.n ? s.p[i] : 0.0f, i + 1 < s.n ? s.p[i + 1] : 0.0f, i + 2 < s.n ? s.p[i + 2] : 0.0f, 0.0f};
    }
    *reinterpret_cast<clip_f4*>(d + i) = o;
  }
}

__device__ __forceinline__ void cut_wave_chunk(const ClipSrc s, float* __restrict__ d, long lo, long hi, int tid) {
  const int head = (int)min((long)((4 - (int)((reinterpret_cast<uintptr_t>(d + lo) >> 2) & 3)) & 3), hi - lo);
  const long body = lo + head;
  const int nvec = (int)((hi - body) >> 2);
  const long tail = body + 4L * nvec;
  if (tid < head) d[lo + tid] = lo + tid < s.n ? s.p[lo + tid] : 0.0f;
  if ((reinterpret_cast<uintptr_t>(s.p + body) & 15) == 0)
    cut_wave_body<true>(s, d, body, nvec, tid);
  else
    cut_wave_body<false>(s, d, body, nvec, tid);
  if (tid < (int)(hi - tail)) d[tail + tid] = tail + tid < s.n ? s.p[tail + tid] : 0.0f;
}

// one clip's events: the scan range of the table and the clip's times
struct ClipScan {
  int j0, j1;
  double t0, t1, W;
};

__device__ __forceinline__ ClipScan clip_scan(int n_rec, const int32_t* pick_rec, const int64_t* pick_start, int b, long window, int sr,
                                              const int32_t* ev_off, const double* ev_on, const double* ev_pmax,
                                              int n_events, int& st) {
  ClipScan c;
  c.W = (double)window / (double)sr;
  const int r = pick_rec[b];
  const long start = pick_start[b];
  c.j0 = c.j1 = 0;
  c.t0 = c.t1 = 0.0;
  if (r < 0 || r >= n_rec || start < 0) {
    st = 2;
    return c;
  }
  st = 0;
  c.t0 = (double)start / (double)sr;
  c.t1 = c.t0 + c.W;
  const int e0 = min(max(ev_off[r], 0), n_events), e1 = min(max(ev_off[r + 1], e0), n_events);
  int lo = e0, hi = e1;                     // the first event whose prefix maximum of the offsets exceeds t0
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ev_pmax[mid] > c.t0) hi = mid; else lo = mid + 1;
  }
  c.j0 = lo;
  hi = e1;                                  // the first onset >= t1 (lo: no earlier than j0)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ev_on[mid] >= c.t1) hi = mid; else lo = mid + 1;
  }
  c.j1 = lo;
  return c;
}

// event j clipped to the clip: kept or not, and its box
__device__ __forceinline__ bool clip_event(const ClipScan& c, double on, double end, double min_len, float& centre, float& length) {
  const double a = fmax(on, c.t0) - c.t0, z = fmin(end, c.t1) - c.t0;
  const double d = z - a;
  if (!(d > 0.0 && d >= min_len)) return false;
  centre = (float)(((a + z) * 0.5) / c.W);
  length = (float)(d / c.W);
  return true;
}

__global__ __launch_bounds__(SEDT_CLIPS_THREADS) void cut_clips_kernel(
    const float* __restrict__ flat, long flat_len, const int64_t* __restrict__ rec_off, const int64_t* __restrict__ rec_len, int n_rec,
    const int32_t* __restrict__ pick_rec, const int64_t* __restrict__ pick_start, int B, long window, int chunks, int sr,
    const int32_t* __restrict__ ev_off, const double* __restrict__ ev_on, const double* __restrict__ ev_end,
    const int32_t* __restrict__ ev_cls, const double* __restrict__ ev_pmax, int n_events, int M, double min_len,
    float* __restrict__ wave, unsigned char* __restrict__ blob, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  if (blockIdx.x < (unsigned)B * (unsigned)chunks) {
    // ---- the wave part: one chunk of one row
    const int b = (int)(blockIdx.x / (unsigned)chunks), c = (int)(blockIdx.x % (unsigned)chunks);
    const ClipSrc s = clip_source(flat, flat_len, rec_off, rec_len, n_rec, pick_rec, pick_start, b, window);
    const long lo = (long)c * SEDT_CLIPS_CHUNK;
    cut_wave_chunk(s, wave + (long)b * window, lo, min(lo + SEDT_CLIPS_CHUNK, window), tid);
    return;
  }
  // ---- the target part: thread t owns clips SEDT_CLIPS_PER_THREAD * t .. + SEDT_CLIPS_PER_THREAD - 1 (consecutive, so the scan over
  // the clips is a scan over the threads)
  __shared__ int wave_sum[SEDT_CLIPS_THREADS / 64];
  ClipScan scan[SEDT_CLIPS_PER_THREAD];
  int cnt[SEDT_CLIPS_PER_THREAD];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < SEDT_CLIPS_PER_THREAD; ++k) {
    const int b = SEDT_CLIPS_PER_THREAD * tid + k;
    cnt[k] = 0;
    if (b >= B) continue;
    int st;
    scan[k] = clip_scan(n_rec, pick_rec, pick_start, b, window, sr, ev_off, ev_on, ev_pmax, n_events, st);
    int n = 0;
    for (int j = scan[k].j0; j < scan[k].j1 && n <= M; ++j) {
      float cx, len;
      n += clip_event(scan[k], ev_on[j], ev_end[j], min_len, cx, len) ? 1 : 0;
    }
    if (n > M) st = 1;
    status[b] = st;
    cnt[k] = min(n, M);
    mine += cnt[k];
  }
  // exclusive scan of `mine` over the 256 threads
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if ((tid & 63) >= o) incl += up;
  }
  if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
  __syncthreads();
  int base = incl - mine, total = 0;
#pragma unroll
  for (int w = 0; w < SEDT_CLIPS_THREADS / 64; ++w) {
    if (w < (tid >> 6)) base += wave_sum[w];
    total += wave_sum[w];
  }
  int32_t* lab_off = reinterpret_cast<int32_t*>(blob);
  int32_t* box_off = lab_off + (B + 1);
  int64_t* lab_cat = reinterpret_cast<int64_t*>(blob + 8L * B + 16);
  float* box_cat = reinterpret_cast<float*>(blob + 8L * B + 16 + 8L * B * M);
  if (tid == 0) {
    lab_off[B] = total;
    box_off[B] = total;
    box_off[B + 1] = B;          // the split words: every clip strong, every clip labelled
    box_off[B + 2] = B;
  }
#pragma unroll
  for (int k = 0; k < SEDT_CLIPS_PER_THREAD; ++k) {
    const int b = SEDT_CLIPS_PER_THREAD * tid + k;
    if (b >= B) continue;
    lab_off[b] = base;
    box_off[b] = base;
    int n = 0;
    for (int j = scan[k].j0; j < scan[k].j1 && n < cnt[k]; ++j) {
      float cx, len;
      if (!clip_event(scan[k], ev_on[j], ev_end[j], min_len, cx, len)) continue;
      lab_cat[base + n] = (int64_t)ev_cls[j];
      box_cat[2 * (base + n)] = cx;
      box_cat[2 * (base + n) + 1] = len;
      ++n;
    }
    base += cnt[k];
  }
}

}  // namespace sedt

extern "C" int sedt_cut_clips(const float* flat, int64_t flat_len, const int64_t* rec_off, const int64_t* rec_len, int n_rec,
                              const int32_t* pick_rec, const int64_t* pick_start, int B, int64_t window, int sr, const int32_t* ev_off,
                              const double* ev_on, const double* ev_end, const int32_t* ev_cls, const double* ev_pmax, int n_events,
                              int max_targets, double min_event_seconds, float* wave, void* blob, int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(B >= 1 && B <= SEDT_CLIPS_MAXB && max_targets >= 1 && max_targets <= 63,
               "cut_clips: B=%d max_targets=%d outside the envelope (1 <= B <= %d clips per launch; 1 <= max_targets <= 63, the target "
               "tables' own limit)", B, max_targets, SEDT_CLIPS_MAXB);
  SEDT_REQUIRE(window >= 1 && window <= 0x7fffffffL && sr >= 1 && n_rec >= 1 && n_events >= 0 && flat_len >= 0,
               "cut_clips: window=%lld sr=%d n_rec=%d n_events=%d flat_len=%lld", (long long)window, sr, n_rec, n_events,
               (long long)flat_len);
  SEDT_REQUIRE(min_event_seconds == min_event_seconds, "cut_clips: min_event_seconds is NaN");
  const long chunks = (long)((window + SEDT_CLIPS_CHUNK - 1) / SEDT_CLIPS_CHUNK);
  SEDT_REQUIRE((long)B * chunks + 1 <= 0x7fffffffL, "cut_clips: %d windows of %lld samples are more workgroups than a launch holds", B,
               (long long)window);
  SEDT_REQUIRE(flat && rec_off && rec_len && pick_rec && pick_start && ev_off && ev_on && ev_end && ev_cls && ev_pmax && wave && blob &&
               status, "cut_clips: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(blob) & 7) == 0 && (reinterpret_cast<uintptr_t>(wave) & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(flat) & 3) == 0, "cut_clips: the blob is 8-byte aligned, the waveforms 4-byte aligned");
  hipLaunchKernelGGL(cut_clips_kernel, dim3((unsigned)((long)B * chunks + 1)), dim3(SEDT_CLIPS_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), flat, (long)flat_len, rec_off, rec_len, n_rec, pick_rec, pick_start, B,
                     (long)window, (int)chunks, sr, ev_off, ev_on, ev_end, ev_cls, ev_pmax, n_events, max_targets, min_event_seconds, wave,
                     reinterpret_cast<unsigned char*>(blob), status);
  return check_launch("cut_clips");
}
