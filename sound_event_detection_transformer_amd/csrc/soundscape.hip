// soundscape.hip - training soundscapes synthesized on the device from a bank of isolated sounds and background recordings
// (utilities/soundscape.py; DESIGN.md section 4, "Soundscapes synthesized on the device"; tests/soundscape_ref.py restates it in NumPy)
//   * bank_stats_kernel    one workgroup per source: sum of squares in float64 and max |x| (staging; sedt_bank_stats)
//   * scape_mix_kernel     workgroup 0 owns the targets; workgroups 1 .. B * chunks mix SEDT_SCAPE_CHUNK samples of one clip each and
//                          write their chunk's max |x| to `part`
//   * scape_scale_kernel   one workgroup per chunk: the clip's peak from its `part` row, the scale, and - only when the scale is not 1 -
//                          the rescaled chunk
// The reference trains on soundscapes that were mixed and annotated offline (URBAN-SED, DESED's synthetic subset) and merged per class
// by data_utils/collapse_event.py; there is no counterpart as a kernel.
//
// Wave: float32, every operation rounded on its own (no contraction).  acc = g_bg * bg[(start + t) mod len_bg] (0 without a background);
//   for every event k of the clip in plan order with onset_k <= t < e_k = min(onset_k + n_k, window), i = t - onset_k:
//   acc = acc + ((g_k * w_k(i)) * src_k[src_start_k + i]); w_k(i) = min(w_in, w_out), w_in = i < fade ? float((double)(i + 1) /
//   (double)(fade + 1)) : 1, w_out = n_k - 1 - i < fade ? float((double)(n_k - i) / (double)(fade + 1)) : 1.  peak = max |acc| over the
//   clip, scale = peak > peak_limit ? float((double)peak_limit / (double)peak) : 1; the written sample is acc * scale (acc untouched
//   when the scale is 1).  Sources are only 4-byte aligned: a chunk is split on the DESTINATION's 16-byte boundaries and a source is
//   loaded 16 bytes wide where its address allows it, as clips.hip does.
// Targets: every valid event gives (cls, onset, e_k) in samples.  With collapse the events of one class, sorted by (onset, end), are
//   merged while onset <= the running end (touching events included; data_utils/collapse_event.py: collapse), on the integer grid.
//   The merged events that pass the box test are ordered by (onset, end, cls); boxes with sedt_cut_clips' float64 formula from
//   a = onset / sr, z = end / sr, W = window / sr.  The targets workgroup walks the batch once, in tiles of consecutive clips: a
//   tile's events are resolved one per thread into LDS, one wave per clip merges and orders in registers, and the survivors written
//   so far are the next tile's offset.
// status: 2 a record outside the bank (it contributes nothing) or a CSR range longer than SEDT_SCAPE_MAXEV (cut to its first
//   SEDT_SCAPE_MAXEV events); else 1 more than max_targets survivors (the first max_targets are written); else 0.
// Every index is clamped before it is used: a source's [offset, offset + length) to the flat vector, a clip's event range to
//   ev_off[B] (itself clamped to 0 .. SEDT_SCAPE_MAXEV * B) and to SEDT_SCAPE_MAXEV events.
#include "common.h"

#pragma clang fp contract(off)     // g * w, (g * w) * x, acc + ...: every float32 operation of the definition is rounded on its own

namespace sedt {

#define SEDT_SCAPE_THREADS 256
#define SEDT_SCAPE_WAVES (SEDT_SCAPE_THREADS / 64)

struct __attribute__((packed, aligned(4))) ScapeF4 { float v[4]; };      // four floats behind a pointer that is only 4-byte aligned
typedef __attribute__((ext_vector_type(4))) float scape_f4;

__device__ __forceinline__ scape_f4 scape_load4(const float* p) {
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const scape_f4*>(p);
  const ScapeF4 u = *reinterpret_cast<const ScapeF4*>(p);
  return scape_f4{u.v[0], u.v[1], u.v[2], u.v[3]};
}

struct ScapeSrc {
  long off, len;      // clamped to the flat vector
  bool ok;            // the index names a source
};

__device__ __forceinline__ ScapeSrc scape_source(const int64_t* src_off, const int64_t* src_len, int n_src, long flat_len, int s) {
  if (s < 0 || s >= n_src) return {0, 0, false};
  const long off = min(max((long)src_off[s], 0L), flat_len);
  const long len = min(max((long)src_len[s], 0L), flat_len - off);
  return {off, len, true};
}

// an event resolved against the bank: p[0 .. n - 1] are its samples (never dereferenced outside), [onset, end) its place in the clip
struct ScapeEv {
  const float* p;
  long onset, end, n;
  float gain;
  int fade, cls, ok;
};

__device__ __forceinline__ ScapeEv scape_event(const float* flat, long flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                                               const SedtScapeEvent e, long window) {
  ScapeEv r;
  r.p = flat; r.onset = 0; r.end = 0; r.n = 0; r.gain = 0.0f; r.fade = 0; r.cls = e.cls; r.ok = 0;
  const ScapeSrc s = scape_source(src_off, src_len, n_src, flat_len, e.src);
  if (!s.ok || e.src_start < 0 || e.n < 0 || e.src_start > s.len || e.n > s.len - e.src_start || e.onset < 0) return r;
  r.ok = 1;
  r.p = flat + s.off + e.src_start;
  r.onset = e.onset;
  r.n = e.n;
  r.end = e.onset >= window ? window : min((long)(e.onset + e.n), window);      // min(onset + n, window) without overflow
  r.gain = e.gain;
  r.fade = max(e.fade, 0);
  return r;
}

// clip b's events: records e0 .. e0 + k - 1; cut: the range was longer than SEDT_SCAPE_MAXEV
__device__ __forceinline__ void scape_range(const int32_t* ev_off, int B, int b, int& e0, int& k, bool& cut) {
  const int total = min(max(ev_off[B], 0), SEDT_SCAPE_MAXEV * B);
  e0 = min(max(ev_off[b], 0), total);
  const int e1 = min(max(ev_off[b + 1], e0), total);
  cut = e1 - e0 > SEDT_SCAPE_MAXEV;
  k = min(e1 - e0, SEDT_SCAPE_MAXEV);
}

struct ScapeBgSrc {
  const float* p;     // the background's first sample
  long len, start;    // 0 <= start < len
  long lo, phase;     // the chunk's first sample and (start + lo) mod len (set by the mixing workgroup)
  float gain;
  bool on, bad;       // on: there is one; bad: the record names none and is not "none"
};

__device__ __forceinline__ ScapeBgSrc scape_background(const float* flat, long flat_len, const int64_t* src_off, const int64_t* src_len,
                                                       int n_src, const SedtScapeBg g) {
  ScapeBgSrc r;
  r.p = flat; r.len = 1; r.start = 0; r.lo = 0; r.phase = 0; r.gain = 0.0f; r.on = false; r.bad = false;
  if (g.src == -1) return r;
  const ScapeSrc s = scape_source(src_off, src_len, n_src, flat_len, g.src);
  if (!s.ok || g.start < 0 || g.start >= s.len) {
    r.bad = true;
    return r;
  }
  r.p = flat + s.off; r.len = s.len; r.start = g.start; r.gain = g.gain; r.on = true;
  return r;
}

__device__ __forceinline__ float scape_fade(long i, long n, int fade) {
  const float w_in = i < fade ? (float)((double)(i + 1) / (double)((long)fade + 1)) : 1.0f;
  const float w_out = n - 1 - i < fade ? (float)((double)(n - i) / (double)((long)fade + 1)) : 1.0f;
  return fminf(w_in, w_out);
}

// samples t .. t + N - 1 of the clip (all inside the chunk): N = 4 takes a source 16 bytes at a time where the four lie inside it
template <int N>
__device__ __forceinline__ void scape_mix(const ScapeBgSrc& g, const ScapeEv* evs, int n_act, long t, float* acc) {
  if (g.on) {
    long q = g.phase + (t - g.lo);                            // (start + t) mod len: one division per chunk, not per vector
    if (q >= g.len) {
      q -= g.len;
      if (q >= g.len) q %= g.len;
    }
    if (N == 4 && q + 4 <= g.len) {
      const scape_f4 x = scape_load4(g.p + q);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = g.gain * x[e];
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] = g.gain * g.p[(q + e) % g.len];
    }
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.0f;
  }
  for (int a = 0; a < n_act; ++a) {
    const ScapeEv& ev = evs[a];
    if (!(ev.onset < t + N && ev.end > t)) continue;
    const long i0 = t - ev.onset;
    if (N == 4 && i0 >= 0 && t + 4 <= ev.end) {
      const scape_f4 x = scape_load4(ev.p + i0);
      if (i0 >= ev.fade && ev.n - 4 - i0 >= ev.fade) {        // outside both ramps: w = 1 and g * 1 is g
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + (ev.gain * x[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + ((ev.gain * scape_fade(i0 + e, ev.n, ev.fade)) * x[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const long i = i0 + e;
        if (i >= 0 && t + e < ev.end) acc[e] = acc[e] + ((ev.gain * scape_fade(i, ev.n, ev.fade)) * ev.p[i]);
      }
    }
  }
}

__device__ __forceinline__ float scape_block_max(float m, float* red, int tid) {
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < SEDT_SCAPE_WAVES; ++w) r = fmaxf(r, red[w]);
  return r;
}

// ---- the targets.  A pass over the batch goes tile by tile: a tile is a run of consecutive clips (at most SEDT_SCAPE_TILE_CLIPS, at
// most SEDT_SCAPE_TILE_EV events; a clip holds at most SEDT_SCAPE_MAXEV, so a tile is never empty).  All threads resolve the tile's event
// records against the bank into LDS, one event per thread - the dependent loads (record, then the source's table entry) are paid once
// per tile, not once per clip; then one wave per clip merges and orders in registers.  Onsets are kept as min(onset, window): an
// event that starts at or behind the window's end has no samples and gives no target either way.
#define SEDT_SCAPE_TILE_CLIPS 64
#define SEDT_SCAPE_TILE_EV 256

struct ScapeTile {
  // the tile's events, one slot each; when a clip is done, its first slots hold its survivors in output order instead:
  // cls | the bits of the centre in on | the bits of the length in end
  int on[SEDT_SCAPE_TILE_EV], end[SEDT_SCAPE_TILE_EV], cls[SEDT_SCAPE_TILE_EV], ok[SEDT_SCAPE_TILE_EV];
  int who[SEDT_SCAPE_TILE_EV];              // the clip (of the tile) a slot belongs to
  int base[SEDT_SCAPE_TILE_CLIPS + 1];      // the tile's slots of clip c: base[c] .. base[c + 1] - 1
  int bad[SEDT_SCAPE_TILE_CLIPS];
  int cnt[SEDT_SCAPE_TILE_CLIPS];           // survivors of clip c (at most max_targets)
};

__device__ __forceinline__ bool scape_before(int on_a, int end_a, int cls_a, int ia, int on_b, int end_b, int cls_b, int ib) {
  if (on_a != on_b) return on_a < on_b;
  if (end_a != end_b) return end_a < end_b;
  if (cls_a != cls_b) return cls_a < cls_b;
  return ia < ib;
}

// clip b's event range from the clamped offsets in LDS: records e0 .. e0 + k - 1; cut: it was longer than SEDT_SCAPE_MAXEV
__device__ __forceinline__ void scape_range_lds(const int* eoff, int b, int& e0, int& k, bool& cut) {
  e0 = eoff[b];
  const int n = max(eoff[b + 1], e0) - e0;
  cut = n > SEDT_SCAPE_MAXEV;
  k = min(n, SEDT_SCAPE_MAXEV);
}

__device__ __forceinline__ int scape_lane(int v, int i) { return __builtin_amdgcn_readlane(v, i); }

// one clip from the tile, by one wave, in registers: lane j holds event j of the clip and reads the others' through readlane under
// wave-uniform loops - no LDS traffic, no barrier.  The survivors go to the clip's own slots of the tile, in output order.  Returns
// their number (at most M), st the clip's status.
__device__ int scape_clip_targets(ScapeTile& tile, int lane, int c_tile, long window, int sr, int M, double min_len, int collapse,
                                  int& st) {
  const int s0 = tile.base[c_tile], k = tile.base[c_tile + 1] - s0;
  const bool ok = lane < k && tile.ok[s0 + lane] != 0;
  const unsigned long long valid = __ballot(ok);              // the valid events, in plan order
  int c = 0, o = 0, e = 0;
  if (ok) { c = tile.cls[s0 + lane]; o = tile.on[s0 + lane]; e = tile.end[s0 + lane]; }
  bool kept = ok;
  if (collapse) {
    const int nv = __popcll(valid);
    int rank = 0;                                             // by (class, onset, end, plan order)
    for (unsigned long long r = valid; r; r &= r - 1ull) {
      const int i = __ffsll((long long)r) - 1;
      const int ci = scape_lane(c, i), oi = scape_lane(o, i), ei = scape_lane(e, i);
      rank += (ci != c ? ci < c : scape_before(oi, ei, 0, i, o, e, 0, lane)) ? 1 : 0;
    }
    if (!ok) rank = -1;
    int sc = 0, so = 0, se = 0;                               // lane j < nv takes the event of rank j
    for (unsigned long long r = valid; r; r &= r - 1ull) {
      const int i = __ffsll((long long)r) - 1;
      const int ri = scape_lane(rank, i), ci = scape_lane(c, i), oi = scape_lane(o, i), ei = scape_lane(e, i);
      if (ri == lane) { sc = ci; so = oi; se = ei; }
    }
    bool first = true;                                        // an event opens a group unless it starts inside the class's running end
    int pmax = 0;
    for (int i = 0; i < nv; ++i) {
      const int ci = scape_lane(sc, i), ei = scape_lane(se, i);
      if (i < lane && ci == sc) { pmax = first ? ei : max(pmax, ei); first = false; }
    }
    const int head = (lane < nv && (first || so > pmax)) ? 1 : 0;
    bool open = true;                                         // the group's end: the maximum over the events that joined it
    int ge = se;
    for (int i = 1; i < nv; ++i) {
      const int ci = scape_lane(sc, i), hi = scape_lane(head, i), ei = scape_lane(se, i);
      if (i > lane && open) {
        if (ci == sc && !hi) ge = max(ge, ei); else open = false;
      }
    }
    c = sc; o = so; e = ge;
    kept = head != 0;
  }
  const double W = (double)window / (double)sr;
  float centre = 0.0f, length = 0.0f;
  if (kept) {
    const double a = (double)o / (double)sr, z = (double)e / (double)sr;
    const double d = z - a;
    kept = d > 0.0 && d >= min_len;
    centre = (float)(((a + z) * 0.5) / W);
    length = (float)(d / W);
  }
  const unsigned long long keep = __ballot(kept);
  const int total = __popcll(keep);
  int rank = 0;                                               // place by (onset, end, class)
  for (unsigned long long r = keep; r; r &= r - 1ull) {
    const int i = __ffsll((long long)r) - 1;
    const int ci = scape_lane(c, i), oi = scape_lane(o, i), ei = scape_lane(e, i);
    rank += scape_before(oi, ei, ci, i, o, e, c, lane) ? 1 : 0;
  }
  if (kept && rank < M) {                                     // (every lane has read its event: the slots are this wave's to reuse)
    tile.cls[s0 + rank] = c;
    tile.on[s0 + rank] = __float_as_int(centre);
    tile.end[s0 + rank] = __float_as_int(length);
  }
  st = tile.bad[c_tile] ? 2 : (total > M ? 1 : 0);
  return min(total, M);
}

__device__ __forceinline__ int scape_scan64(int v, int lane) {              // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// the targets of the batch (the whole workgroup), tile by tile in clip order: the survivors written so far are the next tile's offset,
// so one walk both counts and writes
__device__ void scape_targets(ScapeTile& tile, const int* eoff, const float* flat, long flat_len, const int64_t* src_off,
                              const int64_t* src_len, int n_src, const SedtScapeBg* bg, const SedtScapeEvent* ev, int B, long window,
                              int sr, int M, double min_len, int collapse, int32_t* lab_off, int32_t* box_off, int64_t* lab_cat,
                              float* box_cat, int32_t* status) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  int run = 0;                                                // survivors written so far
  for (int b0 = 0; b0 < B;) {
    // the tile: lane c of every wave looks at clip b0 + c; the tile ends before the first clip that would pass SEDT_SCAPE_TILE_EV
    int e0 = 0, k = 0;
    bool cut = false;
    const bool has = b0 + lane < B;
    if (has) scape_range_lds(eoff, b0 + lane, e0, k, cut);
    const int incl = scape_scan64(k, lane);
    const int nc = __popcll(__ballot(has && incl <= SEDT_SCAPE_TILE_EV));        // (a prefix of the lanes; at least one)
    const int slots = __shfl(incl, nc - 1, 64);
    if (w == 0 && lane < nc) {
      tile.base[lane] = incl - k;
      tile.bad[lane] = (cut || scape_background(flat, flat_len, src_off, src_len, n_src, bg[b0 + lane]).bad) ? 1 : 0;
      if (lane == nc - 1) tile.base[nc] = incl;
    }
    __syncthreads();
    if (tid < slots) {                                        // one event per thread (a tile holds no more events than threads)
      int lo = 0, hi = nc - 1;                                // the clip c with base[c] <= tid < base[c + 1]
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile.base[mid] <= tid) lo = mid; else hi = mid - 1;
      }
      const ScapeEv r = scape_event(flat, flat_len, src_off, src_len, n_src, ev[eoff[b0 + lo] + (tid - tile.base[lo])], window);
      tile.ok[tid] = r.ok;
      tile.cls[tid] = r.cls;
      tile.on[tid] = (int)min(r.onset, window);
      tile.end[tid] = (int)r.end;
      tile.who[tid] = lo;
      if (!r.ok) tile.bad[lo] = 1;                            // (every writer writes 1)
    }
    __syncthreads();
    for (int c = w; c < nc; c += SEDT_SCAPE_WAVES) {         // wave w: clips w, w + 4, ... of the tile
      int st;
      const int n = scape_clip_targets(tile, lane, c, window, sr, M, min_len, collapse, st);
      if (lane == 0) {
        tile.cnt[c] = n;
        status[b0 + c] = st;
      }
    }
    __syncthreads();
    // the clips' offsets: every wave scans the same counts; then one staged survivor per thread goes to its place
    const int n = lane < nc ? tile.cnt[lane] : 0;
    const int upto = scape_scan64(n, lane);
    const int excl = upto - n;
    if (w == 0 && lane < nc) {
      lab_off[b0 + lane] = run + excl;
      box_off[b0 + lane] = run + excl;
    }
    const int c = tid < slots ? tile.who[tid] : 0;
    const int n_c = __shfl(n, c, 64), at_c = __shfl(excl, c, 64);
    if (tid < slots) {
      const int r = tid - tile.base[c];
      if (r < n_c) {
        const int dst = run + at_c + r;
        lab_cat[dst] = (int64_t)tile.cls[tid];
        box_cat[2 * dst] = __int_as_float(tile.on[tid]);
        box_cat[2 * dst + 1] = __int_as_float(tile.end[tid]);
      }
    }
    run += __shfl(upto, 63, 64);
    __syncthreads();                                          // the next tile overwrites this one
    b0 += nc;
  }
  if (tid == 0) {
    lab_off[B] = run;
    box_off[B] = run;
    box_off[B + 1] = B;          // the split words: every clip strong, every clip labelled
    box_off[B + 2] = B;
  }
}

struct ScapeMixLds {
  ScapeEv evs[64];               // the events that reach into the chunk
  int n_act;
  float red[SEDT_SCAPE_WAVES];
};
struct ScapeTargetsLds {
  ScapeTile tile;
  int eoff[SEDT_SCAPE_MAXB + 1]; // ev_off, clamped
};
union ScapeLds {
  ScapeMixLds mix;
  ScapeTargetsLds tgt;
};

__global__ __launch_bounds__(SEDT_SCAPE_THREADS) void scape_mix_kernel(
    const float* __restrict__ flat, long flat_len, const int64_t* __restrict__ src_off, const int64_t* __restrict__ src_len, int n_src,
    const SedtScapeBg* __restrict__ bg, const SedtScapeEvent* __restrict__ ev, const int32_t* __restrict__ ev_off, int B, long window,
    int chunks, int sr, int M, double min_len, int collapse, float* __restrict__ wave, float* __restrict__ part,
    unsigned char* __restrict__ blob, int32_t* __restrict__ status) {
  __shared__ ScapeLds lds;       // a workgroup mixes or owns the targets: one footprint, 8 workgroups per CU
  const int tid = threadIdx.x;
  if (blockIdx.x > 0) {
    // ---- the wave part: one chunk of one clip
    ScapeEv* evs = lds.mix.evs;
    float* red = lds.mix.red;
    const unsigned blk = blockIdx.x - 1u;
    const int b = (int)(blk / (unsigned)chunks), c = (int)(blk % (unsigned)chunks);
    const long lo = (long)c * SEDT_SCAPE_CHUNK, hi = min(lo + SEDT_SCAPE_CHUNK, window);
    ScapeBgSrc g = scape_background(flat, flat_len, src_off, src_len, n_src, bg[b]);
    g.lo = lo;
    g.phase = (g.start + lo) % g.len;
    if (tid < 64) {                                           // wave 0: the events that reach into this chunk, in plan order
      int e0, k;
      bool cut;
      scape_range(ev_off, B, b, e0, k, cut);
      ScapeEv r;
      bool act = false;
      if (tid < k) {
        r = scape_event(flat, flat_len, src_off, src_len, n_src, ev[e0 + tid], window);
        act = r.ok && r.onset < hi && r.end > lo;
      }
      const unsigned long long m = __ballot(act);
      if (act) evs[__popcll(m & ((1ull << tid) - 1ull))] = r;
      if (tid == 0) lds.mix.n_act = __popcll(m);
    }
    __syncthreads();
    const int n_act = lds.mix.n_act;
    float* __restrict__ d = wave + (long)b * window;
    const int head = (int)min((long)((4 - (int)((reinterpret_cast<uintptr_t>(d + lo) >> 2) & 3)) & 3), hi - lo);
    const long body = lo + head;
    const int nvec = (int)((hi - body) >> 2);
    const long tail = body + 4L * nvec;
    float peak = 0.0f;
    if (tid < head) {
      float a[1];
      scape_mix<1>(g, evs, n_act, lo + tid, a);
      d[lo + tid] = a[0];
      peak = fmaxf(peak, fabsf(a[0]));
    }
    for (int v = tid; v < nvec; v += SEDT_SCAPE_THREADS) {
      const long t = body + 4L * v;
      float a[4];
      scape_mix<4>(g, evs, n_act, t, a);
      *reinterpret_cast<scape_f4*>(d + t) = scape_f4{a[0], a[1], a[2], a[3]};
      peak = fmaxf(fmaxf(peak, fmaxf(fabsf(a[0]), fabsf(a[1]))), fmaxf(fabsf(a[2]), fabsf(a[3])));
    }
    if (tid < (int)(hi - tail)) {
      float a[1];
      scape_mix<1>(g, evs, n_act, tail + tid, a);
      d[tail + tid] = a[0];
      peak = fmaxf(peak, fabsf(a[0]));
    }
    peak = scape_block_max(peak, red, tid);
    if (tid == 0) part[(long)b * chunks + c] = peak;
    return;
  }
  // ---- the target part
  int* eoff = lds.tgt.eoff;
  int32_t* lab_off = reinterpret_cast<int32_t*>(blob);
  {
    const int total = min(max(ev_off[B], 0), SEDT_SCAPE_MAXEV * B);      // the record count: every offset is clamped to it
    for (int b = tid; b <= B; b += SEDT_SCAPE_THREADS) eoff[b] = min(max(ev_off[b], 0), total);
  }
  __syncthreads();
  scape_targets(lds.tgt.tile, eoff, flat, flat_len, src_off, src_len, n_src, bg, ev, B, window, sr, M, min_len, collapse, lab_off,
                lab_off + (B + 1), reinterpret_cast<int64_t*>(blob + 8L * B + 16),
                reinterpret_cast<float*>(blob + 8L * B + 16 + 8L * B * M), status);
}

__global__ __launch_bounds__(SEDT_SCAPE_THREADS) void scape_scale_kernel(const float* __restrict__ part, int B, long window, int chunks,
                                                                          float peak_limit, float* __restrict__ wave,
                                                                          float* __restrict__ peak, float* __restrict__ scale) {
  __shared__ float red[SEDT_SCAPE_WAVES];
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)chunks), c = (int)(blockIdx.x % (unsigned)chunks);
  float m = 0.0f;
  for (int i = tid; i < chunks; i += SEDT_SCAPE_THREADS) m = fmaxf(m, part[(long)b * chunks + i]);
  m = scape_block_max(m, red, tid);
  const float s = m > peak_limit ? (float)((double)peak_limit / (double)m) : 1.0f;
  if (c == 0 && tid == 0) {
    peak[b] = m;
    scale[b] = s;
  }
  if (s == 1.0f) return;                                      // the same for the whole workgroup
  float* __restrict__ d = wave + (long)b * window;
  const long lo = (long)c * SEDT_SCAPE_CHUNK, hi = min(lo + SEDT_SCAPE_CHUNK, window);
  const int head = (int)min((long)((4 - (int)((reinterpret_cast<uintptr_t>(d + lo) >> 2) & 3)) & 3), hi - lo);
  const long body = lo + head;
  const int nvec = (int)((hi - body) >> 2);
  const long tail = body + 4L * nvec;
  if (tid < head) d[lo + tid] = d[lo + tid] * s;
  for (int v = tid; v < nvec; v += SEDT_SCAPE_THREADS) {
    scape_f4* q = reinterpret_cast<scape_f4*>(d + body + 4L * v);
    const scape_f4 x = *q;
    *q = scape_f4{x[0] * s, x[1] * s, x[2] * s, x[3] * s};
  }
  if (tid < (int)(hi - tail)) d[tail + tid] = d[tail + tid] * s;
}

// one workgroup per source: thread t adds the squares of elements t, t + 256, ... in float64 (a float32 square is exact there), then a
// fixed tree over the 256 partial sums - no atomics, so the bits do not depend on the launch
__global__ __launch_bounds__(SEDT_SCAPE_THREADS) void bank_stats_kernel(const float* __restrict__ flat, long flat_len,
                                                                         const int64_t* __restrict__ src_off,
                                                                         const int64_t* __restrict__ src_len,
                                                                         double* __restrict__ sumsq, float* __restrict__ peak) {
  __shared__ double acc[SEDT_SCAPE_THREADS];
  __shared__ float top[SEDT_SCAPE_THREADS];
  const int tid = threadIdx.x, s = blockIdx.x;
  const long off = min(max((long)src_off[s], 0L), flat_len);
  const long len = min(max((long)src_len[s], 0L), flat_len - off);
  const float* p = flat + off;
  double a = 0.0;
  float m = 0.0f;
  for (long i = tid; i < len; i += SEDT_SCAPE_THREADS) {
    const float x = p[i];
    a = a + (double)x * (double)x;
    m = fmaxf(m, fabsf(x));
  }
  acc[tid] = a;
  top[tid] = m;
  __syncthreads();
  for (int h = SEDT_SCAPE_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      acc[tid] = acc[tid] + acc[tid + h];
      top[tid] = fmaxf(top[tid], top[tid + h]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    sumsq[s] = acc[0];
    peak[s] = top[0];
  }
}

}  // namespace sedt

extern "C" int sedt_bank_stats(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                               double* sumsq, float* peak, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_src >= 1 && n_src <= 0x7fffffff && flat_len >= 0, "bank_stats: n_src=%d flat_len=%lld (1 <= n_src, 0 <= flat_len)", n_src,
               (long long)flat_len);
  SEDT_REQUIRE(flat && src_off && src_len && sumsq && peak, "bank_stats: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 3) == 0 && (reinterpret_cast<uintptr_t>(sumsq) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(src_off) & 7) == 0 && (reinterpret_cast<uintptr_t>(src_len) & 7) == 0,
               "bank_stats: the waveforms are 4-byte aligned, the tables and sums 8-byte aligned");
  hipLaunchKernelGGL(bank_stats_kernel, dim3((unsigned)n_src), dim3(SEDT_SCAPE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), flat,
                     (long)flat_len, src_off, src_len, sumsq, peak);
  return check_launch("bank_stats");
}

extern "C" int sedt_soundscape(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                               const SedtScapeBg* bg, const SedtScapeEvent* ev, const int32_t* ev_off, int B, int64_t window, int sr,
                               int max_targets, double min_event_seconds, int collapse, float peak_limit, float* wave, float* part,
                               float* peak, float* scale, void* blob, int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(B >= 1 && B <= SEDT_SCAPE_MAXB && max_targets >= 1 && max_targets <= 63,
               "soundscape: B=%d max_targets=%d outside the envelope (1 <= B <= %d clips per call; 1 <= max_targets <= 63, the target "
               "tables' own limit)", B, max_targets, SEDT_SCAPE_MAXB);
  SEDT_REQUIRE(window >= 1 && window <= 0x7fffffffL && sr >= 1 && n_src >= 1 && flat_len >= 0,
               "soundscape: window=%lld sr=%d n_src=%d flat_len=%lld", (long long)window, sr, n_src, (long long)flat_len);
  SEDT_REQUIRE(min_event_seconds == min_event_seconds, "soundscape: min_event_seconds is NaN");
  SEDT_REQUIRE(peak_limit == peak_limit && peak_limit > 0.0f, "soundscape: peak_limit=%g is not a number > 0", (double)peak_limit);
  const long chunks = (long)((window + SEDT_SCAPE_CHUNK - 1) / SEDT_SCAPE_CHUNK);
  SEDT_REQUIRE((long)B * chunks + 1 <= 0x7fffffffL, "soundscape: %d clips of %lld samples are more workgroups than a launch holds", B,
               (long long)window);
  SEDT_REQUIRE(flat && src_off && src_len && bg && ev && ev_off && wave && part && peak && scale && blob && status,
               "soundscape: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(blob) & 7) == 0 && (reinterpret_cast<uintptr_t>(bg) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(ev) & 7) == 0 && (reinterpret_cast<uintptr_t>(src_off) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(src_len) & 7) == 0 && (reinterpret_cast<uintptr_t>(wave) & 3) == 0 &&
               (reinterpret_cast<uintptr_t>(flat) & 3) == 0 && (reinterpret_cast<uintptr_t>(ev_off) & 3) == 0,
               "soundscape: the blob, the records and the source tables are 8-byte aligned, the waveforms 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(scape_mix_kernel, dim3((unsigned)((long)B * chunks + 1)), dim3(SEDT_SCAPE_THREADS), 0, s, flat, (long)flat_len,
                     src_off, src_len, n_src, bg, ev, ev_off, B, (long)window, (int)chunks, sr, max_targets, min_event_seconds,
                     collapse ? 1 : 0, wave, part, reinterpret_cast<unsigned char*>(blob), status);
  hipLaunchKernelGGL(scape_scale_kernel, dim3((unsigned)((long)B * chunks)), dim3(SEDT_SCAPE_THREADS), 0, s, part, B, (long)window,
                     (int)chunks, peak_limit, wave, peak, scale);
  return check_launch("soundscape");
}
