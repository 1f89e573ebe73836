// reverb.hip - reverberation of E excerpts of a staged sound bank: each convolved with a room impulse response of a staged RIR bank
// by uniformly partitioned overlap-save convolution (utilities/reverb.py; DESIGN.md section 4, "Reverberation on the device";
// tests/reverb_ref.py restates the definition in float64).  The reference has no counterpart: its corpora were generated offline.
//
// N = n_fft, Bs = N / 2 samples per block, K = N / 2 + 1 bins.  RIR r of L taps is P = ceil(L / Bs) partitions; H[r][p] is the N-point
// real FFT of taps [p Bs, (p + 1) Bs) followed by Bs zeros (sedt_reverb_spectra: one launch over the bank, separate re / im arrays).
// Per job (SedtReverbJob, include/sedt_hip.h): x = flat[src_off .. src_off + n) times the event's fade, wet = dst[dst_off .. dst_off +
// n + L - 1).  Two launches behind one another on the stream, each over all E jobs (grid y = the job):
//   reverb_fwd_kernel   ST_FPB input blocks per workgroup in LDS: block j = x[(j - 1) Bs, (j + 1) Bs), zero outside [0, n), faded, the
//                       packed real FFT of fft_lds.h, X[j][K] to the workspace; workgroup (0, e) also writes status[e]
//   reverb_mac_kernel   a workgroup owns G consecutive output blocks: Y_j = sum over p ascending of X[j - p] H[r][p], the accumulators
//                       in registers, a window of G input spectra sliding through registers so that every step loads ONE X and ONE H
//                       for G products; then the packed inverse real FFT in LDS and the LAST Bs samples of each frame to dst
// No atomics anywhere, no allocation, no synchronisation: the same call gives the same bits, whatever G.
// Every kernel re-checks its DEVICE record (rv_job_ok) against the bank, the destination, the workspace and the DEVICE RIR table before
// it touches memory: a bad record raises status 2 and nothing is read or written for it.  The loops are bounded by the record's own n
// and the table's own L, which the check ties to the buffers.
// sedt_reverb_bed lays the wet events' tails over a clip's background (one thread per sample, every operation rounded on its own).
// LDS: (2 (N/2 + 1) + ST_FPB * 2 N) * 4 bytes = 72 KB at N = 2048, as stretch_stft_kernel.
#include "common.h"
#include "fft_lds.h"

#include <math.h>

namespace sedt {

constexpr long RV_MAX_N = 1L << 26;
constexpr int RV_G_DEFAULT = 4;          // output blocks per workgroup of the MAC launch (DESIGN.md quotes the measurement)
constexpr int RV_BED_THREADS = 256;

__host__ __device__ inline long rv_blocks_in(int N, long n) { return (n + N / 2 - 1) / (N / 2) + 1; }
__host__ __device__ inline long rv_job_floats(int N, long n) { return (2L * rv_blocks_in(N, n) * (N / 2 + 1) + 3) & ~3L; }

// what both the entry point (on the host copies) and every kernel (on the device copies) ask of a job and its response, the buffers aside
__host__ __device__ inline bool rv_shape_ok(int N, long n, long L, long fade) {
  if (!(N == 512 || N == 1024 || N == 2048)) return false;
  return n >= 1 && n <= RV_MAX_N && L >= 1 && L <= (long)SEDT_REVERB_MAXPART * (N / 2) && fade >= 0 && fade <= RV_MAX_N;
}

// the RIR table int64 [3][R]: taps | first partition | first tap in the tap array
struct RvRir {
  long L, part, tap;
};
__host__ __device__ inline bool rv_rir_ok(const int64_t* tab, int R, long r, int N, long n_parts, RvRir* out) {
  if (r < 0 || r >= R) return false;
  const long L = (long)tab[r], part = (long)tab[R + r];
  if (!(L >= 1 && L <= (long)SEDT_REVERB_MAXPART * (N / 2))) return false;
  const long P = (L + N / 2 - 1) / (N / 2);
  if (part < 0 || part > n_parts || P > n_parts - part) return false;
  out->L = L, out->part = part, out->tap = (long)tab[2 * R + r];
  return true;
}

__device__ __forceinline__ bool rv_job_ok(const SedtReverbJob& j, int N, long flat_len, long dst_len, long ws_len, const int64_t* tab, int R,
                                          long n_parts, RvRir* rir) {
  if (!rv_rir_ok(tab, R, (long)j.rir, N, n_parts, rir)) return false;
  if (!rv_shape_ok(N, j.n, rir->L, (long)j.fade)) return false;
  if (j.src_off < 0 || j.src_off > flat_len || j.n > flat_len - j.src_off) return false;
  if (j.dst_off < 0 || j.dst_off > dst_len || j.n + rir->L - 1 > dst_len - j.dst_off) return false;
  if (j.ws_off < 0 || (j.ws_off & 3) || j.ws_off > ws_len || rv_job_floats(N, j.n) > ws_len - j.ws_off) return false;
  return true;
}

// the ramp of soundscape.hip's scape_fade over n samples: float64 divisions, only inside a ramp
__device__ __forceinline__ float rv_fade(long i, long n, int fade) {
  const float w_in = i < fade ? (float)((double)(i + 1) / (double)((long)fade + 1)) : 1.0f;
  const float w_out = n - 1 - i < fade ? (float)((double)(n - i) / (double)((long)fade + 1)) : 1.0f;
  return fminf(w_in, w_out);
}

// ST_FPB real frames of N samples, packed in buffer 0 of `frames` (z[k] = v[2 k] + i v[2 k + 1]) -> their bins 0 .. N/2 to
// out_re / out_im [t][K], rows t0 .. min(t0 + ST_FPB, T) - 1:  X[k] = (Z[k] + conj Z[M-k]) / 2 + W[k] (Z[k] - conj Z[M-k]) / (2i)
__device__ __forceinline__ void rv_forward(float* frames, const float* twr, const float* twi, int N, int tid, float* out_re, float* out_im,
                                           long t0, long T) {
  const int M = N / 2, K = N / 2 + 1;
  const int p = st_fft(frames, twr, twi, N, tid);
  for (int idx = tid; idx < ST_FPB * K; idx += ST_THREADS) {
    const int f = idx / K, k = idx - f * K;
    const long t = t0 + f;
    if (t >= T) continue;
    const float* xr = frames + (long)f * 4 * M + p * 2 * M;
    const float* xi = xr + M;
    const int ka = k & (M - 1), kb = (M - k) & (M - 1);
    const scf32 zk{xr[ka], xi[ka]}, zm{xr[kb], -xi[kb]};
    const scf32 s = zk + zm, d = zk - zm;
    const scf32 o{0.5f * d.im, -0.5f * d.re};                              // (zk - zm) / 2i
    const float wr = twr[k], wi = twi[k];
    out_re[t * K + k] = 0.5f * s.re + (o.re * wr - o.im * wi);
    out_im[t * K + k] = 0.5f * s.im + (o.re * wi + o.im * wr);
  }
}

// the partition spectra of the whole bank: workgroup (x, r) owns partitions x ST_FPB .. of response r
__global__ __launch_bounds__(ST_THREADS) void reverb_spectra_kernel(const float* __restrict__ taps, long taps_len,
                                                                     const int64_t* __restrict__ tab, int R, float* __restrict__ hre,
                                                                     float* __restrict__ him, long n_parts,
                                                                     const float* __restrict__ twiddle, int N) {
  extern __shared__ float rv_lds[];
  const int M = N / 2, H = N / 2, K = N / 2 + 1, Bs = N / 2;
  const int r = blockIdx.y, tid = threadIdx.x;
  const long p0 = (long)blockIdx.x * ST_FPB;
  RvRir rir;
  if (!rv_rir_ok(tab, R, r, N, n_parts, &rir)) return;
  if (rir.tap < 0 || rir.tap > taps_len || rir.L > taps_len - rir.tap) return;
  const long P = (rir.L + Bs - 1) / Bs;
  if (p0 >= P) return;                     // (uniform over the workgroup)
  float* twr = rv_lds;                     // [H + 1] cos
  float* twi = rv_lds + (H + 1);           // [H + 1] -sin
  float* frames = rv_lds + 2 * (H + 1);    // [ST_FPB][2 buffers][re M | im M]
  for (int i = tid; i < 2 * (H + 1); i += ST_THREADS) rv_lds[i] = twiddle[i];
  const float* __restrict__ h = taps + rir.tap;
  // ---- load, pack: frame p = taps [p Bs, (p + 1) Bs) then Bs zeros
  for (int idx = tid; idx < ST_FPB * M; idx += ST_THREADS) {
    const int f = idx / M, k = idx - f * M;
    const long p = p0 + f;
    float v[2] = {0.f, 0.f};
    if (p < P && 2 * k < Bs) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const long q = p * Bs + 2 * k + c;
        if (q < rir.L) v[c] = h[q];
      }
    }
    float* re = frames + (long)f * 4 * M;
    re[k] = v[0];
    re[M + k] = v[1];
  }
  __syncthreads();
  rv_forward(frames, twr, twi, N, tid, hre + rir.part * K, him + rir.part * K, p0, P);
}

__global__ __launch_bounds__(ST_THREADS) void reverb_fwd_kernel(const float* __restrict__ flat, long flat_len,
                                                                 const SedtReverbJob* __restrict__ jobs, long dst_len,
                                                                 float* __restrict__ ws, long ws_len, const int64_t* __restrict__ tab, int R,
                                                                 long n_parts, const float* __restrict__ twiddle, int N,
                                                                 int32_t* __restrict__ status) {
  extern __shared__ float rv_lds[];
  const int M = N / 2, H = N / 2, K = N / 2 + 1, Bs = N / 2;
  const int e = blockIdx.y, tid = threadIdx.x;
  const long j0 = (long)blockIdx.x * ST_FPB;
  const SedtReverbJob job = jobs[e];
  RvRir rir;
  const bool ok = rv_job_ok(job, N, flat_len, dst_len, ws_len, tab, R, n_parts, &rir);
  if (blockIdx.x == 0 && tid == 0) status[e] = ok ? 0 : 2;
  if (!ok) return;
  const long n = job.n, nb = rv_blocks_in(N, n);
  if (j0 >= nb) return;                    // (uniform over the workgroup)
  float* twr = rv_lds;
  float* twi = rv_lds + (H + 1);
  float* frames = rv_lds + 2 * (H + 1);
  for (int i = tid; i < 2 * (H + 1); i += ST_THREADS) rv_lds[i] = twiddle[i];
  const float* __restrict__ x = flat + job.src_off;
  // ---- load, fade, pack: block j covers samples (j - 1) Bs .. (j + 1) Bs - 1, zero outside [0, n)
  for (int idx = tid; idx < ST_FPB * M; idx += ST_THREADS) {
    const int f = idx / M, k = idx - f * M;
    const long j = j0 + f;
    float v[2] = {0.f, 0.f};
    if (j < nb) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const long q = (j - 1) * Bs + 2 * k + c;
        if (q >= 0 && q < n) v[c] = x[q] * rv_fade(q, n, job.fade);
      }
    }
    float* re = frames + (long)f * 4 * M;
    re[k] = v[0];
    re[M + k] = v[1];
  }
  __syncthreads();
  float* xre = ws + job.ws_off;
  rv_forward(frames, twr, twi, N, tid, xre, xre + nb * K, j0, nb);
}

template <int N, int G>
__global__ __launch_bounds__(ST_THREADS) void reverb_mac_kernel(const SedtReverbJob* __restrict__ jobs, long flat_len, float* __restrict__ dst,
                                                                 long dst_len, const float* __restrict__ ws, long ws_len,
                                                                 const float* __restrict__ hre, const float* __restrict__ him, long n_parts,
                                                                 const int64_t* __restrict__ tab, int R,
                                                                 const float* __restrict__ twiddle) {
  extern __shared__ float rv_lds[];
  constexpr int M = N / 2, H = N / 2, K = N / 2 + 1, Bs = N / 2;
  constexpr int NB = (K + ST_THREADS - 1) / ST_THREADS;                    // bins per thread: k = tid + s ST_THREADS
  const int e = blockIdx.y, tid = threadIdx.x;
  const long j0 = (long)blockIdx.x * G;
  const SedtReverbJob job = jobs[e];
  RvRir rir;
  if (!rv_job_ok(job, N, flat_len, dst_len, ws_len, tab, R, n_parts, &rir)) return;
  const long total = job.n + rir.L - 1, nout = (total + Bs - 1) / Bs;
  if (j0 >= nout) return;                  // (uniform over the workgroup)
  const long nb = rv_blocks_in(N, job.n), P = (rir.L + Bs - 1) / Bs;
  float* twr = rv_lds;
  float* twi = rv_lds + (H + 1);
  float* frames = rv_lds + 2 * (H + 1);
  for (int i = tid; i < 2 * (H + 1); i += ST_THREADS) rv_lds[i] = twiddle[i];
  const float* __restrict__ xre = ws + job.ws_off;
  const float* __restrict__ xim = xre + nb * K;
  const float* __restrict__ hr = hre + rir.part * K;
  const float* __restrict__ hi = him + rir.part * K;
  // ---- the products.  Step p multiplies H[p] into the G accumulators, block j0 + g with X[j0 + g - p]: the window of G input
  //      spectra moves down by one block per step.  Blocks outside [0, nb) are zero, so the steps whose whole window is are skipped.
  float ar[G][NB], ai[G][NB], wr[G][NB], wi[G][NB];
  const auto load_x = [&](long i, float* re, float* im) {
    const bool in = i >= 0 && i < nb;      // (uniform over the workgroup)
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      const int k = tid + s * ST_THREADS;
      const bool on = in && k < K;
      re[s] = on ? xre[i * K + k] : 0.f;
      im[s] = on ? xim[i * K + k] : 0.f;
    }
  };
  const long p_lo = j0 - nb + 1 > 0 ? j0 - nb + 1 : 0, p_hi = P - 1 < j0 + G - 1 ? P - 1 : j0 + G - 1;
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int s = 0; s < NB; ++s) ar[g][s] = ai[g][s] = 0.f;
    load_x(j0 + g - p_lo, wr[g], wi[g]);
  }
  for (long p = p_lo; p <= p_hi; ++p) {
    float cr[NB], ci[NB], nr[NB], ni[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      const int k = tid + s * ST_THREADS;
      cr[s] = k < K ? hr[p * K + k] : 0.f;
      ci[s] = k < K ? hi[p * K + k] : 0.f;
    }
    load_x(p < p_hi ? j0 - p - 1 : -1, nr, ni);      // the block that enters the window for step p + 1 (none behind the last)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int s = 0; s < NB; ++s) {
        // four fused multiply-adds, written out: what the compiler contracts on its own may differ from one G to the next
        ar[g][s] = fmaf(-wi[g][s], ci[s], fmaf(wr[g][s], cr[s], ar[g][s]));
        ai[g][s] = fmaf(wi[g][s], cr[s], fmaf(wr[g][s], ci[s], ai[g][s]));
      }
#pragma unroll
    for (int g = G - 1; g > 0; --g)
#pragma unroll
      for (int s = 0; s < NB; ++s) wr[g][s] = wr[g - 1][s], wi[g][s] = wi[g - 1][s];
#pragma unroll
    for (int s = 0; s < NB; ++s) wr[0][s] = nr[s], wi[0][s] = ni[s];
  }
  // ---- the inverse, ST_FPB blocks at a time: Y to buffer 1 of its frame (the real part of bin M in the slot of bin 0's imaginary
  //      part, which the packed transform drops), packed into buffer 0, the forward FFT of conj Z = M conj z
  const float inv = 1.0f / (float)M;                                        // a power of two: exact
  float* __restrict__ y = dst + job.dst_off;
#pragma unroll
  for (int g0 = 0; g0 < G; g0 += ST_FPB) {
    __syncthreads();                       // the twiddles are staged; the previous round's frames are read
#pragma unroll
    for (int f = 0; f < ST_FPB; ++f) {
      if (g0 + f >= G) continue;
      float* sr = frames + (long)f * 4 * M + 2 * M;
      float* si = sr + M;
#pragma unroll
      for (int s = 0; s < NB; ++s) {
        const int k = tid + s * ST_THREADS;
        if (k < M) {
          sr[k] = ar[g0 + f][s];
          if (k > 0) si[k] = ai[g0 + f][s];
        } else if (k == M) {
          si[0] = ar[g0 + f][s];
        }
      }
    }
    __syncthreads();
    // pack: E[k] = (Y[k] + conj Y[M-k]) / 2, O[k] = (Y[k] - conj Y[M-k]) / 2 * conj W[k], Z[k] = E[k] + i O[k]
    for (int idx = tid; idx < ST_FPB * M; idx += ST_THREADS) {
      const int f = idx / M, k = idx - f * M;
      float zr = 0.f, zi = 0.f;
      if (g0 + f < G && j0 + g0 + f < nout) {
        const float* sr = frames + (long)f * 4 * M + 2 * M;
        const float* si = sr + M;
        const scf32 xk{sr[k], k == 0 ? 0.f : si[k]};
        const scf32 xm{k == 0 ? si[0] : sr[M - k], k == 0 ? 0.f : -si[M - k]};
        const scf32 ev{0.5f * (xk.re + xm.re), 0.5f * (xk.im + xm.im)}, od{0.5f * (xk.re - xm.re), 0.5f * (xk.im - xm.im)};
        const float cw = twr[k], sw = -twi[k];                             // conj W[k]
        const scf32 o{od.re * cw - od.im * sw, od.re * sw + od.im * cw};
        zr = ev.re - o.im;
        zi = -(ev.im + o.re);
      }
      float* re = frames + (long)f * 4 * M;
      re[k] = zr;
      re[M + k] = zi;
    }
    __syncthreads();
    const int pb = st_fft(frames, twr, twi, N, tid);
    // the last Bs samples of frame j are wet[j Bs, (j + 1) Bs): sample Bs + 2 i + c of the frame is in z[M / 2 + i]
    for (int idx = tid; idx < ST_FPB * (M / 2); idx += ST_THREADS) {
      const int f = idx / (M / 2), i = idx - f * (M / 2);
      const long j = j0 + g0 + f;
      if (g0 + f >= G || j >= nout) continue;
      const float* xr = frames + (long)f * 4 * M + pb * 2 * M;
      const float* xi = xr + M;
      const long q = j * Bs + 2 * i;
      if (q < total) y[q] = xr[M / 2 + i] * inv;
      if (q + 1 < total) y[q + 1] = -xi[M / 2 + i] * inv;
    }
  }
}

// the tails of a clip's wet events over its background (include/sedt_hip.h: sedt_reverb_bed); one thread per sample
__global__ __launch_bounds__(RV_BED_THREADS) void reverb_bed_kernel(const float* flat, long flat_len, const int64_t* __restrict__ src_off,
                                                                     const int64_t* __restrict__ src_len, int n_src,
                                                                     const SedtReverbBed* __restrict__ beds,
                                                                     const SedtReverbTail* __restrict__ tails, int n_tails, long window,
                                                                     float* dst, long dst_len) {
#pragma clang fp contract(off)             // g * x, acc + ...: every float32 operation of the definition is rounded on its own
  const SedtReverbBed bed = beds[blockIdx.y];
  const long t = (long)blockIdx.x * RV_BED_THREADS + threadIdx.x;
  if (t >= window || bed.dst_off < 0 || bed.dst_off > dst_len || window > dst_len - bed.dst_off) return;
  float acc = 0.0f;
  if (bed.src >= 0 && bed.src < n_src) {
    const long off = (long)src_off[bed.src], len = (long)src_len[bed.src];
    if (off >= 0 && len >= 1 && off <= flat_len && len <= flat_len - off && bed.start >= 0 && bed.start < len)
      acc = bed.gain * flat[off + (bed.start % len + t % len) % len];
  }
  const int lo = bed.tail_lo < 0 ? 0 : bed.tail_lo, hi = bed.tail_hi > n_tails ? n_tails : bed.tail_hi;
  for (int k = lo; k < hi; ++k) {                                           // plan order
    const SedtReverbTail tl = tails[k];
    if (tl.wet_off < 0 || tl.head < 0 || tl.total < tl.head || tl.wet_off > flat_len || tl.total > flat_len - tl.wet_off || tl.onset < 0)
      continue;
    const long i = t - tl.onset;
    if (i >= tl.head && i < tl.total) acc = acc + (tl.gain * flat[tl.wet_off + i]);
  }
  dst[bed.dst_off + t] = acc;
}

// the host half of the entry points: one pass over the HOST copy of the RIR table (the responses' partitions lie behind one another)
static int rv_check_rirs(const char* who, const int64_t* tab, int R, int N, int64_t n_parts, int64_t taps_len, int* maxP) {
  int64_t part = 0;
  *maxP = 0;
  for (int r = 0; r < R; ++r) {
    const int64_t L = tab[r];
    SEDT_REQUIRE(L >= 1 && L <= (int64_t)SEDT_REVERB_MAXPART * (N / 2),
                 "%s: response %d has %lld taps (1 .. %d partitions of n_fft / 2 = %d: at most %lld)", who, r, (long long)L,
                 SEDT_REVERB_MAXPART, N / 2, (long long)SEDT_REVERB_MAXPART * (N / 2));
    SEDT_REQUIRE(tab[R + r] == part, "%s: response %d starts at partition %lld: the responses' partitions lie behind one another (%lld)", who,
                 r, (long long)tab[R + r], (long long)part);
    if (taps_len >= 0)
      SEDT_REQUIRE(tab[2 * R + r] >= 0 && tab[2 * R + r] <= taps_len && L <= taps_len - tab[2 * R + r],
                   "%s: response %d (taps %lld .. +%lld) does not lie inside the %lld taps given", who, r, (long long)tab[2 * R + r],
                   (long long)L, (long long)taps_len);
    const int P = (int)((L + N / 2 - 1) / (N / 2));
    part += P;
    if (P > *maxP) *maxP = P;
  }
  SEDT_REQUIRE(part == n_parts, "%s: n_parts=%lld, the responses have %lld partitions", who, (long long)n_parts, (long long)part);
  return 0;
}

static int rv_check_jobs(const SedtReverbJob* jobs, int E, int N, const int64_t* tab, int R, int64_t* need_floats, int64_t* max_nb,
                         int64_t* max_nout) {
  int64_t end = 0;
  *max_nb = *max_nout = 0;
  for (int e = 0; e < E; ++e) {
    const SedtReverbJob& j = jobs[e];
    SEDT_REQUIRE(j.n >= 1, "reverb: job %d has n=%lld samples (n >= 1)", e, (long long)j.n);
    if (tab) SEDT_REQUIRE(j.rir >= 0 && j.rir < R, "reverb: job %d names response %d of %d", e, j.rir, R);
    const int64_t L = tab ? tab[j.rir] : 1;
    SEDT_REQUIRE(rv_shape_ok(N, j.n, L, j.fade),
                 "reverb: job %d (n=%lld fade=%d, %lld taps) is outside the envelope: 1 <= n <= 2^26; 0 <= fade <= 2^26; 1 <= taps <= %d "
                 "n_fft / 2", e, (long long)j.n, j.fade, (long long)L, SEDT_REVERB_MAXPART);
    SEDT_REQUIRE(j.ws_off >= end && (j.ws_off & 3) == 0,
                 "reverb: job %d has ws_off=%lld: the regions are multiples of 4 floats, in job order, behind one another (>= %lld)", e,
                 (long long)j.ws_off, (long long)end);
    end = j.ws_off + rv_job_floats(N, j.n);
    const int64_t nb = rv_blocks_in(N, j.n), nout = (j.n + L - 1 + N / 2 - 1) / (N / 2);
    if (nb > *max_nb) *max_nb = nb;
    if (nout > *max_nout) *max_nout = nout;
  }
  *need_floats = end;
  return 0;
}

template <int N, int G>
static void rv_launch_mac(dim3 grid, size_t lds, hipStream_t s, const SedtReverbJob* jobs, long flat_len, float* dst, long dst_len,
                          const float* ws, long ws_len, const float* hre, const float* him, long n_parts, const int64_t* tab, int R,
                          const float* twiddle) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_mac_kernel<N, G>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL((reverb_mac_kernel<N, G>), grid, dim3(ST_THREADS), lds, s, jobs, flat_len, dst, dst_len, ws, ws_len, hre, him, n_parts,
                     tab, R, twiddle);
}

template <int N, typename... A>
static void rv_launch_mac_g(int G, int64_t max_nout, unsigned E, A... a) {
  const dim3 grid((unsigned)((max_nout + G - 1) / G), E);
  switch (G) {
    case 1: rv_launch_mac<N, 1>(grid, a...); break;
    case 2: rv_launch_mac<N, 2>(grid, a...); break;
    case 8: rv_launch_mac<N, 8>(grid, a...); break;
    default: rv_launch_mac<N, 4>(grid, a...); break;
  }
}

}  // namespace sedt

extern "C" int sedt_reverb_ok(int n_fft, int64_t n, int64_t taps, int fade) {
  return sedt::rv_shape_ok(n_fft, (long)n, (long)taps, (long)fade) ? 1 : 0;
}

extern "C" int64_t sedt_reverb_workspace(const SedtReverbJob* jobs, int n_jobs, int n_fft) {
  using namespace sedt;
  if (!jobs || n_jobs < 0 || !(n_fft == 512 || n_fft == 1024 || n_fft == 2048)) {
    set_error("reverb_workspace: null pointer, n_jobs=%d < 0 or n_fft=%d (512, 1024 or 2048)", n_jobs, n_fft);
    return -1;
  }
  int64_t need, nb, nout;
  if (rv_check_jobs(jobs, n_jobs, n_fft, nullptr, 0, &need, &nb, &nout)) return -1;
  return need * (int64_t)sizeof(float);
}

extern "C" int sedt_reverb_spectra(const float* taps, int64_t taps_len, const int64_t* rir_tab_host, const int64_t* rir_tab_dev, int n_rirs,
                                   float* h_re, float* h_im, int64_t n_parts, const float* twiddle, int n_fft, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "reverb_spectra: n_fft=%d (512, 1024 or 2048)", n_fft);
  SEDT_REQUIRE(n_rirs >= 1 && n_rirs <= 65535 && taps_len >= 1 && n_parts >= 1,
               "reverb_spectra: n_rirs=%d (1 .. 65535) taps_len=%lld n_parts=%lld (both >= 1)", n_rirs, (long long)taps_len, (long long)n_parts);
  SEDT_REQUIRE(taps && rir_tab_host && rir_tab_dev && h_re && h_im && twiddle, "reverb_spectra: null pointer");
  int maxP;
  if (rv_check_rirs("reverb_spectra", rir_tab_host, n_rirs, n_fft, n_parts, taps_len, &maxP)) return 1;
  const size_t lds = (2 * (size_t)(n_fft / 2 + 1) + (size_t)ST_FPB * 2 * n_fft) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_spectra_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipLaunchKernelGGL(reverb_spectra_kernel, dim3((unsigned)((maxP + ST_FPB - 1) / ST_FPB), (unsigned)n_rirs), dim3(ST_THREADS), lds,
                     reinterpret_cast<hipStream_t>(stream), taps, (long)taps_len, rir_tab_dev, n_rirs, h_re, h_im, (long)n_parts, twiddle,
                     n_fft);
  return check_launch("reverb_spectra");
}

extern "C" int sedt_reverb(const float* flat, int64_t flat_len, const SedtReverbJob* jobs_host, const SedtReverbJob* jobs_dev, int n_jobs,
                           float* dst, int64_t dst_len, void* workspace, int64_t workspace_bytes, const float* h_re, const float* h_im,
                           int64_t n_parts, const int64_t* rir_tab_host, const int64_t* rir_tab_dev, int n_rirs, const float* twiddle,
                           int n_fft, int group, int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "reverb: n_fft=%d (512, 1024 or 2048)", n_fft);
  SEDT_REQUIRE(n_jobs >= 0 && flat_len >= 0 && dst_len >= 0 && workspace_bytes >= 0,
               "reverb: n_jobs=%d flat_len=%lld dst_len=%lld workspace_bytes=%lld (none may be negative)", n_jobs, (long long)flat_len,
               (long long)dst_len, (long long)workspace_bytes);
  SEDT_REQUIRE(n_jobs <= 65535, "reverb: n_jobs=%d (at most 65535 per call)", n_jobs);
  SEDT_REQUIRE(n_rirs >= 1 && n_rirs <= 65535 && n_parts >= 1, "reverb: n_rirs=%d (1 .. 65535) n_parts=%lld (>= 1)", n_rirs,
               (long long)n_parts);
  SEDT_REQUIRE(group == 0 || group == 1 || group == 2 || group == 4 || group == 8,
               "reverb: group=%d output blocks per workgroup (0: the default, or 1, 2, 4, 8)", group);
  SEDT_REQUIRE(flat && jobs_host && jobs_dev && dst && workspace && h_re && h_im && rir_tab_host && rir_tab_dev && twiddle && status,
               "reverb: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(jobs_dev) & 7) == 0,
               "reverb: the workspace is 16-byte aligned, the records 8-byte aligned");
  int maxP;
  if (rv_check_rirs("reverb", rir_tab_host, n_rirs, n_fft, n_parts, -1, &maxP)) return 1;
  int64_t need, max_nb, max_nout;
  if (rv_check_jobs(jobs_host, n_jobs, n_fft, rir_tab_host, n_rirs, &need, &max_nb, &max_nout)) return 1;
  SEDT_REQUIRE(need * (int64_t)sizeof(float) <= workspace_bytes,
               "reverb: workspace_bytes=%lld is too small: the jobs need %lld (sedt_reverb_workspace)", (long long)workspace_bytes,
               (long long)(need * (int64_t)sizeof(float)));
  if (n_jobs == 0) return 0;
  const long ws_len = (long)(workspace_bytes / (int64_t)sizeof(float));
  float* ws = reinterpret_cast<float*>(workspace);
  const size_t lds = (2 * (size_t)(n_fft / 2 + 1) + (size_t)ST_FPB * 2 * n_fft) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(reverb_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned E = (unsigned)n_jobs;
  hipLaunchKernelGGL(reverb_fwd_kernel, dim3((unsigned)((max_nb + ST_FPB - 1) / ST_FPB), E), dim3(ST_THREADS), lds, s, flat, (long)flat_len,
                     jobs_dev, (long)dst_len, ws, ws_len, rir_tab_dev, n_rirs, (long)n_parts, twiddle, n_fft, status);
  const int G = group ? group : RV_G_DEFAULT;
  if (n_fft == 512)
    rv_launch_mac_g<512>(G, max_nout, E, lds, s, jobs_dev, (long)flat_len, dst, (long)dst_len, (const float*)ws, ws_len, h_re, h_im,
                         (long)n_parts, rir_tab_dev, n_rirs, twiddle);
  else if (n_fft == 1024)
    rv_launch_mac_g<1024>(G, max_nout, E, lds, s, jobs_dev, (long)flat_len, dst, (long)dst_len, (const float*)ws, ws_len, h_re, h_im,
                          (long)n_parts, rir_tab_dev, n_rirs, twiddle);
  else
    rv_launch_mac_g<2048>(G, max_nout, E, lds, s, jobs_dev, (long)flat_len, dst, (long)dst_len, (const float*)ws, ws_len, h_re, h_im,
                          (long)n_parts, rir_tab_dev, n_rirs, twiddle);
  return check_launch("reverb");
}

extern "C" int sedt_reverb_bed(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                               const SedtReverbBed* beds, int n_beds, const SedtReverbTail* tails, int n_tails, int64_t window, float* dst,
                               int64_t dst_len, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_src >= 1 && n_beds >= 0 && n_beds <= 65535 && n_tails >= 0 && flat_len >= 0 && dst_len >= 0 && window >= 1 &&
                   window < (1LL << 31),
               "reverb_bed: n_src=%d (>= 1) n_beds=%d (0 .. 65535) n_tails=%d flat_len=%lld dst_len=%lld (none negative) window=%lld (1 .. "
               "2^31 - 1)", n_src, n_beds, n_tails, (long long)flat_len, (long long)dst_len, (long long)window);
  SEDT_REQUIRE(flat && src_off && src_len && beds && tails && dst, "reverb_bed: null pointer");
  if (n_beds == 0) return 0;
  hipLaunchKernelGGL(reverb_bed_kernel, dim3((unsigned)((window + RV_BED_THREADS - 1) / RV_BED_THREADS), (unsigned)n_beds),
                     dim3(RV_BED_THREADS), 0, reinterpret_cast<hipStream_t>(stream), flat, (long)flat_len, src_off, src_len, n_src, beds, tails,
                     n_tails, (long)window, dst, (long)dst_len);
  return check_launch("reverb_bed");
}
