// stretch.hip - time stretch and pitch shift of E excerpts of a staged sound bank: a phase vocoder followed by band-limited
// resampling at a real ratio (utilities/stretch.py; DESIGN.md section 4, "Pitch shift and time stretch on the device";
// tests/stretch_ref.py restates the definition in float64).  The reference has no counterpart: its corpora were generated offline.
//
// Per job (SedtStretchJob, include/sedt_hip.h): x = flat[src_off .. src_off + n), rate r = 1 / (factor * alpha), alpha = 2^(p / 12).
// Five launches behind one another on the stream, each over all E jobs (grid y = the job):
//   stretch_stft_kernel   ST_FPB frames per workgroup in LDS: periodic Hann window, the packed real FFT of mel.hip (Stockham radix 4,
//                         separate re / im arrays), D[t][k] to the workspace; workgroup (0, e) also writes status[e]
//   stretch_voc_kernel    one thread per (job, bin) walks the output frames in order: the phase in float64, atan2 / sincos in float64
//   stretch_ifft_kernel   ST_FPB synthesis frames per workgroup: the packed inverse real FFT, times the window, to the workspace
//   stretch_ola_kernel    one thread per sample of z: its at most four frames added in ascending frame order, over the window sum
//   stretch_resample_kernel  one thread per sample of y: the Kaiser-sinc taps in ascending j, the filter interpolated linearly in a
//                         table of 512 points per zero crossing, staged in LDS (32 KB for kaiser_fast, 128 KB for kaiser_best: one
//                         workgroup of 1024 per CU, the table loaded once per 2048 outputs)
// No atomics anywhere, no allocation, no synchronisation: the same call gives the same bits.  r == 1 skips the first four (z = x, one
// copy in the ola kernel), alpha == 1 makes the last a copy (y = z).
// Every kernel re-checks its DEVICE record (st_job_ok) before it touches memory: a record outside the bank, the destination or the
// workspace raises status 2 and nothing is read or written for it.  The loops are bounded by the record's own T, U, m1, m, which the
// check ties to the workspace region, so a record that differs from the host copy the entry point saw cannot walk out of a buffer.
// LDS: (2 (N/2 + 1) + ST_FPB * 2 N) * 4 bytes = 72 KB at N = 2048 (two workgroups per CU), as mel_kernel.
#include "common.h"
#include "fft_lds.h"

#include <math.h>

namespace sedt {

constexpr int ST_VOC_THREADS = 64;
constexpr int ST_TABLE_RES = 512;       // table points per zero crossing of the resampling filter
constexpr int ST_RES_THREADS = 1024;    // the resampler's workgroup: the table in LDS is loaded once per ST_RES_PER_WG outputs
constexpr int ST_RES_PER_WG = 2048;
constexpr long ST_MAX_N = 1L << 26;
constexpr float ST_WS_MIN = 1e-8f;      // the overlap-add divides where the window sum exceeds this

__host__ __device__ inline long st_job_floats(int N, long m1, int T, int U) {
  const long K = N / 2 + 1;
  const long f = 2L * T * K + 2L * U * K + (long)U * N + m1;
  return (f + 3) & ~3L;
}

// what both the entry point (on the host copy) and every kernel (on the device copy) ask of a record, the buffers aside
__host__ __device__ inline bool st_shape_ok(int N, long n, long m, long m1, double r, double alpha, int T, int U) {
  if (!(N == 512 || N == 1024 || N == 2048)) return false;
  if (!(n >= 1 && n <= ST_MAX_N)) return false;
  if (!(alpha >= 0.5 && alpha <= 2.0 && r >= 0.25 && r <= 4.0)) return false;               // (NaN fails)
  const double f = 1.0 / (r * alpha);
  if (!(f >= 0.5 * (1.0 - 1e-12) && f <= 2.0 * (1.0 + 1e-12))) return false;
  if (!(m >= 1 && m1 >= 0 && fabs((double)m - (double)n * f) <= 1.0 && fabs((double)m1 - (double)n / r) <= 1.0)) return false;
  if (alpha == 1.0 && m != m1) return false;
  if (r == 1.0) return T == 0 && U == 0 && m1 == n;
  const int hop = N / 4;
  if (T != 1 + (int)(n / hop) || U < 1) return false;
  // U = the number of steps u with fl64(u r) < T
  return (double)(U - 1) * r < (double)T && (double)U * r >= (double)T;
}

__device__ __forceinline__ bool st_job_ok(const SedtStretchJob& j, int N, long flat_len, long dst_len, long ws_len) {
  if (!st_shape_ok(N, j.n, j.m, j.m1, j.r, j.alpha, j.T, j.U)) return false;
  if (j.src_off < 0 || j.src_off > flat_len || j.n > flat_len - j.src_off) return false;
  if (j.dst_off < 0 || j.dst_off > dst_len || j.m > dst_len - j.dst_off) return false;
  if (j.ws_off < 0 || (j.ws_off & 3) || j.ws_off > ws_len || st_job_floats(N, j.m1, j.T, j.U) > ws_len - j.ws_off) return false;
  return true;
}

// the regions of a job's workspace (floats from ws + ws_off): D re [T][K] | D im | S re [U][K] | S im | frames [U][N] | z [m1]
struct StRegions {
  float *dre, *dim, *sre, *sim, *frames, *z;
};
__device__ __forceinline__ StRegions st_regions(float* ws, const SedtStretchJob& j, int N) {
  const long K = N / 2 + 1;
  StRegions g;
  g.dre = ws + j.ws_off;
  g.dim = g.dre + (long)j.T * K;
  g.sre = g.dim + (long)j.T * K;
  g.sim = g.sre + (long)j.U * K;
  g.frames = g.sim + (long)j.U * K;
  g.z = g.frames + (long)j.U * N;
  return g;
}


__global__ __launch_bounds__(ST_THREADS) void stretch_stft_kernel(const float* __restrict__ flat, long flat_len,
                                                                   const SedtStretchJob* __restrict__ jobs, long dst_len,
                                                                   float* __restrict__ ws, long ws_len,
                                                                   const float* __restrict__ window,
                                                                   const float* __restrict__ twiddle, int N,
                                                                   int32_t* __restrict__ status) {
  extern __shared__ float st_lds[];
  const int M = N / 2, H = N / 2, K = N / 2 + 1, hop = N / 4;
  const int e = blockIdx.y, t0 = blockIdx.x * ST_FPB, tid = threadIdx.x;
  const SedtStretchJob job = jobs[e];
  const bool ok = st_job_ok(job, N, flat_len, dst_len, ws_len);
  if (blockIdx.x == 0 && tid == 0) status[e] = ok ? 0 : 2;
  if (!ok || t0 >= job.T) return;          // (uniform over the workgroup; T == 0: the vocoder is skipped)
  float* twr = st_lds;                     // [H + 1] cos
  float* twi = st_lds + (H + 1);           // [H + 1] -sin
  float* frames = st_lds + 2 * (H + 1);    // [ST_FPB][2 buffers][re M | im M]
  for (int i = tid; i < 2 * (H + 1); i += ST_THREADS) st_lds[i] = twiddle[i];
  const float* __restrict__ x = flat + job.src_off;
  const long n = job.n;
  // ---- load, window, pack: frame t covers samples t hop - N/2 .. t hop + N/2 - 1, zero outside [0, n)
  for (int idx = tid; idx < ST_FPB * M; idx += ST_THREADS) {
    const int f = idx / M, k = idx - f * M, t = t0 + f;
    float v[2] = {0.f, 0.f};
    if (t < job.T) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int i = 2 * k + c;
        const long j = (long)t * hop + i - H;
        if (j >= 0 && j < n) v[c] = x[j] * window[i];
      }
    }
    float* re = frames + (long)f * 4 * M;
    re[k] = v[0];
    re[M + k] = v[1];
  }
  __syncthreads();
  const int p = st_fft(frames, twr, twi, N, tid);
  // ---- split the packed spectrum into bins 0 .. M:  X[k] = (Z[k] + conj Z[M-k]) / 2 + W[k] (Z[k] - conj Z[M-k]) / (2i)
  const StRegions g = st_regions(ws, job, N);
  for (int idx = tid; idx < ST_FPB * K; idx += ST_THREADS) {
    const int f = idx / K, k = idx - f * K, t = t0 + f;
    if (t >= job.T) continue;
    const float* xr = frames + (long)f * 4 * M + p * 2 * M;
    const float* xi = xr + M;
    const int ka = k & (M - 1), kb = (M - k) & (M - 1);
    const scf32 zk{xr[ka], xi[ka]}, zm{xr[kb], -xi[kb]};
    const scf32 s = zk + zm, d = zk - zm;
    const scf32 o{0.5f * d.im, -0.5f * d.re};                              // (zk - zm) / 2i
    const float wr = twr[k], wi = twi[k];
    g.dre[(long)t * K + k] = 0.5f * s.re + (o.re * wr - o.im * wi);
    g.dim[(long)t * K + k] = 0.5f * s.im + (o.re * wi + o.im * wr);
  }
}

__device__ __forceinline__ double st_arg(double re, double im) { return (re == 0.0 && im == 0.0) ? 0.0 : atan2(im, re); }

__global__ __launch_bounds__(ST_VOC_THREADS) void stretch_voc_kernel(const SedtStretchJob* __restrict__ jobs, long flat_len, long dst_len,
                                                                      float* __restrict__ ws, long ws_len, int N) {
  const int K = N / 2 + 1, hop = N / 4;
  const int e = blockIdx.y, k = blockIdx.x * ST_VOC_THREADS + threadIdx.x;
  const SedtStretchJob job = jobs[e];
  if (!st_job_ok(job, N, flat_len, dst_len, ws_len) || job.T == 0 || k >= K) return;
  const StRegions g = st_regions(ws, job, N);
  const double two_pi = 6.283185307179586476925286766559;
  const double omega = (two_pi * (double)hop * (double)k) / (double)N;
  const int T = job.T;
  double phi = st_arg((double)g.dre[k], (double)g.dim[k]);
  for (int u = 0; u < job.U; ++u) {
    const double s = __dmul_rn((double)u, job.r);                          // ONE float64 product: never fused into what follows
    const double fl = floor(s);
    const double a = s - fl;
    const long i = (long)fl;
    double r0 = 0.0, i0 = 0.0, r1 = 0.0, i1 = 0.0;                         // frames T and T + 1 are zero
    if (i >= 0 && i < T) r0 = (double)g.dre[i * K + k], i0 = (double)g.dim[i * K + k];
    if (i + 1 >= 0 && i + 1 < T) r1 = (double)g.dre[(i + 1) * K + k], i1 = (double)g.dim[(i + 1) * K + k];
    const double mag = (1.0 - a) * sqrt(r0 * r0 + i0 * i0) + a * sqrt(r1 * r1 + i1 * i1);
    double sn, cs;
    sincos(phi, &sn, &cs);
    g.sre[(long)u * K + k] = (float)(mag * cs);
    g.sim[(long)u * K + k] = (float)(mag * sn);
    double d = st_arg(r1, i1) - st_arg(r0, i0) - omega;
    d = d - two_pi * rint(d / two_pi);
    phi = phi + (omega + d);
  }
}

__global__ __launch_bounds__(ST_THREADS) void stretch_ifft_kernel(const SedtStretchJob* __restrict__ jobs, long flat_len, long dst_len,
                                                                   float* __restrict__ ws, long ws_len,
                                                                   const float* __restrict__ window,
                                                                   const float* __restrict__ twiddle, int N) {
  extern __shared__ float st_lds[];
  const int M = N / 2, H = N / 2, K = N / 2 + 1;
  const int e = blockIdx.y, u0 = blockIdx.x * ST_FPB, tid = threadIdx.x;
  const SedtStretchJob job = jobs[e];
  if (!st_job_ok(job, N, flat_len, dst_len, ws_len) || u0 >= job.U) return;
  float* twr = st_lds;
  float* twi = st_lds + (H + 1);
  float* frames = st_lds + 2 * (H + 1);
  for (int i = tid; i < 2 * (H + 1); i += ST_THREADS) st_lds[i] = twiddle[i];
  __syncthreads();
  const StRegions g = st_regions(ws, job, N);
  // ---- pack: with X the Hermitian spectrum (the imaginary parts of bins 0 and M dropped), E[k] = (X[k] + conj X[M-k]) / 2,
  //      O[k] = (X[k] - conj X[M-k]) / 2 * conj W[k], Z[k] = E[k] + i O[k]; the forward FFT of conj Z is M conj z, z[j] = x[2j] + i x[2j+1]
  for (int idx = tid; idx < ST_FPB * M; idx += ST_THREADS) {
    const int f = idx / M, k = idx - f * M, u = u0 + f;
    float zr = 0.f, zi = 0.f;
    if (u < job.U) {
      const float* sr = g.sre + (long)u * K;
      const float* si = g.sim + (long)u * K;
      const scf32 xk{sr[k], k == 0 ? 0.f : si[k]};
      const scf32 xm{sr[M - k], k == 0 ? 0.f : -si[M - k]};
      const scf32 ev{0.5f * (xk.re + xm.re), 0.5f * (xk.im + xm.im)}, od{0.5f * (xk.re - xm.re), 0.5f * (xk.im - xm.im)};
      const float wr = twr[k], wi = -twi[k];                               // conj W[k]
      const scf32 o{od.re * wr - od.im * wi, od.re * wi + od.im * wr};
      zr = ev.re - o.im;
      zi = -(ev.im + o.re);
    }
    float* re = frames + (long)f * 4 * M;
    re[k] = zr;
    re[M + k] = zi;
  }
  __syncthreads();
  const int p = st_fft(frames, twr, twi, N, tid);
  const float inv = 1.0f / (float)M;                                        // a power of two: exact
  for (int idx = tid; idx < ST_FPB * M; idx += ST_THREADS) {
    const int f = idx / M, j = idx - f * M, u = u0 + f;
    if (u >= job.U) continue;
    const float* xr = frames + (long)f * 4 * M + p * 2 * M;
    const float* xi = xr + M;
    float* out = g.frames + (long)u * N;
    out[2 * j] = (xr[j] * inv) * window[2 * j];
    out[2 * j + 1] = (-xi[j] * inv) * window[2 * j + 1];
  }
}

__global__ __launch_bounds__(ST_THREADS) void stretch_ola_kernel(const float* __restrict__ flat, long flat_len,
                                                                  const SedtStretchJob* __restrict__ jobs, long dst_len,
                                                                  float* __restrict__ ws, long ws_len,
                                                                  const float* __restrict__ window, int N) {
  const int hop = N / 4;
  const int e = blockIdx.y;
  const SedtStretchJob job = jobs[e];
  const long idx = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (!st_job_ok(job, N, flat_len, dst_len, ws_len) || idx >= job.m1) return;
  const StRegions g = st_regions(ws, job, N);
  if (job.T == 0) {                                                         // r == 1: z = x
    g.z[idx] = flat[job.src_off + idx];
    return;
  }
  const long q = idx + N / 2;
  const long last = q / hop;
  const long u_lo = max(last - 3, 0L), u_hi = min(last, (long)job.U - 1);
  float acc = 0.f, wsum = 0.f;
  for (long u = u_lo; u <= u_hi; ++u) {                                     // ascending frame order
    const int j = (int)(q - u * hop);                                       // 0 <= j < N
    const float w = window[j];
    acc = acc + g.frames[u * N + j];
    wsum = wsum + w * w;
  }
  g.z[idx] = wsum > ST_WS_MIN ? acc / wsum : acc;
}

__global__ __launch_bounds__(ST_RES_THREADS) void stretch_resample_kernel(const SedtStretchJob* __restrict__ jobs, long flat_len,
                                                                           float* __restrict__ dst, long dst_len,
                                                                           float* __restrict__ ws, long ws_len,
                                                                           const float* __restrict__ wtab, int Z, int N) {
  extern __shared__ float st_tab[];                                         // the filter table: 512 Z + 1 values, w(q / 512)
  const int e = blockIdx.y, tid = threadIdx.x;
  const SedtStretchJob job = jobs[e];
  const long i0 = (long)blockIdx.x * ST_RES_PER_WG;
  const int points = Z * ST_TABLE_RES;
  if (!st_job_ok(job, N, flat_len, dst_len, ws_len) || i0 >= job.m) return;                 // (uniform over the workgroup)
  const float* __restrict__ z = st_regions(ws, job, N).z;
  float* __restrict__ y = dst + job.dst_off;
  if (job.alpha == 1.0) {                                                   // y = z
    for (long i = i0 + tid; i < min(i0 + ST_RES_PER_WG, job.m); i += ST_RES_THREADS) y[i] = z[i];
    return;
  }
  // lanes next to one another read the table 512 min(alpha, 1) points apart: from memory every lane would fetch a line of its own
  for (int q = tid; q <= points; q += ST_RES_THREADS) st_tab[q] = wtab[q];
  __syncthreads();
  const double sd = job.alpha > 1.0 ? 1.0 / job.alpha : 1.0;
  const float sf = (float)sd;
  const double half = (double)Z / sd;
  for (long i = i0 + tid; i < min(i0 + ST_RES_PER_WG, job.m); i += ST_RES_THREADS) {
    const double t = __dmul_rn((double)i, job.alpha);                       // ONE float64 product
    const long j_lo = max((long)ceil(t - half), 0L), j_hi = min((long)floor(t + half), job.m1 - 1);
    float acc = 0.f;
    double jd = (double)j_lo;                                               // (double)j without a 64-bit conversion per tap: exact
    for (long j = j_lo; j <= j_hi; ++j, jd += 1.0) {                        // ascending j
      const double pos = fabs(sd * (t - jd)) * (double)ST_TABLE_RES;
      const int q = (int)pos;
      if (q >= points) continue;                                            // |s (t - j)| >= Z: outside the filter
      const float frac = (float)(pos - (double)q);
      const float w = st_tab[q] + frac * (st_tab[q + 1] - st_tab[q]);
      acc = acc + (sf * w) * z[j];
    }
    y[i] = acc;
  }
}

// the host half of the entry points: one pass over the HOST copy of the records
static int st_check_jobs(const SedtStretchJob* jobs, int E, int N, int64_t* need_floats, int* maxT, int* maxU, int64_t* max_m,
                         int64_t* max_m1) {
  int64_t end = 0;
  *maxT = *maxU = 0;
  *max_m = *max_m1 = 0;
  for (int e = 0; e < E; ++e) {
    const SedtStretchJob& j = jobs[e];
    SEDT_REQUIRE(j.n >= 1, "stretch: job %d has n=%lld samples (n >= 1)", e, (long long)j.n);
    SEDT_REQUIRE(st_shape_ok(N, j.n, j.m, j.m1, j.r, j.alpha, j.T, j.U),
                 "stretch: job %d (n=%lld m=%lld m1=%lld r=%.17g alpha=%.17g T=%d U=%d) is outside the envelope: 1 <= n <= 2^26; "
                 "alpha = 2^(p/12) in [0.5, 2] (|p| <= 12); the duration factor 1 / (r alpha) in [0.5, 2]; m = round(n factor), "
                 "m1 = round(n / r), T = 1 + n div (n_fft / 4), U = the steps u with u r < T; r == 1: T = U = 0, m1 = n; alpha == 1: m = m1",
                 e, (long long)j.n, (long long)j.m, (long long)j.m1, j.r, j.alpha, j.T, j.U);
    SEDT_REQUIRE(j.ws_off >= end && (j.ws_off & 3) == 0,
                 "stretch: job %d has ws_off=%lld: the regions are multiples of 4 floats, in job order, behind one another (>= %lld)", e,
                 (long long)j.ws_off, (long long)end);
    end = j.ws_off + st_job_floats(N, j.m1, j.T, j.U);
    if (j.T > *maxT) *maxT = j.T;
    if (j.U > *maxU) *maxU = j.U;
    if (j.m > *max_m) *max_m = j.m;
    if (j.m1 > *max_m1) *max_m1 = j.m1;
  }
  *need_floats = end;
  return 0;
}

}  // namespace sedt

extern "C" int sedt_stretch_ok(int n_fft, int64_t n, int64_t m, int64_t m1, double r, double alpha, int T, int U) {
  return sedt::st_shape_ok(n_fft, (long)n, (long)m, (long)m1, r, alpha, T, U) ? 1 : 0;
}

extern "C" int64_t sedt_stretch_workspace(const SedtStretchJob* jobs, int n_jobs, int n_fft) {
  using namespace sedt;
  if (!jobs || n_jobs < 0 || !(n_fft == 512 || n_fft == 1024 || n_fft == 2048)) {
    set_error("stretch_workspace: null pointer, n_jobs=%d < 0 or n_fft=%d (512, 1024 or 2048)", n_jobs, n_fft);
    return -1;
  }
  int64_t need, mm, mm1;
  int mt, mu;
  if (st_check_jobs(jobs, n_jobs, n_fft, &need, &mt, &mu, &mm, &mm1)) return -1;
  return need * (int64_t)sizeof(float);
}

extern "C" int sedt_stretch(const float* flat, int64_t flat_len, const SedtStretchJob* jobs_host, const SedtStretchJob* jobs_dev,
                            int n_jobs, float* dst, int64_t dst_len, void* workspace, int64_t workspace_bytes, const float* window,
                            const float* twiddle, const float* wtab, int zero_crossings, int n_fft, int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(n_fft == 512 || n_fft == 1024 || n_fft == 2048, "stretch: n_fft=%d (512, 1024 or 2048)", n_fft);
  SEDT_REQUIRE(n_jobs >= 0 && flat_len >= 0 && dst_len >= 0 && workspace_bytes >= 0,
               "stretch: n_jobs=%d flat_len=%lld dst_len=%lld workspace_bytes=%lld (none may be negative)", n_jobs, (long long)flat_len,
               (long long)dst_len, (long long)workspace_bytes);
  SEDT_REQUIRE(n_jobs <= 65535, "stretch: n_jobs=%d (at most 65535 per call)", n_jobs);
  SEDT_REQUIRE(zero_crossings >= 1 && zero_crossings <= 64, "stretch: zero_crossings=%d (1 .. 64)", zero_crossings);
  SEDT_REQUIRE(flat && jobs_host && jobs_dev && dst && workspace && window && twiddle && wtab && status, "stretch: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(jobs_dev) & 7) == 0,
               "stretch: the workspace is 16-byte aligned, the records 8-byte aligned");
  int64_t need, max_m, max_m1;
  int maxT, maxU;
  if (st_check_jobs(jobs_host, n_jobs, n_fft, &need, &maxT, &maxU, &max_m, &max_m1)) return 1;
  SEDT_REQUIRE(need * (int64_t)sizeof(float) <= workspace_bytes,
               "stretch: workspace_bytes=%lld is too small: the jobs need %lld (sedt_stretch_workspace)", (long long)workspace_bytes,
               (long long)(need * (int64_t)sizeof(float)));
  if (n_jobs == 0) return 0;
  const long ws_len = (long)(workspace_bytes / (int64_t)sizeof(float));
  float* ws = reinterpret_cast<float*>(workspace);
  const int N = n_fft, K = N / 2 + 1;
  const size_t lds = (2 * (size_t)(N / 2 + 1) + (size_t)ST_FPB * 2 * N) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(stretch_stft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(stretch_ifft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(stretch_resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned E = (unsigned)n_jobs;
  const auto blocks = [](int64_t n, int per) { return (unsigned)(n < 1 ? 1 : (n + per - 1) / per); };
  // the STFT grid covers every job even when no job runs the vocoder: its workgroup (0, e) writes status[e]
  hipLaunchKernelGGL(stretch_stft_kernel, dim3(blocks(maxT, ST_FPB), E), dim3(ST_THREADS), lds, s, flat, (long)flat_len, jobs_dev,
                     (long)dst_len, ws, ws_len, window, twiddle, N, status);
  if (maxT > 0) {
    hipLaunchKernelGGL(stretch_voc_kernel, dim3(blocks(K, ST_VOC_THREADS), E), dim3(ST_VOC_THREADS), 0, s, jobs_dev, (long)flat_len,
                       (long)dst_len, ws, ws_len, N);
    hipLaunchKernelGGL(stretch_ifft_kernel, dim3(blocks(maxU, ST_FPB), E), dim3(ST_THREADS), lds, s, jobs_dev, (long)flat_len,
                       (long)dst_len, ws, ws_len, window, twiddle, N);
  }
  if (max_m1 > 0)
    hipLaunchKernelGGL(stretch_ola_kernel, dim3(blocks(max_m1, ST_THREADS), E), dim3(ST_THREADS), 0, s, flat, (long)flat_len, jobs_dev,
                       (long)dst_len, ws, ws_len, window, N);
  hipLaunchKernelGGL(stretch_resample_kernel, dim3(blocks(max_m, ST_RES_PER_WG), E), dim3(ST_RES_THREADS),
                     ((size_t)zero_crossings * ST_TABLE_RES + 1) * sizeof(float), s, jobs_dev, (long)flat_len, dst, (long)dst_len, ws, ws_len,
                     wtab, zero_crossings, N);
  return check_launch("stretch");
}
