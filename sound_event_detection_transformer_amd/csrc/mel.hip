// mel.hip - the log-mel front end up to the mel amplitudes (reference data_utils/SedData.py:195-217, load_and_compute_mel_spec with
// compute_log=False: librosa.stft(center=True, pad_mode='reflect', window=hamming) -> magnitude -> librosa.filters.mel(htk=False,
// norm=None) -> transpose), waveform in, (T, n_mels) f32 out, ONE launch per batch.
//
// A workgroup of 256 owns MEL_FPB consecutive frames of one clip; everything between the waveform and the mel values lives in LDS:
//   load     frame t covers padded samples [t hop, t hop + n_fft); padded index q is sample q - n_fft/2, reflected once at either end
//            (j < 0 -> -j, j >= n -> 2 (n - 1) - j).  Only the n_window samples under the centred window are read; the flanks are 0.
//            x[i] = sample * window[i] in f32 (int16 PCM: sample = x / 32768, exact).
//   pack     z[k] = x[2k] + i x[2k+1], k < M = n_fft/2: one M-point complex FFT does the work of the n_fft-point real one.
//   FFT      Stockham autosort, radix 4 with one radix-2 stage at the end when M is an odd power of two (n_fft = 1024), between two
//            buffers per frame - no bit reversal, reads at unit stride.  Real and imaginary parts are SEPARATE f32 arrays, so every
//            LDS access is a dword: the reads are conflict-free and the scattered writes (stride Ns) are 2-way at worst, which a
//            dword store does not pay for.  Twiddles come from the host's table W[t] = exp(-2 pi i t / n_fft), t = 0 .. n_fft/2
//            (float64 rounded to f32), staged in LDS; an exponent past n_fft/2 is W[t - n_fft/2] negated.
//   split    X[k] = (Z[k] + conj Z[M-k]) / 2 + W[k] (Z[k] - conj Z[M-k]) / (2i), k = 0 .. M (Z[M] = Z[0]); |X[k]| goes to the
//            buffer the last stage read from.
//   mel      thread (frame, band) walks its band's bins in index order from the CSR table (band_bin0, band_off, band_w): a
//            fixed-order fmaf chain, no atomics.
// A frame's bits depend on the clip, t and the tables alone - not on B, on the other clips or on out_rows.  Rows t >= nframes[b] are
// stored as 0.  LDS: (2 (n_fft/2 + 1) + MEL_FPB * 2 n_fft) * 4 bytes = 72.0 KB at n_fft 2048 (two workgroups per CU), 36 KB at 1024.
#include "common.h"

namespace sedt {

constexpr int MEL_THREADS = 256;
constexpr int MEL_FPB = 4;          // frames per workgroup

struct cf32 {
  float re, im;
};
__device__ __forceinline__ cf32 operator+(cf32 a, cf32 b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cf32 operator-(cf32 a, cf32 b) { return {a.re - b.re, a.im - b.im}; }
// a * W_N^u, u in [0, N): the table holds u <= H = N/2, the other half is its negative
__device__ __forceinline__ cf32 mul_tw(cf32 a, const float* twr, const float* twi, int u, int H) {
  const bool neg = u > H;
  const int i = neg ? u - H : u;
  const float wr = neg ? -twr[i] : twr[i], wi = neg ? -twi[i] : twi[i];
  return {a.re * wr - a.im * wi, a.re * wi + a.im * wr};
}

__device__ __forceinline__ float wave_value(const float* w, long j) { return w[j]; }
__device__ __forceinline__ float wave_value(const int16_t* w, long j) { return (float)w[j] * (1.0f / 32768.0f); }

template <typename WT>
__global__ __launch_bounds__(MEL_THREADS) void mel_kernel(const WT* __restrict__ wave, long wave_stride,
                                                          const int32_t* __restrict__ nsamples, float* __restrict__ out, int out_rows,
                                                          const float* __restrict__ window, const float* __restrict__ twiddle,
                                                          const int32_t* __restrict__ band_bin0, const int32_t* __restrict__ band_off,
                                                          const float* __restrict__ band_w, int n_weights, int n_fft, int n_window,
                                                          int hop, int n_mels) {
  extern __shared__ float mel_lds[];
  const int N = n_fft, M = N / 2, H = N / 2;
  float* twr = mel_lds;                    // [H + 1] cos
  float* twi = mel_lds + (H + 1);          // [H + 1] -sin
  float* frames = mel_lds + 2 * (H + 1);   // [MEL_FPB][2 buffers][re M | im M]
  const int b = blockIdx.y, t0 = blockIdx.x * MEL_FPB, tid = threadIdx.x;
  const int n = (int)min((long)max(nsamples[b], 1), wave_stride);          // never past the samples the batch holds
  const int nframes = 1 + n / hop;
  const int rows = min(MEL_FPB, out_rows - t0);
  float* dst = out + ((long)b * out_rows + t0) * n_mels;
  if (t0 >= nframes) {                     // (uniform over the workgroup) the padding rows of a shorter clip
    for (int i = tid; i < rows * n_mels; i += MEL_THREADS) dst[i] = 0.f;
    return;
  }
  for (int i = tid; i < 2 * (H + 1); i += MEL_THREADS) mel_lds[i] = twiddle[i];

  // ---- load, window, pack
  const int lpad = (N - n_window) / 2;
  const WT* src = wave + (long)b * wave_stride;
  for (int idx = tid; idx < MEL_FPB * M; idx += MEL_THREADS) {
    const int f = idx / M, k = idx - f * M, t = t0 + f;
    float v[2] = {0.f, 0.f};
    if (t < nframes) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * k + e;
        if (i >= lpad && i < lpad + n_window) {
          long j = (long)t * hop + i - H;
          if (j < 0) j = -j;
          if (j >= n) j = 2L * (n - 1) - j;
          j = min(max(j, 0L), (long)n - 1);                                // (a no-op inside the envelope n >= n_fft/2 + 1)
          v[e] = wave_value(src, j) * window[i];
        }
      }
    }
    float* re = frames + (long)f * 4 * M;
    re[k] = v[0];
    re[M + k] = v[1];
  }
  __syncthreads();

  // ---- M-point complex FFT: radix-4 Stockham stages, then a radix-2 one if M is an odd power of two
  int p = 0, Ns = 1;
  const int T4 = M / 4;
  for (; Ns * 4 <= M; Ns *= 4) {
    const int step = N / (4 * Ns);         // W_{4 Ns}^{r k} = W_N^{r k step}
    for (int idx = tid; idx < MEL_FPB * T4; idx += MEL_THREADS) {
      const int f = idx / T4, j = idx - f * T4, k = j & (Ns - 1);
      const float* xr = frames + (long)f * 4 * M + p * 2 * M;
      const float* xi = xr + M;
      float* yr = frames + (long)f * 4 * M + (p ^ 1) * 2 * M;
      float* yi = yr + M;
      cf32 u0{xr[j], xi[j]}, u1{xr[j + T4], xi[j + T4]}, u2{xr[j + 2 * T4], xi[j + 2 * T4]}, u3{xr[j + 3 * T4], xi[j + 3 * T4]};
      if (Ns > 1) {
        u1 = mul_tw(u1, twr, twi, k * step, H);
        u2 = mul_tw(u2, twr, twi, 2 * k * step, H);
        u3 = mul_tw(u3, twr, twi, 3 * k * step, H);
      }
      const cf32 a0 = u0 + u2, a1 = u0 - u2, a2 = u1 + u3, d = u1 - u3;
      const cf32 a3{d.im, -d.re};          // -i d
      const int j0 = ((j - k) << 2) + k;
      const cf32 y0 = a0 + a2, y1 = a1 + a3, y2 = a0 - a2, y3 = a1 - a3;
      yr[j0] = y0.re, yi[j0] = y0.im;
      yr[j0 + Ns] = y1.re, yi[j0 + Ns] = y1.im;
      yr[j0 + 2 * Ns] = y2.re, yi[j0 + 2 * Ns] = y2.im;
      yr[j0 + 3 * Ns] = y3.re, yi[j0 + 3 * Ns] = y3.im;
    }
    p ^= 1;
    __syncthreads();
  }
  if (Ns < M) {                            // Ns = M / 2
    const int T2 = M / 2, step = N / (2 * Ns);
    for (int idx = tid; idx < MEL_FPB * T2; idx += MEL_THREADS) {
      const int f = idx / T2, j = idx - f * T2, k = j & (Ns - 1);
      const float* xr = frames + (long)f * 4 * M + p * 2 * M;
      const float* xi = xr + M;
      float* yr = frames + (long)f * 4 * M + (p ^ 1) * 2 * M;
      float* yi = yr + M;
      const cf32 u0{xr[j], xi[j]};
      const cf32 u1 = mul_tw(cf32{xr[j + T2], xi[j + T2]}, twr, twi, k * step, H);
      const int j0 = ((j - k) << 1) + k;
      const cf32 y0 = u0 + u1, y1 = u0 - u1;
      yr[j0] = y0.re, yi[j0] = y0.im;
      yr[j0 + Ns] = y1.re, yi[j0 + Ns] = y1.im;
    }
    p ^= 1;
    __syncthreads();
  }

  // ---- split the packed spectrum into the real signal's bins 0 .. M and take the magnitude (into the other buffer: M + 1 <= 2 M floats)
  for (int idx = tid; idx < MEL_FPB * (M + 1); idx += MEL_THREADS) {
    const int f = idx / (M + 1), k = idx - f * (M + 1);
    const float* xr = frames + (long)f * 4 * M + p * 2 * M;
    const float* xi = xr + M;
    float* mag = frames + (long)f * 4 * M + (p ^ 1) * 2 * M;
    const int ka = k & (M - 1), kb = (M - k) & (M - 1);
    const cf32 zk{xr[ka], xi[ka]}, zm{xr[kb], -xi[kb]};
    const cf32 s = zk + zm, d = zk - zm;
    const cf32 o{0.5f * d.im, -0.5f * d.re};                               // (zk - zm) / 2i
    const float wr = twr[k], wi = twi[k];
    const float xre = 0.5f * s.re + (o.re * wr - o.im * wi), xim = 0.5f * s.im + (o.re * wi + o.im * wr);
    mag[k] = sqrtf(xre * xre + xim * xim);
  }
  __syncthreads();

  // ---- filterbank, band-wise in bin order
  for (int idx = tid; idx < rows * n_mels; idx += MEL_THREADS) {
    const int f = idx / n_mels, m = idx - f * n_mels;
    const float* mag = frames + (long)f * 4 * M + (p ^ 1) * 2 * M;
    const int bin0 = min(max(band_bin0[m], 0), M + 1), off = min(max(band_off[m], 0), n_weights);
    const int len = min(min(band_off[m + 1] - off, M + 1 - bin0), n_weights - off);      // a table cannot walk out of the buffers
    float s = 0.f;
    for (int i = 0; i < len; ++i) s = fmaf(band_w[off + i], mag[bin0 + i], s);
    dst[idx] = t0 + f < nframes ? s : 0.f;
  }
}

static bool mel_ok(int n_fft, int n_window, int hop, int n_mels) {
  return (n_fft == 512 || n_fft == 1024 || n_fft == 2048) && n_window >= 1 && n_window <= n_fft && hop >= 1 && n_mels >= 1 && n_mels <= 128;
}

}  // namespace sedt

extern "C" int sedt_mel_ok(int n_fft, int n_window, int hop, int n_mels) { return sedt::mel_ok(n_fft, n_window, hop, n_mels) ? 1 : 0; }

extern "C" int sedt_mel_spectrogram(const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* nsamples, int B, float* out,
                                    int out_rows, const float* window, const float* twiddle, const int32_t* band_bin0,
                                    const int32_t* band_off, const float* band_w, int n_weights, int n_fft, int n_window, int hop,
                                    int n_mels, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(mel_ok(n_fft, n_window, hop, n_mels),
               "mel_spectrogram: n_fft=%d n_window=%d hop=%d n_mels=%d outside the envelope (n_fft 512, 1024 or 2048; 1 <= n_window <= n_fft; "
               "hop >= 1; 1 <= n_mels <= 128)", n_fft, n_window, hop, n_mels);
  SEDT_REQUIRE(wave_dtype == SEDT_F32 || wave_dtype == SEDT_I16, "mel_spectrogram: wave_dtype %d is neither SEDT_F32 nor SEDT_I16", wave_dtype);
  SEDT_REQUIRE(wave && nsamples && out && window && twiddle && band_bin0 && band_off && band_w, "mel_spectrogram: null pointer");
  SEDT_REQUIRE(B >= 0 && B <= 65535 && out_rows >= 1 && wave_stride >= 1 && wave_stride <= 0x7fffffffL && n_weights >= 0,
               "mel_spectrogram: B=%d out_rows=%d wave_stride=%lld n_weights=%d", B, out_rows, (long long)wave_stride, n_weights);
  if (B == 0) return 0;
  const size_t lds = (2 * (size_t)(n_fft / 2 + 1) + (size_t)MEL_FPB * 2 * n_fft) * sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mel_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mel_kernel<int16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const dim3 grid((unsigned)((out_rows + MEL_FPB - 1) / MEL_FPB), (unsigned)B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (wave_dtype == SEDT_I16)
    hipLaunchKernelGGL(mel_kernel<int16_t>, grid, dim3(MEL_THREADS), lds, s, reinterpret_cast<const int16_t*>(wave), (long)wave_stride,
                       nsamples, out, out_rows, window, twiddle, band_bin0, band_off, band_w, n_weights, n_fft, n_window, hop, n_mels);
  else
    hipLaunchKernelGGL(mel_kernel<float>, grid, dim3(MEL_THREADS), lds, s, reinterpret_cast<const float*>(wave), (long)wave_stride,
                       nsamples, out, out_rows, window, twiddle, band_bin0, band_off, band_w, n_weights, n_fft, n_window, hop, n_mels);
  return check_launch("mel_spectrogram");
}
