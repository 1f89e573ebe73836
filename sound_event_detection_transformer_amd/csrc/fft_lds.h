// fft_lds.h - the M-point complex FFT in LDS that the packed real transforms of stretch.hip and reverb.hip share: Stockham radix 4,
// separate re / im arrays, ST_FPB frames per workgroup of ST_THREADS (the layout of mel.hip's).  Moved out of stretch.hip unchanged.
#pragma once
#include "common.h"

namespace sedt {

constexpr int ST_THREADS = 256;
constexpr int ST_FPB = 4;               // frames per workgroup

struct scf32 {
  float re, im;
};
__device__ __forceinline__ scf32 operator+(scf32 a, scf32 b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ scf32 operator-(scf32 a, scf32 b) { return {a.re - b.re, a.im - b.im}; }
// a * W_N^u, u in [0, N): the table holds u <= H = N/2, the other half is its negative
__device__ __forceinline__ scf32 st_mul_tw(scf32 a, const float* twr, const float* twi, int u, int H) {
  const bool neg = u > H;
  const int i = neg ? u - H : u;
  const float wr = neg ? -twr[i] : twr[i], wi = neg ? -twi[i] : twi[i];
  return {a.re * wr - a.im * wi, a.re * wi + a.im * wr};
}

// M-point complex forward FFT of ST_FPB frames in LDS: frame f owns frames[f * 4 M ..), two buffers of [re M | im M], the input in
// buffer 0.  Radix-4 Stockham stages, then a radix-2 one when M is an odd power of two.  Returns the buffer that holds the result.
__device__ __forceinline__ int st_fft(float* frames, const float* twr, const float* twi, int N, int tid) {
  const int M = N / 2, H = N / 2;
  int p = 0, Ns = 1;
  const int T4 = M / 4;
  for (; Ns * 4 <= M; Ns *= 4) {
    const int step = N / (4 * Ns);         // W_{4 Ns}^{r k} = W_N^{r k step}
    for (int idx = tid; idx < ST_FPB * T4; idx += ST_THREADS) {
      const int f = idx / T4, j = idx - f * T4, k = j & (Ns - 1);
      const float* xr = frames + (long)f * 4 * M + p * 2 * M;
      const float* xi = xr + M;
      float* yr = frames + (long)f * 4 * M + (p ^ 1) * 2 * M;
      float* yi = yr + M;
      scf32 u0{xr[j], xi[j]}, u1{xr[j + T4], xi[j + T4]}, u2{xr[j + 2 * T4], xi[j + 2 * T4]}, u3{xr[j + 3 * T4], xi[j + 3 * T4]};
      if (Ns > 1) {
        u1 = st_mul_tw(u1, twr, twi, k * step, H);
        u2 = st_mul_tw(u2, twr, twi, 2 * k * step, H);
        u3 = st_mul_tw(u3, twr, twi, 3 * k * step, H);
      }
      const scf32 a0 = u0 + u2, a1 = u0 - u2, a2 = u1 + u3, d = u1 - u3;
      const scf32 a3{d.im, -d.re};         // -i d
      const int j0 = ((j - k) << 2) + k;
      const scf32 y0 = a0 + a2, y1 = a1 + a3, y2 = a0 - a2, y3 = a1 - a3;
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
    for (int idx = tid; idx < ST_FPB * T2; idx += ST_THREADS) {
      const int f = idx / T2, j = idx - f * T2, k = j & (Ns - 1);
      const float* xr = frames + (long)f * 4 * M + p * 2 * M;
      const float* xi = xr + M;
      float* yr = frames + (long)f * 4 * M + (p ^ 1) * 2 * M;
      float* yi = yr + M;
      const scf32 u0{xr[j], xi[j]};
      const scf32 u1 = st_mul_tw(scf32{xr[j + T2], xi[j + T2]}, twr, twi, k * step, H);
      const int j0 = ((j - k) << 1) + k;
      const scf32 y0 = u0 + u1, y1 = u0 - u1;
      yr[j0] = y0.re, yi[j0] = y0.im;
      yr[j0 + Ns] = y1.re, yi[j0 + Ns] = y1.im;
    }
    p ^= 1;
    __syncthreads();
  }
  return p;
}

}  // namespace sedt
