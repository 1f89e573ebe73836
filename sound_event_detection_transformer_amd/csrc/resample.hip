// resample.hip - sample-rate conversion and down-mix of a batch of recordings in ONE launch: band-limited interpolation with a
// Kaiser-windowed sinc in its polyphase form (utilities/resample.py holds the definition; the host makes the coefficient table in
// float64 and rounds it once - the kernel evaluates no Bessel function and no sine).
//
//   y[n] = sum_{k = -H .. taps - 1 - H} T[p][k] * m[i + k],   i = (n M) div L,  p = (n M) mod L,  m[j] = 0 outside 0 <= j < n_in,
//   m[j] = mean over the channels of frame j (interleaved (frames, channels); int16: x / 32768).
//
// A workgroup of 256 owns RS_BLK = 1024 consecutive outputs of one recording:
//   stage    the input span [i(n0) - H, i(n0 + nb - 1) - H + taps) goes to LDS once, down-mixed on the way (channel sum in float64,
//            divided, rounded once; one channel: the sample itself) and zero outside the recording.  (RS_BLK M / L + taps + 1 floats.)
//   table    the device copy is stored [taps][L] with column r = n mod L holding row p = (r M) mod L: lanes that own consecutive
//            outputs read consecutive floats of one tap's line (coalesced, L2-resident: every workgroup reads the same table).
//   sum      the block's outputs e = c L + r form columns of one phase: outputs n and n + L share a table row while their input
//            windows shift by exactly M.  A lane owns (r, RS_Q columns G apart): ONE coefficient load feeds RS_Q FMAs, each of which
//            reads its input from LDS.  Lanes r, r + 1 read LDS a stride of about M / L apart, columns a stride of M.
//   order    every output is ONE chain: acc = T[p][-H] * m[i - H], then fmaf over k ascending.  Its bits depend on the recording, n and
//            the table alone - not on the batch, on the recording's place in it, nor on which lane or workgroup owns n.
// All arithmetic on n M and n_in L is 64-bit.  No atomics, no allocation, no synchronisation; capturable.
#include "common.h"

namespace sedt {

constexpr int RS_THREADS = 256;
constexpr int RS_BLK = SEDT_RESAMPLE_BLK;   // outputs per workgroup
constexpr int RS_Q = 4;                     // outputs of one phase per lane
constexpr int RS_DESC = SEDT_RESAMPLE_DESC_WORDS;
constexpr int64_t RS_MAX_SPAN = 16384;      // floats of LDS (64 KB)
constexpr int64_t RS_MAX_TABLE = 16 << 20;  // bytes
constexpr int64_t RS_MAX_IN = (int64_t)1 << 40;

__device__ __forceinline__ float rs_mix(const void* src, int dtype, int64_t j, int C) {
  if (dtype == SEDT_I16) {
    const int16_t* s = reinterpret_cast<const int16_t*>(src) + j * C;
    if (C == 1) return (float)s[0] * (1.0f / 32768.0f);
    double a = 0.0;
    for (int c = 0; c < C; ++c) a += (double)((float)s[c] * (1.0f / 32768.0f));
    return (float)(a / (double)C);
  }
  const float* s = reinterpret_cast<const float*>(src) + j * C;
  if (C == 1) return s[0];
  double a = 0.0;
  for (int c = 0; c < C; ++c) a += (double)s[c];
  return (float)(a / (double)C);
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const int64_t* __restrict__ desc, const float* __restrict__ table, int L,
                                                              int M, int taps, int H, int max_channels, int64_t max_in, int span_max) {
  extern __shared__ float rs_lds[];
  const int64_t* d = desc + (int64_t)blockIdx.y * RS_DESC;
  const void* src = reinterpret_cast<const void*>(d[0]);
  float* dst = reinterpret_cast<float*>(d[1]);
  const int64_t n_in = min(max(d[2], (int64_t)0), max_in);        // the declared bounds hold whatever the descriptor says
  const int64_t cap = max(d[3], (int64_t)0);
  const int C = (int)min(max(d[4], (int64_t)1), (int64_t)max_channels);
  const int dtype = (int)d[5];
  const int64_t n_out = min((n_in * L + M - 1) / M, cap);
  const int64_t n0 = (int64_t)blockIdx.x * RS_BLK;
  const int tid = threadIdx.x;
  if (n0 >= cap) return;
  const int room = (int)min((int64_t)RS_BLK, cap - n0);           // outputs of this block the destination holds
  const int nb = (int)min((int64_t)RS_BLK, max(n_out - n0, (int64_t)0));   // ... and how many of them are samples of the result
  for (int e = nb + tid; e < room; e += RS_THREADS) dst[n0 + e] = 0.f;
  if (nb == 0) return;                                           // (uniform over the workgroup)

  // ---- stage the input span, down-mixed
  const int64_t i_lo = (n0 * M) / L - H;
  const int64_t i_hi = ((n0 + nb - 1) * M) / L - H + taps;        // exclusive
  const int span = (int)min(i_hi - i_lo, (int64_t)span_max);      // (never cut inside the envelope)
  for (int s = tid; s < span; s += RS_THREADS) {
    const int64_t j = i_lo + s;
    rs_lds[s] = (j >= 0 && j < n_in) ? rs_mix(src, dtype, j, C) : 0.f;
  }
  __syncthreads();

  // ---- columns of one phase: e = c L + r
  const int Lr = min(L, RS_BLK);
  const int cols = (RS_BLK + L - 1) / L;
  const int G = (cols + RS_Q - 1) / RS_Q;
  const int items = Lr * G;
  const int r0 = (int)(n0 % L);
  for (int w = tid; w < items; w += RS_THREADS) {
    const int cg = w / Lr, r = w - cg * Lr;
    const int e0 = cg * L + r;
    if (e0 >= nb) continue;
    const int64_t nM = (n0 + e0) * M;
    const int base = (int)(nM / L - H - i_lo);                    // LDS index of tap -H of output e0
    int rho = r0 + r;
    if (rho >= L) rho -= L;
    const int estep = G * L;                                      // the lane's outputs are e0, e0 + estep, ...: LDS windows G M apart
    const int xstep = G * M;
    int off[RS_Q];
    bool live[RS_Q];
#pragma unroll
    for (int q = 0; q < RS_Q; ++q) {
      live[q] = e0 + (int64_t)q * estep < nb;
      off[q] = live[q] ? base + q * xstep : base;                 // a dead column re-reads column 0: in bounds, never stored
    }
    const float* col = table + rho;
    float acc[RS_Q];
    {
      const float c = col[0];
#pragma unroll
      for (int q = 0; q < RS_Q; ++q) acc[q] = c * rs_lds[off[q]];
    }
    for (int k = 1; k < taps; ++k) {
      const float c = col[(int64_t)k * L];
#pragma unroll
      for (int q = 0; q < RS_Q; ++q) acc[q] = fmaf(c, rs_lds[off[q] + k], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < RS_Q; ++q)
      if (live[q]) dst[n0 + e0 + (int64_t)q * estep] = acc[q];
  }
}

static int64_t rs_span(int L, int M, int taps) { return ((int64_t)RS_BLK * M + L - 1) / L + taps + 1; }

static bool resample_ok(int L, int M, int taps, int H, int max_channels, int64_t max_in) {
  return L >= 1 && L <= 4096 && M >= 1 && M <= 4096 && taps >= 1 && taps <= 8192 && H >= 0 && H < taps &&
         (int64_t)L * taps * 4 <= RS_MAX_TABLE && rs_span(L, M, taps) <= RS_MAX_SPAN && max_channels >= 1 && max_channels <= 64 &&
         max_in >= 1 && max_in <= RS_MAX_IN;
}

}  // namespace sedt

extern "C" int sedt_resample_ok(int L, int M, int taps, int H, int max_channels, int64_t max_in) {
  return sedt::resample_ok(L, M, taps, H, max_channels, max_in) ? 1 : 0;
}

extern "C" int sedt_resample(const int64_t* desc, int B, int64_t max_out, const float* table, int L, int M, int taps, int H,
                             int max_channels, int64_t max_in, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(resample_ok(L, M, taps, H, max_channels, max_in),
               "resample: L=%d M=%d taps=%d H=%d max_channels=%d max_in=%lld outside the envelope (1 <= L, M <= 4096; 1 <= taps <= 8192; "
               "0 <= H < taps; table L * taps * 4 <= %lld bytes; input span of a workgroup ceil(%d M / L) + taps + 1 <= %lld floats; "
               "1 <= channels <= 64; 1 <= frames <= 2^40)",
               L, M, taps, H, max_channels, (long long)max_in, (long long)RS_MAX_TABLE, RS_BLK, (long long)RS_MAX_SPAN);
  SEDT_REQUIRE(B >= 0 && B <= 65535 && max_out >= 1 && (max_out + RS_BLK - 1) / RS_BLK <= 0x7fffffffLL,
               "resample: B=%d max_out=%lld (B <= 65535; 1 <= max_out <= %d * (2^31 - 1))", B, (long long)max_out, RS_BLK);
  SEDT_REQUIRE(desc && table, "resample: null pointer");
  if (B == 0) return 0;
  const int span = (int)rs_span(L, M, taps);
  const dim3 grid((unsigned)((max_out + RS_BLK - 1) / RS_BLK), (unsigned)B);
  hipLaunchKernelGGL(resample_kernel, grid, dim3(RS_THREADS), (size_t)span * sizeof(float), reinterpret_cast<hipStream_t>(stream), desc,
                     table, L, M, taps, H, max_channels, max_in, span);
  return check_launch("resample");
}
