// lds_gemm_common.h - definitions shared by the LDS-DMA kernels (igemm3.hip, wgrad3.hip, wgrad4.hip)
#pragma once
#include "common.h"

namespace sedt {

constexpr int BK2 = 64;           // bf16 elements per K tile = 128 B per row
constexpr int ROWB = BK2 * 2;     // bytes per LDS row

struct Geom2 {
  int Hi, Wi, Ci, Ho, Wo, KH, KW, sh, sw, ph, pw, dh, dw, transposed;
};

__device__ __forceinline__ long gather_pix2(const Geom2& g, int n, int ho, int wo, int kh, int kw) {
  int hi, wi;
  if (!g.transposed) {
    hi = ho * g.sh - g.ph + kh * g.dh;
    wi = wo * g.sw - g.pw + kw * g.dw;
    if ((unsigned)hi >= (unsigned)g.Hi || (unsigned)wi >= (unsigned)g.Wi) return -1;
  } else {
    int th = ho + g.ph - kh * g.dh, tw = wo + g.pw - kw * g.dw;
    if (th < 0 || tw < 0) return -1;
    hi = th / g.sh;
    wi = tw / g.sw;
    if (hi * g.sh != th || wi * g.sw != tw || hi >= g.Hi || wi >= g.Wi) return -1;
  }
  return ((long)n * g.Hi + hi) * g.Wi + wi;
}

typedef __attribute__((address_space(3))) void lds_void;

// Workgroup barrier that first retires this wave's outstanding LDS operations.  A bare s_barrier orders nothing in LDS: the
// compiler may schedule it ABOVE the lgkmcnt wait of the last fragment reads (their consumers are MFMAs, not memory
// operations), and then another wave that passed the barrier can overwrite the buffer - the f32 staging tile of the epilogue
// aliases the ring - before those reads have executed.  Seen on the single-stage K = 64 kernel: sporadic wrong elements, found
// by the bit-reproducibility test of the full-size step.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// ---- host side.  Which kernel instance runs a problem is decided by ONE pure function of the argument block (lds_plan, igemm3.hip): no HIP
// call, no state.  lds_launch (igemm3.hip) is the only place that turns a plan into a launch; the label sedt_igemm_describe prints is
// the plan's name.
enum LdsProgram { LDS_IGEMM3, LDS_IGEMM3_W8, LDS_IGEMM3_W16, LDS_WGRAD3, LDS_WGRAD4, LDS_IGEMM3_BR /* developer builds only */ };
// what the launch is: a problem of its own, one member of a grouped launch (sedt_igemm_group), or the main GEMM of a launch that takes
// weight-gradient riders along (sedt_igemm_co).  Members and carriers run on the 4-wave program igemm3_kernel - the only one with
// grouped / co-scheduled forms -, WHETHER OR NOT the launch then carries the riders (only its 64x64 2-stage instance can)
enum LdsContext { LDS_SINGLE, LDS_MEMBER, LDS_CARRIER };
struct LdsPlan {
  int prog;                     // LdsProgram
  int bm, bn, s, pp;            // tile, ring depth, igemm3_w8's PP
  unsigned a_bytes, b_bytes;    // buffer-descriptor sizes (forward / dgrad: bit 31 = the prefetch bits, see lds_plan)
};
struct WgradGroup;
bool lds_plan(const SedtIgemm& p, LdsContext ctx, LdsPlan* plan);      // false = outside the family's envelope
void lds_plan_name(const LdsPlan& plan, char* out, size_t cap);       // the instance as a profiler prints it
// *taken = the launch carried `riders`
int lds_launch(const LdsPlan& plan, const SedtIgemm& p, hipStream_t st, const WgradGroup* riders = nullptr, bool* taken = nullptr);

// every launch of the family: the dynamic-LDS attribute once per kernel instance, then the launch
int lds_set_attr(const void* kern, size_t lds, const char* what);      // igemm3.hip
template <auto Kern, typename... Args>
int lds_launch_kernel(const char* what, size_t lds, dim3 grid, int threads, hipStream_t st, const Args&... args) {
  static bool attr_set = false;  // idempotent; a benign race sets it twice
  if (!attr_set) {
    if (lds_set_attr(reinterpret_cast<const void*>(Kern), lds, what)) return 1;
    attr_set = true;
  }
  hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, st, args...);
  return check_launch(what);
}

}  // namespace sedt
