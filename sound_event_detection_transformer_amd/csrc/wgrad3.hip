// wgrad3.hip - lean-issue version of the bf16 LDS-DMA weight-gradient GEMM (wgrad2.hip).
//
// Same data path as wgrad2 ([pixel][channel] tiles by LDS-DMA into an XOR-swizzled 2-stage ring, k-contiguous MFMA
// fragments by ds_read_b64_tr_b16, split-K slabs), with the per-K-tile instruction stream stripped the way igemm3 does it:
//   * every DMA lane keeps ONE running 32-bit byte offset; a K tile (64 pixels) advances it by a wave-uniform step, and
//     a conv row wrap (ho >= Ho -> next image) adds a second uniform constant.  Requires 64 % Wo == 0 and Ho*Wo >= 64, so
//     a lane's wo - and with it the horizontal tap validity - never changes; vertical validity is one unsigned compare;
//   * the 4 x 4 transposing-read offsets are per-thread constants, the ring is unrolled so the stage base is an immediate;
//   * optional 64x128 output tile: one dY fragment feeds two MFMAs.
// Problems outside the envelope fall back to wgrad2 (generic gather) and then to the register-staged kernel.
#include <stdlib.h>
#include <algorithm>
#include "wgrad3_body.h"

namespace sedt {

template <int BN>
__global__ __launch_bounds__(256) void wgrad3_kernel(const SedtIgemm p, const unsigned a_bytes, const unsigned b_bytes,
                                                     const int nmajor) {
  wgrad3_body<BN>(p, a_bytes, b_bytes, nmajor, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void wgrad3_group_kernel(const WgradGroup g) { wgrad_group_run(g, blockIdx.x); }

// ---------------------------------------------------------------------------- host side (the plan and the launcher: igemm3.hip)
bool wgrad4_ok(const SedtIgemm& p);                                        // wgrad4.hip: 128x128 / 256x128 ping-pong kernel
int wgrad4_tile_m(int M, int N);
int wgrad4_stages();
int launch_wgrad4_group(WgradGroup& g, hipStream_t st);

static bool wgrad3_conv_ok(const SedtIgemm& p) {
  return !(p.conv && ((64 % p.Wo) != 0 || p.Ho * p.Wo < 64 || p.Ho < 64 / p.Wo));
}

// true when the problem fits the LDS-DMA weight-gradient kernels (wgrad3 / wgrad4); fills the buffer-descriptor sizes
static bool wgrad_lds_envelope(const SedtIgemm& p, unsigned* a_bytes_out, unsigned* b_bytes_out) {
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (p.scale || p.bias || p.res || p.mask || p.act != SEDT_ACT_NONE || p.drop_p > 0.f || p.alpha != 1.f) return false;
  if (p.splitk <= 1 && !p.out_f32) return false;
  if (p.splitk > 1 && !p.slab) return false;
  if ((p.M & 7) || (p.N & 7) || (p.lda & 7) || (p.ldb & 7)) return false;
  if (!al16(p.A) || !al16(p.B)) return false;
  if (p.conv && ((p.Ci & 7) || p.transposed)) return false;
  long a_bytes = ((long)(p.K - 1) * p.lda + p.M) * 2;
  long b_rows = p.conv ? (long)((p.K + (long)p.Ho * p.Wo - 1) / ((long)p.Ho * p.Wo)) * p.Hi * p.Wi : (long)p.K;
  long b_bytes = ((b_rows - 1) * p.ldb + (p.conv ? p.Ci : p.N)) * 2;
  if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31) || a_bytes <= 0 || b_bytes <= 0) return false;
  *a_bytes_out = (unsigned)a_bytes;
  *b_bytes_out = (unsigned)b_bytes;
  return true;
}

// the weight-gradient half of lds_plan: envelope, then wgrad4 for the large problems, else wgrad3.  false = outside the envelope (the
// general kernel takes it)
bool wgrad_plan(const SedtIgemm& p, LdsPlan* plan) {
  static const int v3 = dev_int("SEDT_WGRAD_V3", 1), wide = dev_int("SEDT_WGRAD_WIDE", -1);
  if (!wgrad_lds_envelope(p, &plan->a_bytes, &plan->b_bytes) || !v3 || !wgrad3_conv_ok(p)) return false;
  plan->pp = 0;
  if (wgrad4_ok(p)) {
    plan->prog = LDS_WGRAD4; plan->bm = wgrad4_tile_m(p.M, p.N); plan->bn = 128; plan->s = wgrad4_stages();
    return true;
  }
  // measured on the full step: the wide tile does not pay (fewer, longer workgroups); opt-in only (SEDT_WGRAD_WIDE=1)
  // a 16-byte chunk never straddles a tap (Ci % 8 == 0), so the wide tile needs nothing beyond N % 128 == 0
  plan->prog = LDS_WGRAD3; plan->bm = 64; plan->bn = (wide == 1 && (p.N % 128) == 0) ? 128 : 64; plan->s = 2;
  return true;
}

template <int BN>
static int launch_wgrad3_bn(const LdsPlan& pl, const SedtIgemm& p, hipStream_t st) {
  constexpr size_t lds = (size_t)2 * (64 * ROWB + 64 * BN * 2);
  const int nwg = ((p.N + BN - 1) / BN) * ((p.M + 63) / 64);
  static const int force = dev_int("SEDT_WGRAD_NMAJOR", -1);
  const int nmajor = force >= 0 ? force : (p.N > p.M ? 1 : 0);
  return lds_launch_kernel<wgrad3_kernel<BN>>("wgrad3", lds, dim3(nwg, p.splitk > 1 ? p.splitk : 1), 256, st, p, pl.a_bytes, pl.b_bytes, nmajor);
}
int launch_wgrad3(const LdsPlan& pl, const SedtIgemm& p, hipStream_t st) {
  return pl.bn == 128 ? launch_wgrad3_bn<128>(pl, p, st) : launch_wgrad3_bn<64>(pl, p, st);
}

// ---- grouped launches (sedt_wgrad_group) and riders (sedt_igemm_co)
// the kernel of sedt_wgrad_group that takes a problem: 4 = the 256/128x128 group (wgrad4), 3 = the 64x64 group, 0 = neither.  The label
// sedt_igemm_describe(grouped = 1) prints is this class
// (wgrad3_conv_ok is not part of it: a problem that fails it sends its whole group to single launches, yet is still labelled with a group kernel)
int wgrad_group_class(const SedtIgemm& p, unsigned* a_bytes, unsigned* b_bytes) {
  if (!p.trans || !wgrad_lds_envelope(p, a_bytes, b_bytes)) return 0;
  return wgrad4_ok(p) ? 4 : 3;
}

// Fills g, the group of the 64x64 program, from up to WG_MAXG problems; false = one of them is outside the lean kernel's envelope.
// riders = false (sedt_wgrad_group): the problems of class 4 go to g4 (launch_wgrad4_group completes it); problem ranges start on
//   multiples of 8 workgroups (XCD = id & 7), and a split factor that is a multiple of 8 takes the K-slice map (bit 1 of nmajor).
// riders = true (sedt_igemm_co): every problem rides on the 64x64 program; riders of a co-scheduled launch do not start on an XCD
//   boundary: no padding, no K-slice map.
static bool wgrad_group_fill(const SedtIgemm* jobs, int njobs, bool riders, WgradGroup* g, WgradGroup* g4) {
  g->n = 0;
  if (g4) g4->n = 0;
  int blk = 0;
  for (int j = 0; j < njobs; ++j) {
    const SedtIgemm& p = jobs[j];
    unsigned a, b;
    const int cls = wgrad_group_class(p, &a, &b);
    if (cls == 0 || !wgrad3_conv_ok(p)) return false;
    WgradGroup* t = (cls == 4 && !riders) ? g4 : g;
    const int i = t->n++;
    t->p[i] = p;
    t->a_bytes[i] = a;
    t->b_bytes[i] = b;
    if (t != g) continue;
    const int sk = p.splitk > 1 ? p.splitk : 1;
    g->nwg[i] = ((p.N + 63) / 64) * ((p.M + 63) / 64);
    g->nmajor[i] = (p.N > p.M ? 1 : 0) + ((!riders && sk >= 8 && sk % 8 == 0) ? 2 : 0);
    g->blk0[i] = blk;
    blk += riders ? g->nwg[i] * sk : (g->nwg[i] * sk + 7) / 8 * 8;
  }
  g->blk0[g->n] = blk;
  return true;
}

// 0 = launched, -1 = some problem is outside the lean kernel's envelope (caller launches them one by one)
int wgrad3_group_try(const SedtIgemm* jobs, int njobs, hipStream_t st) {
  static const int on = dev_int("SEDT_WGRAD_GROUP", 1);
  if (!on || njobs < 1) return -1;
  for (int i = 0; i < njobs; ++i) {       // validate everything before launching anything
    unsigned a, b;
    if (wgrad_group_class(jobs[i], &a, &b) == 0 || !wgrad3_conv_ok(jobs[i])) return -1;
  }
  constexpr size_t lds = (size_t)2 * (64 * ROWB + 64 * 64 * 2);
  for (int base = 0; base < njobs; base += WG_MAXG) {
    WgradGroup g, g4;                 // the 64x64 program, and the large problems that take the 128x128 ping-pong kernel
    wgrad_group_fill(jobs + base, std::min(WG_MAXG, njobs - base), false, &g, &g4);
    if (g4.n > 0)
      if (int r = launch_wgrad4_group(g4, st)) return r;
    if (g.n > 0)
      if (int r = lds_launch_kernel<wgrad3_group_kernel>("wgrad3_group", lds, dim3(g.blk0[g.n]), 256, st, g)) return r;
  }
  return 0;
}

// the riders of a co-scheduled launch: fills g from up to WG_MAXG problems; -1 if one of them is outside the lean kernel's envelope
int wgrad3_group_build(const SedtIgemm* jobs, int njobs, WgradGroup* g) {
  return (njobs >= 1 && njobs <= WG_MAXG && wgrad_group_fill(jobs, njobs, true, g, nullptr)) ? 0 : -1;
}

}  // namespace sedt
