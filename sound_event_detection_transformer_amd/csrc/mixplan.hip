// mixplan.hip - the label half of mixup_data (reference utilities/mixup.py:13-127) on the device, for batches whose targets were built on
// the device (utilities/recording_clips.py: the blob sedt_cut_clips writes).  It is the device restatement of
// utilities.mixup.plan_mixup_data; DESIGN.md section 4 ("Mix-up and mean-teacher training on recordings") holds the definition,
// tests/mixup_plan_ref.py restates it in NumPy.  Sibling of mixup_targets_kernel (csrc/input.hip), which plans mixup_label_unlabel.
//
// Source: the first B of B_src all-strong clips (int32 lab_off [B_src + 1] | box_off [B_src + 1] | 2 words, lab_cat int64, box_cat f32
// [.][2]) read under the static split 0 <= ns <= n_lab <= B: clip b has nl(b) labels (0 when b >= n_lab) and nb(b) boxes (0 when
// b >= ns: a weak clip's boxes are ignored).  For i < mix_num <= ns and j = index[i] the decision is the first row that applies:
//   nb(i) == 0 or nb(j) == 0:  nb(i) > 0 keep-1 (target i, job (i, 0, 1, 0)); nb(j) > 0 keep-2 (target j, job (0, j, 2, 0)); else the
//                              weak merge (labels of i then of j, no boxes, ratio lam x nl(i) then (1 - lam) x nl(j), job (i, j, 0, lam))
//   nb(i) + nb(j) > max_events:                                  keep-1
//   two boxes of one class overlap anywhere in boxes(i) ++ boxes(j) (box k carries label k of labels(i) ++ labels(j); s = c - l / 2,
//   e = c + l / 2 in f32; a clash iff !(e_j < s_k) && !(e_k < s_j)):  keep-1
//   else the strong merge: labels, boxes, ratios concatenated, job (i, j, 0, lam)
// Output order: keeps and strong merges in order of i | clips mix_num .. ns - 1 | weak merges in order of i | clips ns .. B - 1; an
// unchanged clip b has job (b, 0, 1, 0) and ratio 1.  With W weak merges the new split is ns' = ns - W | n_lab.
//
// One workgroup of 16 waves, four dependent phases, five barriers (one between phases, one inside each scan):
//   A  one wave per mixed clip: the decision (lanes own the boxes of the candidate, pair-wise test, __any)
//   B  one thread per source clip: scan of the weak merges -> the clip's output slot; slot -> (source, partner, decision, counts) in LDS
//   C  one thread per output slot: scan of the label and box counts -> both offset tables, the split words
//   D  one wave per output slot: labels, ratios, boxes, the job record
// No atomics, no allocation, no synchronisation; every offset read from the source is clamped to its table before it indexes anything.
#include "common.h"

#pragma clang fp contract(off)     // c - l / 2, c + l / 2: the reference's separately rounded f32 operations

namespace sedt {

#define SEDT_MIXPLAN_THREADS 1024

struct PlanJob {                   // the record sedt_mixup reads (MixJob of csrc/input.hip)
  int32_t src1, src2, mode;
  float lam;
};

struct MixPlan {
  const int32_t* lab_off; const int32_t* box_off; const int64_t* lab; const float* box;      // the source tables
  const int32_t* index; const float* lam;
  int32_t* lab_off_out; int32_t* box_off_out; int64_t* lab_out; float* box_out; float* ratio_out;
  PlanJob* jobs; int32_t* status;
  int32_t B, ns, n_lab, mix_num, max_events, M, cap_src;
};

struct PlanClip { int lo, nl, bo, nb; };

// labels and boxes of source clip b under the static split, clamped to the source tables (cap_src entries) and to one lane per label
__device__ __forceinline__ PlanClip plan_clip(const MixPlan& a, int b) {
  PlanClip c{0, 0, 0, 0};
  if (b < a.n_lab) {
    c.lo = min(max(a.lab_off[b], 0), a.cap_src);
    c.nl = min(max(a.lab_off[b + 1] - c.lo, 0), min(63, a.cap_src - c.lo));
  }
  if (b < a.ns) {
    c.bo = min(max(a.box_off[b], 0), a.cap_src);
    c.nb = min(max(a.box_off[b + 1] - c.bo, 0), min(c.nl, a.cap_src - c.bo));      // (the tables' invariant: no more boxes than labels)
  }
  return c;
}

// inclusive scan of the pair (x, y) over the 1024 threads; `sums` [2][16] is this scan's own scratch.  One barrier.
__device__ __forceinline__ void plan_scan(int& x, int& y, int (*sums)[SEDT_MIXPLAN_THREADS / 64], int& total_x, int& total_y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ux = __shfl_up(x, o, 64), uy = __shfl_up(y, o, 64);
    if (lane >= o) { x += ux; y += uy; }
  }
  if (lane == 63) { sums[0][wave] = x; sums[1][wave] = y; }
  __syncthreads();
  total_x = total_y = 0;
#pragma unroll
  for (int w = 0; w < SEDT_MIXPLAN_THREADS / 64; ++w) {
    const int sx = sums[0][w], sy = sums[1][w];
    if (w < wave) { x += sx; y += sy; }
    total_x += sx; total_y += sy;
  }
}

__global__ __launch_bounds__(SEDT_MIXPLAN_THREADS) void mixup_plan_kernel(const MixPlan a) {
  __shared__ int dec[1024];                      // phase A: decision of mixed clip i (0 strong merge, 1 keep-1, 2 keep-2, 3 weak merge; +4 bad index)
  __shared__ int prim[1024], part[1024], code[1024], cntl[1024], cntb[1024];      // per output slot
  __shared__ int offl[1025], offb[1025];
  __shared__ int sums[4][SEDT_MIXPLAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = SEDT_MIXPLAN_THREADS / 64;
  // ---- A: decisions
  for (int i = wave; i < a.mix_num; i += nw) {
    int j = a.index[i];
    const bool bad = j < 0 || j >= a.B;
    if (bad) j = i;
    const PlanClip c1 = plan_clip(a, i), c2 = plan_clip(a, j);
    int d;
    if (bad) {
      d = 1 | 4;
    } else if (c1.nb == 0 || c2.nb == 0) {
      d = c1.nb > 0 ? 1 : (c2.nb > 0 ? 2 : 3);
    } else if (c1.nb + c2.nb > a.max_events) {
      d = 1;
    } else {
      const int n = c1.nb + c2.nb;                 // <= max_events <= 63: one lane per box; box k carries label k of the concatenated LABEL list
      bool clash = false;
      if (lane < n) {
        const int k = lane;
        const float* bk = k < c1.nb ? a.box + 2L * (c1.bo + k) : a.box + 2L * (c2.bo + k - c1.nb);
        const int64_t ek = k < c1.nl ? a.lab[c1.lo + k] : a.lab[c2.lo + k - c1.nl];
        const float ck = bk[0], lk = bk[1];
        const float sk = ck - lk / 2, tk = ck + lk / 2;
        for (int m = 0; m < k; ++m) {
          const int64_t em = m < c1.nl ? a.lab[c1.lo + m] : a.lab[c2.lo + m - c1.nl];
          if (em != ek) continue;
          const float* bm = m < c1.nb ? a.box + 2L * (c1.bo + m) : a.box + 2L * (c2.bo + m - c1.nb);
          const float cm = bm[0], lm = bm[1];
          const float sm = cm - lm / 2, tm = cm + lm / 2;
          if (!(tk < sm) && !(tm < sk)) clash = true;
        }
      }
      d = __any(clash) ? 1 : 0;
    }
    if (lane == 0) dec[i] = d;
  }
  __syncthreads();
  // ---- B: the output slot of source clip t
  const int mine = t < a.mix_num ? dec[t] : 1;
  int W, unused, wincl = (mine & 3) == 3 ? 1 : 0, zero = 0;
  plan_scan(wincl, zero, sums, W, unused);
  if (t < a.B) {
    const int d = mine & 3;
    int j = 0, p;
    if (t < a.mix_num) {
      j = (mine & 4) ? t : a.index[t];
      p = d == 3 ? a.ns - W + (wincl - 1) : t - wincl;
    } else {
      p = t < a.ns ? t - W : t;
    }
    const PlanClip c1 = plan_clip(a, t);
    PlanClip c2{0, 0, 0, 0};
    if (d != 1) c2 = plan_clip(a, j);
    int nl = d == 1 ? c1.nl : (d == 2 ? c2.nl : c1.nl + c2.nl);
    int nb = d == 1 ? c1.nb : (d == 2 ? c2.nb : (d == 0 ? c1.nb + c2.nb : 0));
    a.status[t] = nl > a.M ? 1 : ((mine & 4) ? 2 : 0);
    nl = min(nl, a.M);
    nb = min(nb, nl);
    prim[p] = t; part[p] = j; code[p] = d; cntl[p] = nl; cntb[p] = nb;
  }
  __syncthreads();
  // ---- C: offsets of output slot t
  int totl, totb, il = t < a.B ? cntl[t] : 0, ib = t < a.B ? cntb[t] : 0;
  plan_scan(il, ib, sums + 2, totl, totb);
  if (t < a.B) {
    offl[t + 1] = il; offb[t + 1] = ib;
    a.lab_off_out[t + 1] = il; a.box_off_out[t + 1] = ib;
  }
  if (t == 0) {
    offl[0] = 0; offb[0] = 0;
    a.lab_off_out[0] = 0; a.box_off_out[0] = 0;
    a.box_off_out[a.B + 1] = a.ns - W;             // the split words: strong | labelled clips of this batch
    a.box_off_out[a.B + 2] = a.n_lab;
  }
  __syncthreads();
  // ---- D: the write phase
  const float lam = a.lam[0], lam1 = a.lam[1];
  for (int p = wave; p < a.B; p += nw) {
    const int i = prim[p], j = part[p], d = code[p], nl = cntl[p], nb = cntb[p], lo = offl[p], bo = offb[p];
    const bool merged = d == 0 || d == 3;
    if (lane == 0) a.jobs[p] = d == 2 ? PlanJob{0, j, 2, 0.f} : PlanJob{i, merged ? j : 0, merged ? 0 : 1, merged ? lam : 0.f};
    PlanClip c1{0, 0, 0, 0}, c2{0, 0, 0, 0};
    if (d != 2) c1 = plan_clip(a, i);
    if (d != 1) c2 = plan_clip(a, j);
    if (lane < nl) {                               // nl <= M <= 63
      a.lab_out[lo + lane] = lane < c1.nl ? a.lab[c1.lo + lane] : a.lab[c2.lo + lane - c1.nl];
      a.ratio_out[lo + lane] = merged ? (lane < c1.nl ? lam : lam1) : 1.f;
    }
    for (int k = lane; k < 2 * nb; k += 64)
      a.box_out[2L * bo + k] = k < 2 * c1.nb ? a.box[2L * c1.bo + k] : a.box[2L * c2.bo + k - 2 * c1.nb];
  }
}

}  // namespace sedt

extern "C" int sedt_mixup_plan(const void* src_blob, int B_src, int max_targets_src, int B, int ns, int n_lab, const int32_t* index,
                               const float* lam, int mix_num, int max_events, int max_targets_out, void* out_blob, void* jobs,
                               int32_t* status, void* stream) {
  using namespace sedt;
  SEDT_REQUIRE(B >= 1 && B <= B_src && B_src <= 1024 && ns >= 0 && ns <= n_lab && n_lab <= B && mix_num >= 0 && mix_num <= ns,
               "mixup_plan: B=%d B_src=%d ns=%d n_lab=%d mix_num=%d outside the envelope (1 <= B <= B_src <= 1024; 0 <= ns <= n_lab <= B; "
               "0 <= mix_num <= ns: the batch then keeps its size on every draw)", B, B_src, ns, n_lab, mix_num);
  SEDT_REQUIRE(max_events >= 1 && max_events <= max_targets_out && max_targets_out <= 63 && max_targets_src >= 1 && max_targets_src <= 63,
               "mixup_plan: max_events=%d max_targets_out=%d max_targets_src=%d outside the envelope (1 <= max_events <= max_targets_out "
               "<= 63, 1 <= max_targets_src <= 63: the target tables' own limit)", max_events, max_targets_out, max_targets_src);
  SEDT_REQUIRE(src_blob && index && lam && out_blob && jobs && status, "mixup_plan: null pointer");
  SEDT_REQUIRE((reinterpret_cast<uintptr_t>(src_blob) & 7) == 0 && (reinterpret_cast<uintptr_t>(out_blob) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(jobs) & 3) == 0, "mixup_plan: the blobs are 8-byte aligned, the job table 4-byte aligned");
  const unsigned char* s = reinterpret_cast<const unsigned char*>(src_blob);
  unsigned char* o = reinterpret_cast<unsigned char*>(out_blob);
  const long cs = (long)B_src * max_targets_src, co = (long)B * max_targets_out;
  MixPlan a;
  a.lab_off = reinterpret_cast<const int32_t*>(s);
  a.box_off = a.lab_off + (B_src + 1);
  a.lab = reinterpret_cast<const int64_t*>(s + 8L * B_src + 16);
  a.box = reinterpret_cast<const float*>(s + 8L * B_src + 16 + 8 * cs);
  a.index = index;
  a.lam = lam;
  a.lab_off_out = reinterpret_cast<int32_t*>(o);
  a.box_off_out = a.lab_off_out + (B + 1);
  a.lab_out = reinterpret_cast<int64_t*>(o + 8L * B + 16);
  a.box_out = reinterpret_cast<float*>(o + 8L * B + 16 + 8 * co);
  a.ratio_out = reinterpret_cast<float*>(o + 8L * B + 16 + 16 * co);
  a.jobs = reinterpret_cast<PlanJob*>(jobs);
  a.status = status;
  a.B = B; a.ns = ns; a.n_lab = n_lab; a.mix_num = mix_num; a.max_events = max_events; a.M = max_targets_out; a.cap_src = (int)cs;
  hipLaunchKernelGGL(mixup_plan_kernel, dim3(1), dim3(SEDT_MIXPLAN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return check_launch("mixup_plan");
}
