// attn_mfma.hip - bf16 multi-head attention forward/backward on MFMA for gfx950 (head dim 32, L <= 256).
//
// One workgroup per (batch, head); Q/K/V (and dO) tiles of that head are staged once in LDS as bf16 [L][32] images
// (64-B rows).  All four contractions run on v_mfma_f32_32x32x16_bf16:
//
//   forward, wave = 32 queries:   S^T = K Q^T   (lane <-> query, registers <-> keys: softmax statistics are in-lane
//                                                reductions + one cross-half shuffle)
//                                 O  += P V      P straight from the S^T accumulators (k-slot s of half h <-> key
//                                                16u + (s&3) + 8(s>>2) + 4h); the matching V^T fragment is read with
//                                                ds_read_b64_tr_b16 (same k-slot order), so no cross-lane movement.
//   backward pass B (32 keys):    S = Q K^T, dP = dO V^T (lane <-> key, registers <-> queries), dS = P (dP - delta)
//                                 dV^T += dO^T Pd,  dK^T += Q^T dS            (dO^T, Q^T via tr reads)
//                                 dS also goes, as the bf16 the MFMA reads, into an LDS image [query tile][key][32 queries]
//   backward dQ phase (32 queries), after one workgroup barrier:  dQ += dS K  (dS and K^T via tr reads of the two images)
//
// Probabilities never touch HBM: backward recomputes them from the saved log-sum-exp; the dropout mask is the counter
// hash of ((b*H+h)*Lq + q)*Lk + k, identical in forward and backward (and to the f32 reference kernels).
#include <stdlib.h>
#include "common.h"
#include "attn_frag.h"

namespace sedt {

// ============================================================================================ forward
template <int NT, bool AMASK>   // key tiles; additive attention mask present
__global__ __launch_bounds__(256, 2) void attn_fwd_mfma_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ k,
                                                               long ldk, const bf16_t* __restrict__ v, long ldv,
                                                               bf16_t* __restrict__ o, long ldo, float* __restrict__ lse,
                                                               const uint8_t* __restrict__ kpm, const float* __restrict__ amask,
                                                               int H, int Lq, int Lk, float scale, uint32_t thresh, float inv_keep,
                                                               uint32_t seed, const uint32_t* seed_ptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int LkP = NT * 32, LqP = (Lq + 31) & ~31;
  unsigned char* Ki = smem;
  unsigned char* Vi = Ki + LkP * AROW;
  unsigned char* Qi = Vi + LkP * AROW;
  float* Kb = reinterpret_cast<float*>(Qi + LqP * AROW);
  float* Rs = Kb + LkP;                                // [waves][32] 1 / row-sum strips
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = blockDim.x, nwave = nthr >> 6;
  stage_image(Ki, k + (long)b * Lk * ldk + h * AD, ldk, Lk, LkP, tid, nthr);
  stage_image(Vi, v + (long)b * Lk * ldv + h * AD, ldv, Lk, LkP, tid, nthr);
  stage_image(Qi, q + (long)b * Lq * ldq + h * AD, ldq, Lq, LqP, tid, nthr);
  stage_key_bias(Kb, kpm ? kpm + (long)b * Lk : nullptr, Lk, LkP, tid, nthr);
  __syncthreads();
  const uint32_t sd = eff_seed(seed, seed_ptr);
  const int hf = lane >> 5;
  for (int q0 = wave * 32; q0 < Lq; q0 += nwave * 32) {
    const int qi = q0 + (lane & 31);                   // this lane's query
    const bf16x8 qf0 = frag_rows(Qi, q0, 0, lane), qf1 = frag_rows(Qi, q0, 1, lane);
    // one score tile (32 keys x this wave's 32 queries): S^T = K Q^T, scaled and masked.  Register r of half hf <-> key
    // 8*(r>>2) + 4*hf + (r&3): four consecutive keys per register group
    auto score_tile = [&](int kt, f32x16& st) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Ki, kt * 32, 0, lane), qf0, st, 0, 0, 0);
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Ki, kt * 32, 1, lane), qf1, st, 0, 0, 0);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int key0 = kt * 32 + 8 * g4 + 4 * hf;
        const float4 kb = *reinterpret_cast<const float4*>(Kb + key0);
        const float kbv[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float sc = st[4 * g4 + e] * scale + kbv[e];
          if (AMASK) { if (qi < Lq && key0 + e < Lk) sc += amask[(long)qi * Lk + key0 + e]; }
          st[4 * g4 + e] = sc;
        }
      }
    };
    // pass 1: the row maximum only (no exponentials: v_exp_f32 is quarter rate, and the first version of this kernel paid
    // it twice per score - once for the row sum here, once for the probabilities below)
    float m = -INFINITY;
#pragma unroll 1
    for (int kt = 0; kt < NT; ++kt) {
      f32x16 st;
      score_tile(kt, st);
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, st[r]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float ms = m > -INFINITY ? m : 0.f;             // a fully masked row: every exp(-inf - 0) = 0, sum 0, output NaN as torch
    const uint64_t rowbase = ((uint64_t)bh * Lq + qi) * Lk;
    const uint32_t d_hi = (uint32_t)(rowbase >> 33), d_inner = drop_inner(sd, d_hi);      // seed half of the dropout hash, once per row
    // pass 2: O = dropout(exp(S - max)) V with the row sum gathered on the way (before dropout), scores recomputed tile by
    // tile (two MFMAs per tile - cheaper than keeping them); the 1 / sum goes onto the output rows at the end
    float sum = 0.f;
    f32x16 oacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
#pragma unroll 1
    for (int kt = 0; kt < NT; ++kt) {
      f32x16 st;
      score_tile(kt, st);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float pv[8];
#pragma unroll
        for (int s4 = 0; s4 < 2; ++s4) {                  // a lane's keys come in runs of four: two hashes per run
          uint32_t keep = 0xfu;
          if (thresh) keep = drop_keep4(d_inner, d_hi, sd, rowbase + (kt * 32 + crow(8 * u + 4 * s4, hf)), thresh);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float p = __expf(st[8 * u + 4 * s4 + e] - ms);
            sum += p;
            pv[4 * s4 + e] = (keep >> e & 1u) ? (thresh ? p * inv_keep : p) : 0.f;
          }
        }
        oacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pack8(pv), frag_cols_tr(Vi, kt * 32 + 16 * u, lane), oacc, 0, 0, 0);
      }
    }
    sum += __shfl_xor(sum, 32, 64);
    if (hf == 0 && qi < Lq) lse[((long)b * H + h) * Lq + qi] = m + __logf(sum);
    // 1 / sum is per QUERY = per lane here, but per accumulator ROW in oacc (lane <-> dim): through this wave's 32-float LDS strip
    float* strip = Rs + wave * 32;
    if (hf == 0) strip[lane] = 1.f / sum;
    __builtin_amdgcn_s_waitcnt(0xc07f);                   // lgkmcnt(0): the strip is written (same wave reads it back)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const float4 iv = *reinterpret_cast<const float4*>(strip + 8 * g4 + 4 * hf);
      oacc[4 * g4 + 0] *= iv.x; oacc[4 * g4 + 1] *= iv.y; oacc[4 * g4 + 2] *= iv.z; oacc[4 * g4 + 3] *= iv.w;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = q0 + crow(r, hf);
      if (qr < Lq) o[((long)b * Lq + qr) * ldo + h * AD + (lane & 31)] = (bf16_t)oacc[r];
    }
  }
}

// ============================================================================================ backward
// a thread's 16-byte chunks of one [LP][32] image (chunk u = tid + i * NTHR <-> row u / 4, columns 8 (u % 4) ..), held in registers
// between the global loads and the LDS stores; rows from L on are stored as zeros (stage_image's layout and padding); 1 <= L <= LP
template <int LP, int NTHR>
struct BwdChunks {
  static constexpr int N = (LP * 4 + NTHR - 1) / NTHR;
  uint4 r[N];
  // no branch around a load (the join would wait for it): rows beyond L read row L - 1 and become zeros on their way to LDS
  __device__ __forceinline__ void load(const bf16_t* src, long ld, int L, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int u = tid + i * NTHR, row = min(u >> 2, L - 1);
      r[i] = *reinterpret_cast<const uint4*>(src + (long)row * ld + (u & 3) * 8);
    }
  }
  __device__ __forceinline__ void store(unsigned char* img, int L, int tid) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int u = tid + i * NTHR;
      if (u < LP * 4) *reinterpret_cast<uint4*>(img + (u >> 2) * AROW + (u & 3) * 16) = (u >> 2) < L ? r[i] : make_uint4(0, 0, 0, 0);
    }
  }
};

template <int NTQ, int NTK, bool AMASK>
__global__ __launch_bounds__(256, 2) void attn_bwd_mfma_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ k,
                                                               long ldk, const bf16_t* __restrict__ v, long ldv,
                                                               const bf16_t* __restrict__ o, long ldo, const bf16_t* __restrict__ dout,
                                                               long lddo, const float* __restrict__ lse, const uint8_t* __restrict__ kpm,
                                                               const float* __restrict__ amask, bf16_t* __restrict__ dq, long lddq,
                                                               bf16_t* __restrict__ dk, long lddk, bf16_t* __restrict__ dv, long lddv,
                                                               int H, int Lq, int Lk, float scale, uint32_t thresh, float inv_keep,
                                                               uint32_t seed, const uint32_t* seed_ptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int LqP = NTQ * 32, LkP = NTK * 32;
  unsigned char* Qi = smem;
  unsigned char* Ki = Qi + LqP * AROW;
  unsigned char* Vi = Ki + LkP * AROW;
  unsigned char* Di = Vi + LkP * AROW;                  // dO image
  float* Ls = reinterpret_cast<float*>(Di + LqP * AROW);   // lse   [LqP]
  float* De = Ls + LqP;                                 // delta [LqP]
  float* Kb = De + LqP;                                 // key bias [LkP]
  unsigned char* Si = reinterpret_cast<unsigned char*>(Kb + LkP);   // dS image, bf16 [NTQ][LkP keys][32 queries], 64-B rows
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  // one wave per tile of the longer side (attn_bwd_mfma_try launches exactly this many threads)
  constexpr int NTHR = 64 * (NTQ > NTK ? NTQ : NTK), nwave = NTHR / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Prologue.  Every global load of a thread is issued before the first LDS store waits for one: the workgroups of a launch all
  // start together (one round of two per CU), so a dependent load - store - load chain per image and loop trip is a chain of exposed
  // memory round trips.  Here it is one.
  const uint32_t sd = eff_seed(seed, seed_ptr);
  BwdChunks<LqP, NTHR> cq, cd;
  BwdChunks<LkP, NTHR> ck, cv;
  uint4 ro[4], rg[4];                                   // row tid of o and dO: delta = dO . o
  const int qrow = min(tid, Lq - 1);
  const float l = lse[((long)b * H + h) * Lq + qrow];
  {
    const uint4* op = reinterpret_cast<const uint4*>(o + ((long)b * Lq + qrow) * ldo + h * AD);
    const uint4* dp = reinterpret_cast<const uint4*>(dout + ((long)b * Lq + qrow) * lddo + h * AD);
#pragma unroll
    for (int c = 0; c < 4; ++c) { ro[c] = op[c]; rg[c] = dp[c]; }
  }
  cq.load(q + (long)b * Lq * ldq + h * AD, ldq, Lq, tid);
  ck.load(k + (long)b * Lk * ldk + h * AD, ldk, Lk, tid);
  cv.load(v + (long)b * Lk * ldv + h * AD, ldv, Lk, tid);
  cd.load(dout + (long)b * Lq * lddo + h * AD, lddo, Lq, tid);
  uint8_t kp = 0;
  if (kpm) kp = kpm[(long)b * Lk + min(tid, Lk - 1)];   // the one branch, after every other load is on its way
  cq.store(Qi, Lq, tid);
  ck.store(Ki, Lk, tid);
  cv.store(Vi, Lk, tid);
  cd.store(Di, Lq, tid);
  if (tid < LkP) Kb[tid] = (tid >= Lk || kp) ? -INFINITY : 0.f;      // LkP, LqP <= NTHR / 2
  if (tid < LqP) {
    float dl = 0.f;
    if (tid < Lq) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 a = __builtin_bit_cast(bf16x8, ro[c]), g = __builtin_bit_cast(bf16x8, rg[c]);
#pragma unroll
        for (int e = 0; e < 8; ++e) dl += (float)a[e] * (float)g[e];
      }
    }
    Ls[tid] = tid < Lq ? l : 0.f;
    De[tid] = dl;
  }
  __syncthreads();
  const int hf = lane >> 5;

  // ---------------- pass B: this wave's 32 keys, all queries -> dK, dV (accumulated transposed: rows = dims, cols = keys) and the
  // dS image.  Every key tile belongs to one wave and every (query tile, key, query) element of the image is written (zero where
  // the query is beyond Lq or the key is padded: p = 0 there), so the dQ phase reads nothing stale.
  for (int k0 = wave * 32; k0 < Lk; k0 += nwave * 32) {
    const int kj = k0 + (lane & 31);                    // this lane's key
    const float kbj = Kb[kj];
    // The dropout hash of element e0 + t0 (e0: this (clip, head)'s first element, t0 = query * Lk + key < 2^14) is that of the 64-bit
    // index (e0 >> 1) + x, x = ((e0 & 1) + t0) >> 1.  Its high word is that of e0 >> 1 plus the carry of the low words' sum, so the
    // seed half of the hash is one of two values computed here, and what is left per element is 32-bit arithmetic.
    const uint64_t e0 = ((uint64_t)bh * Lq) * Lk;
    const uint32_t k_hi = (uint32_t)(e0 >> 33), hb_lo = (uint32_t)(e0 >> 1);
    const uint32_t k_inner = drop_inner(sd, k_hi), k_inner_c = drop_inner(sd, k_hi + 1);
    const uint32_t tl = (uint32_t)(e0 & 1) + kj + 4 * hf * Lk;   // the lane's part of (e0 & 1) + t0
    auto keep_at = [&](int qu) -> bool {                         // qu = query - 4 * hf: uniform
      const uint32_t t = tl + (uint32_t)(qu * Lk);
      const uint32_t lo = hb_lo + (t >> 1);
      const uint32_t hs = mix32(lo ^ (lo < hb_lo ? k_inner_c : k_inner));
      return __builtin_amdgcn_ubfe(hs, (t & 1u) << 4, 16) >= thresh;
    };
    f32x16 dkt, dvt;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dkt[r] = 0.f; dvt[r] = 0.f; }
#pragma unroll 1
    for (int qt = 0; qt < NTQ; ++qt) {
      f32x16 sa, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sa[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 kf = frag_rows(Ki, k0, ks, lane), vf = frag_rows(Vi, k0, ks, lane);
        sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Qi, qt * 32, ks, lane), kf, sa, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Di, qt * 32, ks, lane), vf, dp, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float pd[8], ds[8];
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2) {
          const int qr0 = qt * 32 + 16 * u + 8 * g2 + 4 * hf;
          const float4 l4 = *reinterpret_cast<const float4*>(Ls + qr0), d4 = *reinterpret_cast<const float4*>(De + qr0);
          const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 8 * u + 4 * g2 + e, qr = qr0 + e;
            float sc = sa[r] * scale + kbj;
            if (AMASK) { if (qr < Lq && kj < Lk) sc += amask[(long)qr * Lk + kj]; }
            float p = (qr < Lq) ? __expf(sc - lv[e]) : 0.f;
            float g = dp[r], pk = p;
            if (thresh) {
              const bool keep = keep_at(qr - 4 * hf);
              g = keep ? g * inv_keep : 0.f;
              pk = keep ? p * inv_keep : 0.f;
            }
            pd[4 * g2 + e] = pk;
            ds[4 * g2 + e] = p * (g - dv4[e]);
          }
        }
        // the bf16 dS that feeds dK also goes to the image: a lane's four consecutive queries of one register group are 8 bytes
        // of its key's row
        const bf16x8 dsb = pack8(ds);
        unsigned char* srow = Si + (long)(qt * LkP + kj) * AROW + (16 * u + 4 * hf) * 2;
        *reinterpret_cast<bf16x4*>(srow) = __builtin_shufflevector(dsb, dsb, 0, 1, 2, 3);
        *reinterpret_cast<bf16x4*>(srow + 16) = __builtin_shufflevector(dsb, dsb, 4, 5, 6, 7);
        dvt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_tr(Di, qt * 32 + 16 * u, lane), pack8(pd), dvt, 0, 0, 0);
        dkt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_tr(Qi, qt * 32 + 16 * u, lane), dsb, dkt, 0, 0, 0);
      }
    }
    // dvt/dkt: register r <-> dim crow(r, hf), lane <-> key: four 4-dim (8-byte) stores per row
    if (kj < Lk) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = (bf16_t)(dkt[4 * g4 + e] * scale); c[e] = (bf16_t)dvt[4 * g4 + e]; }
        const int d0 = 8 * g4 + 4 * hf;
        *reinterpret_cast<bf16x4*>(dk + ((long)b * Lk + kj) * lddk + h * AD + d0) = a;
        *reinterpret_cast<bf16x4*>(dv + ((long)b * Lk + kj) * lddv + h * AD + d0) = c;
      }
    }
  }
  __syncthreads();                                      // every wave's dS stores have retired

  // ---------------- dQ phase: this wave's 32 queries, all keys: dQ = dS K, both operands through transposing reads of images whose
  // rows are keys (k-slots in the same order).  One wave sums a query row over the key tiles in ascending order.
  for (int q0 = wave * 32; q0 < Lq; q0 += nwave * 32) {
    const unsigned char* Sq = Si + (long)q0 * LkP * 2;  // query tile q0 / 32 of the image
    f32x16 dqa;
#pragma unroll
    for (int r = 0; r < 16; ++r) dqa[r] = 0.f;
#pragma unroll
    for (int kb16 = 0; kb16 < LkP; kb16 += 16)
      dqa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols_tr(Sq, kb16, lane), frag_cols_tr(Ki, kb16, lane), dqa, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = q0 + crow(r, hf);
      if (qr < Lq) dq[((long)b * Lq + qr) * lddq + h * AD + (lane & 31)] = (bf16_t)(dqa[r] * scale);
    }
  }
}

template <typename K>
static int set_attr_once(K kern, bool& done, size_t bytes, const char* what) {
  if (done) return 0;
  done = true;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    set_error("%s: hipFuncSetAttribute failed: %s", what, hipGetErrorString(e));
    return 1;
  }
  return 0;
}

static bool aligned_ok(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 7) == 0; }

// The envelopes of the MFMA kernels, as host predicates: the launch paths below and sedt_attention_describe (which runs the same
// launch paths in describe mode) decide with them.  Forward: both lengths within 8 tiles of 32, q / k / v rows readable as 16-byte
// chunks (o and lse are written element by element).  Returns the key tile count, 0 when outside.
static int attn_fwd_mfma_tiles(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int Lq, int Lk) {
  if (Lk < 1 || Lq < 1 || Lk > 32 * AMAXT || Lq > 32 * AMAXT) return 0;
  if (!aligned_ok(q, ldq) || !aligned_ok(k, ldk) || !aligned_ok(v, ldv)) return 0;
  return (Lk + 31) / 32;
}
// Backward: a 4 x 4 matrix of tile counts; q / k / v / dO staged and o read (the delta pre-pass) as 16-byte chunks, dk / dv written
// as 8-byte groups (dq element by element)
static bool attn_bwd_mfma_fits(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                               int64_t ldo, const void* dout, int64_t lddo, const void* dk, int64_t lddk, const void* dv, int64_t lddv,
                               int Lq, int Lk) {
  if (Lk < 1 || Lq < 1 || Lk > 128 || Lq > 128) return false;              // template matrix kept small: 4 x 4 tile counts
  if (!aligned_ok(q, ldq) || !aligned_ok(k, ldk) || !aligned_ok(v, ldv) || !aligned_ok(dout, lddo) || !aligned_ok(o, ldo)) return false;
  if ((lddk & 3) || (lddv & 3) || (reinterpret_cast<uintptr_t>(dk) & 7) || (reinterpret_cast<uintptr_t>(dv) & 7)) return false;
  return true;
}

// returns -1 if outside the envelope (caller falls back to the generic kernels)
int attn_fwd_mfma_try(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                      float* lse, const uint8_t* kpm, const float* amask, int B, int H, int Lq, int Lk, float drop_p,
                      uint32_t seed, const uint32_t* seed_ptr, hipStream_t st) {
  const int nt = attn_fwd_mfma_tiles(q, ldq, k, ldk, v, ldv, Lq, Lk), LqP = (Lq + 31) & ~31;
  if (nt == 0) return -1;
  const int nwave = 4;     // all four waves stage K/V/Q; waves beyond the query tiles then idle
  const size_t lds = (size_t)(2 * nt * 32 + LqP) * AROW + (size_t)(nt * 32 + nwave * 32) * sizeof(float);
  const float scale = 1.f / sqrtf((float)AD);
  const uint32_t th = drop_p > 0.f ? drop_threshold(drop_p) : 0u;
  const float ik = 1.f / (1.f - drop_p);
  dim3 grid(B * H), block(64 * nwave);
#define SEDT_AF1(NT_, AM_)                                                                                                 \
  {                                                                                                                        \
    SEDT_DESCRIBE("attn_fwd_mfma_kernel<%d, %s>", NT_, AM_ ? "true" : "false");                                            \
    static bool done = false;                                                                                              \
    if (set_attr_once(attn_fwd_mfma_kernel<NT_, AM_>, done, 64 * 1024, "attention_fwd")) return 1;                         \
    hipLaunchKernelGGL((attn_fwd_mfma_kernel<NT_, AM_>), grid, block, lds, st, (const bf16_t*)q, (long)ldq, (const bf16_t*)k, \
                       (long)ldk, (const bf16_t*)v, (long)ldv, (bf16_t*)o, (long)ldo, lse, kpm, amask, H, Lq, Lk, scale,   \
                       th, ik, seed, seed_ptr);                                                                            \
  }
#define SEDT_AF(NT_)                                                                                                       \
  case NT_:                                                                                                                \
    if (amask) SEDT_AF1(NT_, true) else SEDT_AF1(NT_, false)                                                               \
    break;
  switch (nt) {
    SEDT_AF(1) SEDT_AF(2) SEDT_AF(3) SEDT_AF(4) SEDT_AF(5) SEDT_AF(6) SEDT_AF(7) SEDT_AF(8)
    default: return -1;
  }
#undef SEDT_AF
#undef SEDT_AF1
  return check_launch("attention_fwd_mfma");
}

template <int NTQ>
static int launch_bwd_q(int ntk, dim3 grid, dim3 block, size_t lds, hipStream_t st, const void* q, int64_t ldq, const void* k,
                        int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo, const void* dout, int64_t lddo,
                        const float* lse, const uint8_t* kpm, const float* amask, void* dq, int64_t lddq, void* dk, int64_t lddk,
                        void* dv, int64_t lddv, int H, int Lq, int Lk, float scale, uint32_t th, float ik, uint32_t seed,
                        const uint32_t* seed_ptr) {
#define SEDT_AB1(NTK_, AM_)                                                                                                \
  {                                                                                                                        \
    SEDT_DESCRIBE("attn_bwd_mfma_kernel<%d, %d, %s>", NTQ, NTK_, AM_ ? "true" : "false");                                  \
    static bool done = false;                                                                                              \
    if (set_attr_once(attn_bwd_mfma_kernel<NTQ, NTK_, AM_>, done, 96 * 1024, "attention_bwd")) return 1;                   \
    hipLaunchKernelGGL((attn_bwd_mfma_kernel<NTQ, NTK_, AM_>), grid, block, lds, st, (const bf16_t*)q, (long)ldq,          \
                       (const bf16_t*)k, (long)ldk, (const bf16_t*)v, (long)ldv, (const bf16_t*)o, (long)ldo,              \
                       (const bf16_t*)dout, (long)lddo, lse, kpm, amask, (bf16_t*)dq, (long)lddq, (bf16_t*)dk, (long)lddk, \
                       (bf16_t*)dv, (long)lddv, H, Lq, Lk, scale, th, ik, seed, seed_ptr);                                 \
  }
#define SEDT_AB(NTK_)                                                                                                      \
  case NTK_:                                                                                                               \
    if (amask) SEDT_AB1(NTK_, true) else SEDT_AB1(NTK_, false)                                                             \
    break;
  switch (ntk) {
    SEDT_AB(1) SEDT_AB(2) SEDT_AB(3) SEDT_AB(4)
    default: return -1;
  }
#undef SEDT_AB
#undef SEDT_AB1
  return check_launch("attention_bwd_mfma");
}

int attn_bwd_mfma_try(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                      int64_t ldo, const void* dout, int64_t lddo, const float* lse, const uint8_t* kpm, const float* amask,
                      void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int B, int H, int Lq, int Lk,
                      float drop_p, uint32_t seed, const uint32_t* seed_ptr, hipStream_t st) {
  if (!attn_bwd_mfma_fits(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dk, lddk, dv, lddv, Lq, Lk)) return -1;
  const int ntq = (Lq + 31) / 32, ntk = (Lk + 31) / 32;
  // Q / dO and K / V images, lse / delta / key bias, the dS image (at most 32 KB; 65.5 KB in all at 4 x 4: two workgroups per CU)
  const size_t lds = (size_t)(2 * ntq * 32 + 2 * ntk * 32) * AROW + (size_t)(2 * ntq * 32 + ntk * 32) * sizeof(float) +
                     (size_t)(ntq * 32) * (ntk * 32) * sizeof(bf16_t);
  const int nwave = std::min(4, std::max(ntq, ntk));
  const float scale = 1.f / sqrtf((float)AD);
  const uint32_t th = drop_p > 0.f ? drop_threshold(drop_p) : 0u;
  const float ik = 1.f / (1.f - drop_p);
  dim3 grid(B * H), block(64 * nwave);
#define SEDT_ARGS ntk, grid, block, lds, st, q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, lse, kpm, amask, dq, lddq, dk, lddk, dv, \
                  lddv, H, Lq, Lk, scale, th, ik, seed, seed_ptr
  switch (ntq) {
    case 1: return launch_bwd_q<1>(SEDT_ARGS);
    case 2: return launch_bwd_q<2>(SEDT_ARGS);
    case 3: return launch_bwd_q<3>(SEDT_ARGS);
    case 4: return launch_bwd_q<4>(SEDT_ARGS);
    default: return -1;
  }
#undef SEDT_ARGS
}

}  // namespace sedt

