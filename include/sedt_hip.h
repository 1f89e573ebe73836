/* sedt_hip.h - C ABI of libsedt_hip.so, the MI355X (gfx950) implementation of the
 * SEDT forward/backward hot path.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t (passed as
 * void*); no torch types cross this boundary.  All buffers (inputs, parameters,
 * gradients, outputs, saved activations, workspaces) are owned by the caller; the
 * library never allocates or frees device memory and keeps no pointer across calls
 * (the weight-pack cache in a plan handle stores host-side copies of pointer VALUES
 * only, to detect changes).  Return value: 0 = ok, non-zero = error;
 * sedt_last_error() returns the message (thread-local).  No exception crosses the ABI.
 *
 * dtype codes: SEDT_F32 = parity mode (f32 operands, v_mfma_f32_32x32x2_f32, exact f32
 * FMA chains); SEDT_BF16 = throughput mode (bf16 operands, f32 accumulate,
 * v_mfma_f32_32x32x16_bf16).  Parameters and gradients are always f32.
 *
 * Binding: the library is built with plain `hipcc -shared` and bound with ctypes (sound_event_detection_transformer_amd/
 * lib.py mirrors every prototype below); no torch headers are involved - torch only supplies device pointers and streams.
 *
 * Reference interface each group replaces (file:line under the reference repo):
 *   sedt_igemm / sedt_igemm_group / sedt_wgrad_group / sedt_multi_wgrad_reduce / sedt_skinny_linear_*
 *        torch.nn.Conv2d / Linear forward + autograd: sedt/transformer.py:160-165, 183-204, 220-233, 248-284,
 *        sedt/sedt.py:36, 88-92, 398-409, torchvision Bottleneck convs behind sedt/backbone.py:98-100
 *   sedt_bn_fold / sedt_multi_bn_fold / sedt_pack_conv / sedt_multi_pack      FrozenBatchNorm2d     sedt/backbone.py:17-53
 *   sedt_stem_* / sedt_maxpool_* / sedt_avgpool / sedt_mask_resize            Backbone.forward      sedt/backbone.py:56-113
 *   sedt_layernorm_* / sedt_attention_* / sedt_add / sedt_dropout_grad        TransformerEncoder/DecoderLayer  sedt/transformer.py:155-297
 *   sedt_posenc                                                               PositionEmbeddingSine sedt/position_encoding.py:27-47
 *   sedt_match_targets / sedt_hungarian_batch                                 HungarianMatcher      sedt/matcher.py:41-133
 *   sedt_set_criterion(_bwd) / sedt_feature_loss                              SetCriterion          sedt/sedt.py:134-352
 *   sedt_postprocess / sedt_pseudo_labels                                     PostProcess, get_pseudo_labels  sedt/sedt.py:355-396, engine.py:300-348
 *   sedt_event_metrics_update                                                 decode_strong + sed_eval event-based / clip-level counts
 *                                                                             utilities/BoxEncoder.py:179-226, engine.py:199-297,
 *                                                                             utilities/metrics.py:43-80, 281-322
 *   sedt_event_segment_metrics_update                                         + sed_eval segment-based counts  utilities/metrics.py:83-116
 *   sedt_decode_events                                                        decode_strong + the clip, written out as event records
 *                                                                             utilities/BoxEncoder.py:179-226, engine.py:218-297
 *   sedt_decode_events_classwise                                              the same with one threshold per class (the reference's
 *                                                                             classwise_threshold, engine.py:300-348, applied to decode_strong)
 *   sedt_event_sweep_update                                                   sed_eval event-based / clip-level counts at every operating
 *                                                                             point, from those event records  utilities/metrics.py:43-80, 281-322
 *   sedt_psds_update                                                          PSDS confusion counts from those event records
 *                                                                             utilities/metrics.py:120-145, 325-330 (psds_eval)
 *   sedt_stitch_events                                                        no counterpart (the reference scores 10 s clips only):
 *                                                                             the windows' event records -> one list per recording
 *   sedt_stitch_stream / sedt_stream_reset / sedt_stream_append / sedt_stream_cut   no counterpart: live streams - waveform rings on
 *                                                                             the device, the same sweep one window per launch
 *   sedt_recording_event_counts / sedt_recording_segment_counts               no counterpart: those lists against a recording's annotations,
 *                                                                             sed_eval's event- and segment-based counts at every threshold
 *   sedt_recording_psds_counts                                                no counterpart: PSDS confusion counts from those lists
 *   sedt_cut_clips                                                            no counterpart as a kernel: training windows and their
 *                                                                             target tables cut from recordings on the device
 *   sedt_bank_stats / sedt_soundscape                                         no counterpart as a kernel: training soundscapes mixed from
 *                                                                             a sound bank on the device, targets merged per class
 *                                                                             as data_utils/collapse_event.py merges annotations
 *   sedt_loudness / sedt_scale_sources                                        no counterpart: ITU-R BS.1770 loudness (K-weighted, gated)
 *                                                                             of the sources of a bank, and gains applied in place
 *   sedt_stretch / sedt_stretch_workspace / sedt_stretch_ok                   no counterpart: per-event time stretch and pitch shift
 *                                                                             (phase vocoder, then resampling at a real ratio)
 *   sedt_reverb / sedt_reverb_spectra / sedt_reverb_workspace / sedt_reverb_ok no counterpart: per-event reverberation with room
 *   / sedt_reverb_bed                                                         impulse responses (partitioned FFT convolution)
 *   sedt_relevel / sedt_relevel_workspace                                     no counterpart: the level of every processed event (RMS or
 *                                                                             BS.1770) measured on the device, its gain written into the
 *                                                                             device records before they are mixed
 *   sedt_mixup_plan                                                           mixup_data's label half  utilities/mixup.py:30-127
 *   sedt_multi_sumsq / sedt_multi_adamw / sedt_adamw_clip                     clip_grad_norm_ + AdamW.step  engine.py:77-80
 *   sedt_multi_ema                                                            EMA.update            utilities/utils.py:62-67
 *   sedt_multi_gather                                                         DDP gradient buckets  train_spsedt.py:157-158
 */
#ifndef SEDT_HIP_H
#define SEDT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEDT_F32 0
#define SEDT_BF16 1
/* GEMM entry points only (sedt_igemm, sedt_igemm_group, sedt_wgrad_group, sedt_igemm_splitk): f32 tensors exactly as SEDT_F32, but
 * every product computed from bf16 hi / lo splits of both operands - hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16, f32
 * accumulation - instead of v_mfma_f32_32x32x2_f32: ~2^-16 relative error per product, about five times the matrix rate of the
 * exact-f32 mode.  The "bf16x3" compute mode (runtime.set_compute_dtype('bf16x3')): f32 activations and gradients everywhere,
 * this code for the contractions; meets the 1e-3 parity tolerance (tests/test_x3_gpu.py). */
#define SEDT_BF16X3 2
/* sedt_mel_spectrogram only: the waveform as 16-bit PCM, a sample worth x / 32768 */
#define SEDT_I16 3

#define SEDT_ACT_NONE 0
#define SEDT_ACT_RELU 1
#define SEDT_ACT_SIGMOID 2

const char* sedt_last_error(void);
int sedt_version(void);

/* ------------------------------------------------------------------ implicit GEMM
 * C[M,N] = epilogue( sum_k A(m,k) * B(n,k) )
 *
 * trans == 0 (forward / dgrad):
 *   A(m,k): conv == 0: A[m*lda + k]
 *           conv == 1: m = (img, ho, wo) over the Ho x Wo "row grid", k = (tap, c) with c < Ci,
 *                      element = A[pix*lda + c], pix = gathered pixel of the Hi x Wi grid:
 *                        transposed == 0: hi = ho*sh - ph + kh*dh        (convolution forward)
 *                        transposed == 1: hi = (ho + ph - kh*dh)/sh      (dgrad: rows are input pixels)
 *                      out-of-range / non-divisible taps read as 0.
 *   B(n,k): B[n*ldb + k]    (weights packed [N][taps][Ci])
 * trans == 1 (wgrad; the reduction runs over pixels):
 *   A(m,k): A[k*lda + m]                      (dY: k = output pixel, m = output channel)
 *   B(n,k): conv == 0: B[k*ldb + n]
 *           conv == 1: n = (tap, c), element = B[pix(k,tap)*ldb + c] (forward gather)
 *   splitk > 1: partial sums go to slab[z][M][N] (f32) and the epilogue is skipped.
 *
 * epilogue, in order: v = acc*scale[n] + bias[n]; if(!act_post_res) v = act(v);
 *   dropout(v); v += res[(res_mod ? m % res_mod : rmap ? coarse(m) : m)*ldr + n] (rmap: only where m lies on the coarse grid, see
 *   SedtIgemm.rmap); if(act_post_res) v = act(v);
 *   v = mask[m*ldm+n] > 0 ? v : 0; v *= alpha; store as f32 (out_f32) or the compute dtype.
 * 1-bit ReLU masks (round 3): a backward pass needs only the SIGN of a saved post-ReLU activation.  mask_bits != 0: `mask` is a
 *   uint8 bit image - bit (n & 7) of mask[m*ldm + (n >> 3)], ldm in BYTES - instead of the activation itself (1/16 of the bytes of a
 *   bf16 tensor); bits_out != null: the same image of the value stored to C (bit = v > 0) is written to bits_out[m*ldbits + (n >> 3)]
 *   (N must be a multiple of 8).  trans == 0 only.
 */
typedef struct SedtIgemm {
  int32_t M, N, K;
  const void* A;
  const void* B;
  int64_t lda, ldb;
  int32_t trans, conv, transposed;
  int32_t Hi, Wi, Ci, Ho, Wo;
  int32_t KH, KW, sh, sw, ph, pw, dh, dw;
  void* C;
  int64_t ldc;
  int32_t out_f32;
  const float* scale;
  const float* bias;
  const void* res;
  int64_t ldr;
  int32_t res_mod;
  const void* mask;
  int64_t ldm;
  int32_t act, act_post_res;
  float alpha;
  float drop_p;
  uint32_t seed;            /* effective seed = seed + (seed_ptr ? *seed_ptr : 0): the device word */
  const uint32_t* seed_ptr; /* lets a captured hipGraph draw a fresh mask on every replay */
  int32_t splitk;
  float* slab;
  int32_t tile_m, tile_n; /* 0 = choose automatically; else 64 or 128 */
  float* colsum_out;      /* trans == 1, bf16 LDS-DMA kernel only: if non-null, per-split column sums of A over the
                             reduction axis (= the bias gradient sum_pix dY[pix][m]) are written to colsum_out[z][M];
                             sedt_wgrad_reduce adds them up.  sedt_igemm fails if the fast kernel cannot take the problem. */
  uint8_t* bits_out;      /* or null: sign bits of the stored output (see "1-bit ReLU masks") */
  int64_t ldbits;         /* bytes per row of bits_out */
  int32_t mask_bits;      /* != 0: `mask` is a bit image, ldm in bytes */
  int32_t f32ep;          /* bf16 operands with an f32 epilogue (the fast bf16x3 mode, sedt_split3): C (out_f32 must be set), res and a
                             non-bit mask are f32 tensors (ldc / ldr / ldm in f32 elements); trans == 0, LDS-DMA kernels only */
  /* conv problems on the LDS-DMA kernels only (a parity class of a stride-2 input gradient, ops.conv_dgrad): */
  int32_t omap;           /* != 0: GEMM row (n, ho, wo) of the Ho x Wo grid is pixel (ho * o_sh + o_h0, wo * o_sw + o_w0) of an o_Hi x o_Wi
                             image: C, res, mask, bits_out are indexed by that pixel */
  int32_t o_Hi, o_Wi, o_sh, o_sw, o_h0, o_w0;
  int32_t btap_on;        /* != 0: tap t of the (<= 8-tap) walk reads the Ci channels starting at element btap[t] of a B row (ldb spans
                             all the taps the packed weight holds) */
  int32_t btap[8];
  void* split_out;        /* f32ep only, or null: bf16 [M][2 N] = the [hi | lo] operand image (sedt_split3, pattern 0) of the stored
                             output, written by the epilogue - the GEMMs that consume this output then need no split pass */
  int32_t awrap;          /* bf16x3, trans == 0: the A rows hold [hi | lo] = 2 awrap channels while the contraction walks 3 awrap per pixel
                             (K = 3 awrap, a convolution: Ci = 3 awrap): the last third re-reads hi.  0 = off */
  int32_t rmap;           /* != 0: the residual lives on a coarser grid (the input gradient of a stride-s 1x1 projection, held as the plain
                             GEMM on the projection's OUTPUT grid).  Packed r_Hi | r_Wi << 12 | r_sh << 24 | r_sw << 28 (r_Hi, r_Wi <= 4095,
                             1 <= r_sh, r_sw <= 15; SEDT_RMAP below): the output pixel - the GEMM row, or the omap-mapped row - is pixel
                             (n, h, w) of an r_Hi x r_Wi image and takes res[((n * rH + h / r_sh) * rW + w / r_sw) * ldr + col], rH =
                             (r_Hi - 1) / r_sh + 1, rW = (r_Wi - 1) / r_sw + 1, when r_sh divides h and r_sw divides w - and NO residual
                             otherwise (it stores the bits of the same launch without `res`).  trans == 0, res_mod == 0, fewer than 2^24
                             output pixels, a whole number of images; every kernel that reads `res` honours it, an entry point that
                             cannot fails.  One packed word in the former padding: the struct keeps its size - ten of them travel in
                             the kernel arguments of a grouped weight-gradient launch */
  const void* bfrag;      /* or null: the fragment-major image (sedt_pack_frag) of the WHOLE B operand [N][ldb] (trans == 0, bf16): kernels
                             that stream B from L2 into registers read it instead of B (developer build only so far) */
} SedtIgemm;
#define SEDT_RMAP(r_Hi, r_Wi, r_sh, r_sw) ((int32_t)((uint32_t)(r_Hi) | (uint32_t)(r_Wi) << 12 | (uint32_t)(r_sh) << 24 | (uint32_t)(r_sw) << 28))

int sedt_igemm(const SedtIgemm* args, int dtype, void* stream);
/* sizeof of an argument struct as THIS library was compiled (0 SedtIgemm, 1 SedtReduceJob, 2 SedtSplitJob, 3 SedtPrefetch, 4 SedtCriterion,
 * 5 SedtMatch, 6 SedtChunk, 7 SedtBnJob, 8 SedtPackJob, 9 SedtFragJob, 10 SedtPoolAt, 11 SedtCopyJob, 12 SedtViewAug; -1 otherwise): lets a binding verify its mirror of the structs */
int sedt_sizeof(int which);
/* njobs (<= 8 per launch) independent trans == 0 problems - e.g. the q / k / v projections of an attention block; one
 * launch when every problem resolves to the 64x64 2-stage bf16 kernel, otherwise njobs sedt_igemm calls.  HOST array. */
int sedt_igemm_group(const SedtIgemm* jobs, int njobs, int dtype, void* stream);
/* njobs independent trans == 1 (weight-gradient) problems; in bf16 they run as ONE launch (grouped workgroup ranges) when
 * every problem fits the LDS-DMA kernel, otherwise this is njobs sedt_igemm calls.  `jobs` is a HOST array. */
int sedt_wgrad_group(const SedtIgemm* jobs, int njobs, int dtype, void* stream);
/* one forward / dgrad problem (`main`, trans == 0) plus nw <= 10 weight-gradient problems in ONE launch: the wgrad tiles run
 * in workgroup slots the main problem leaves idle (co-scheduling).  *taken = 1: semantically sedt_igemm(main) +
 * sedt_wgrad_group(wjobs); *taken = 0: only `main` was launched (its kernel configuration cannot carry riders, or a rider
 * is outside the grouped kernel's envelope) and the caller still owns the weight-gradient problems. */
int sedt_igemm_co(const SedtIgemm* main, const SedtIgemm* wjobs, int nw, int dtype, void* stream, int* taken);
/* recommended split-K factor and slab bytes for a trans==1 problem */
int sedt_igemm_splitk(int M, int N, int K, int dtype);
/* measurement aid: the name of the kernel instance the problem runs on - as rocprofv3 prints it, e.g. "igemm3_w16_kernel<64, 128, 3>" -
 * through sedt_igemm (grouped = 0) or through sedt_wgrad_group (grouped = 1, trans problems).  Nothing is launched.  bench.py joins
 * these names with the per-kernel times of the measured step to price every kernel family against its roofline. */
int sedt_igemm_describe(const SedtIgemm* args, int dtype, int grouped, char* out, int cap);
/* the same for sedt_igemm_group: the ONE kernel instance the njobs problems run on as a group ("igemm3_group_kernel<2>",
 * "igemm3_w8_group_kernel<128, 128, 3>"), or "" when the dispatcher would launch them one by one */
int sedt_igemm_group_describe(const SedtIgemm* jobs, int njobs, int dtype, char* out, int cap);

/* out[r][c...] = rowscale[r] * sum_z slab[z][r][tap][c], written in (R, Ci, taps) order
 * (the torch (Cout, Cin, KH, KW) parameter layout) as f32.  taps == 1: plain [R][Ci]. */
int sedt_wgrad_reduce(const float* slab, int splitk, int R, int taps, int Ci, const float* rowscale,
                      float* out, void* stream);
/* same, plus bias_out[r] = sum_z colsum_slab[z][r] (no rowscale) when colsum_slab is non-null */
int sedt_wgrad_reduce_bias(const float* slab, int splitk, int R, int taps, int Ci, const float* rowscale, float* out,
                           const float* colsum_slab, float* bias_out, void* stream);

/* A prefetch hint, passed BY THE LAUNCH THAT CONSUMES IT (the library keeps no pointers between calls): up to three regions (null /
 * bytes 0 = none) that the launch AFTER this one will stream - fragment-major weights.  The launch touches one 128-byte line of them
 * per load so that every XCD's L2 holds them when the streaming launch starts.  Taken by sedt_encoder_qkv_fwd (the weights of
 * sedt_encoder_attn_ffn_fwd), sedt_bneck3_fwd / sedt_bneck3_bwd (the next block's operands) and sedt_multi_wgrad_reduce (what the next
 * layer's backward streams first); `pf` may be null. */
typedef struct SedtPrefetch {
  const void* ptr[3];
  size_t bytes[3];
} SedtPrefetch;

/* Operand preparation of the fast bf16x3 mode (csrc/split3.hip): src f32 [rows][cols] (row stride ld) -> bf16, hi = bf16(x), lo = bf16(x - hi):
 *   pattern 0 (an activation / gradient operand): dst [rows][2 * cols] = [hi | lo] - the bytes of the f32 tensor;
 *   pattern 1 (a weight operand; rows = Cout * taps, cols = Cin): dst [rows][3 * cols] = [hi | hi | lo].
 * A bf16 GEMM whose contraction walks hi, lo, hi of the activation (SedtIgemm.awrap: the last third wraps back onto hi) against
 * [hi | hi | lo] of the weight yields hi hi + lo hi + hi lo in its f32 accumulator: an f32 product to ~2^-16 at bf16 MFMA rate (with
 * SedtIgemm.f32ep for the epilogue).  Up to 8 jobs per launch (HOST array, copied into the kernel arguments).  cols and ld multiples of 4,
 * src 16-byte aligned. */
typedef struct SedtSplitJob {
  const float* src;
  int64_t ld;
  void* dst;
  int32_t rows, cols, pattern;
  int32_t blk0;           /* filled by the library */
} SedtSplitJob;
int sedt_split3(const SedtSplitJob* jobs, int njobs, void* stream);

/* up to SEDT_MAX_REDUCE_JOBS split-K reductions in ONE launch (jobs are copied into the kernel arguments, so a captured
 * graph holds them by value).  `jobs` is a HOST array; fields as the arguments of sedt_wgrad_reduce_bias. */
#define SEDT_MAX_REDUCE_JOBS 40
typedef struct SedtReduceJob {
  const float* slab;
  const float* rowscale;
  float* out;
  const float* colsum_slab;
  float* bias_out;
  int32_t splitk, R, taps, Ci;
  int32_t blk0;           /* filled by the library */
  int32_t cs_splitk;      /* slices of colsum_slab when they differ from splitk (0 = splitk) */
} SedtReduceJob;
int sedt_multi_wgrad_reduce(const SedtReduceJob* jobs, int njobs, const SedtPrefetch* pf, void* stream);

/* ------------------------------------------------------------------ linear layers with N <= 16 outputs (the SEDT heads,
 * sedt/sedt.py:36-38, 90-95, 398-409): direct kernels on the f32 MASTER weight w[N][K] (no packing).
 * fwd: y[m][n] = act(x[m] . w[n] + bias[n]); y is f32 (out_f32) or the compute dtype.
 * bwd: g[M][N] f32 is the gradient of y; with act != NONE the derivative is folded in from ysaved (= y, f32, same ld as g).
 *      gx (compute dtype, optional; masked by mask > 0 when given) = g' w - or gx += g' w when accumulate_gx != 0 (a head that
 *      shares its input with other heads adds to the running input gradient; rows ldo apart, so a strided row subset works);
 *      dw[N][K], db[N] (optional) = g'^T x, column sums.  With scratch given and dw NULL only the partial sums are left in
 *      scratch as [16 slabs][17][K] (rows 0..15 dW, row 16 = the bias sums in its first 16 entries): the caller adds the slabs. */
int sedt_skinny_linear_fwd(const void* x, int64_t ldx, const float* w, const float* bias, void* y, int64_t ldy, int M, int N,
                           int K, int act, int out_f32, int dtype, void* stream);
size_t sedt_skinny_linear_bwd_scratch(int K); /* bytes of `scratch` (row-slice partial sums) when dw is requested */
int sedt_skinny_linear_bwd(const float* g, const float* ysaved, int64_t ldg, const float* w, const void* x, int64_t ldx,
                           const void* mask, int64_t ldm, void* gx, int64_t ldo, float* dw, float* db, float* scratch, int M, int N,
                           int K, int act, int accumulate_gx, int dtype, void* stream);

/* ------------------------------------------------------------------ elementwise / reductions */
/* out[c] = sum_r in[r*ld + c]   (in: compute dtype or f32 if in_f32), out f32 */
int sedt_colsum(const void* in, int64_t ld, int rows, int cols, int in_f32, int dtype, float* out,
                float* scratch, size_t scratch_bytes, void* stream);
size_t sedt_colsum_scratch(int rows, int cols);
/* out = in * keep(seed, r*cols+c) / (1-p)   - the gradient side of the epilogue dropout */
int sedt_dropout_grad(const void* in, int64_t ldi, void* out, int64_t ldo, int rows, int cols, float p,
                      uint32_t seed, const uint32_t* seed_ptr, int dtype, void* stream);
/* out[r][c] = a[r][c] + b[(b_mod ? r % b_mod : r)][c] */
int sedt_add(const void* a, const void* b, void* out, int rows, int cols, int b_mod, int dtype, void* stream);
/* out = srcs[0] + ... + srcs[n-1] (n <= 8 equally shaped tensors of the compute dtype, numel a multiple of 8; srcs is a HOST array of
 * device pointers): the gradient of a tensor with several consumers in one launch */
int sedt_add_n(const void* const* srcs, int n, void* out, int64_t numel, int dtype, void* stream);
/* dtype conversion f32 <-> compute dtype, elementwise over n */
int sedt_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, void* stream);
/* out = y > 0 ? g : 0 (ReLU backward), compute dtype, elementwise over n */
int sedt_relu_mask(const void* g, const void* y, void* out, int64_t n, int dtype, void* stream);
/* up to 8 strided 2-D copies in one launch (jobs: HOST array, copied into the kernel arguments): `outer` items of `inner` bytes (multiple of 4),
 * src_stride / dst_stride bytes apart.  The clip-range split of the stacked head outputs [L][B][Q][C] between the two criterion calls of the
 * mean-teacher step (reference engine.py:134-165 computes a supervised and an unsupervised loss on two forwards; here ONE student forward
 * covers both clip sets) and the merge of their gradients are one launch each. */
typedef struct SedtCopyJob {
  const void* src;
  void* dst;
  int64_t src_stride, dst_stride;
  int32_t outer, inner;
  int32_t blk0;           /* filled by the library */
  int32_t pad_;
} SedtCopyJob;
int sedt_copy2d(const SedtCopyJob* jobs, int njobs, void* stream);
/* SP-SEDT decoder input, reference sedt/spsedt.py:48-69 in one launch each way.  patch [B*P][D] (compute dtype: patch2query of the pooled patch
 * features), query f32 [Q][D] (query_embed.weight rows from `start`), out [B*Q][D] token-major (compute dtype):
 *   train: out[b][q] = 2 * query[q] + keep(q, b) * patch[b][q / qpp]     eval: out[b][q] = query[q] + patch[b][q / qpp]
 * keep_in f32 [Q][B] (may be NULL): the Bernoulli(1 - ratio) query-patch mask of spsedt.py:65; NULL = drawn from the counter hash of
 * (seed (+ *seed_ptr), q * B + b), ratio <= 0 keeps every patch.  keep_out f32 [Q][B] (may be NULL) receives the mask used.
 * Backward: d_patch [B*P][D] (compute dtype, may be NULL) = sum over the qpp queries of a patch of keep * g; d_query f32 [Q][D] =
 * (train ? 2 : 1) * sum_b g[b][q], a fixed-order sum (four consecutive clip ranges added in clip order, then the four partials in range
 * order).  D a multiple of 8 (forward); a multiple of 64, <= 256 (backward). */
int sedt_spsedt_dec_in(const void* patch, const float* query, const float* keep_in, float* keep_out, void* out, int B, int Q, int P, int qpp,
                       int D, int train, float ratio, uint32_t seed, const uint32_t* seed_ptr, int dtype, void* stream);
int sedt_spsedt_dec_in_bwd(const void* g, const float* keep, void* d_patch, float* d_query, int B, int Q, int P, int qpp, int D, int train,
                           int dtype, void* stream);
/* the FFN activation "gelu" of reference sedt/transformer.py:423-431 (F.gelu, erf form) with the FFN's dropout behind it
 * (transformer.py:187 / :203: dropout(activation(linear1(x)))):  a = keep(seed, e) * gelu(h) / (1-p);
 * backward: out = keep(seed, e) * g * gelu'(h) / (1-p).  h is the saved PRE-activation.  Elementwise over n (a multiple of 8) in the
 * compute dtype; the keep decision is the GEMM epilogue's (seed, element index) hash; p = 0: no dropout */
int sedt_gelu_fwd(const void* h, void* a, int64_t n, float p, uint32_t seed, const uint32_t* seed_ptr, int dtype, void* stream);
int sedt_gelu_bwd(const void* g, const void* h, void* out, int64_t n, float p, uint32_t seed, const uint32_t* seed_ptr, int dtype,
                  void* stream);
/* y = g * s * (1 - s) (sigmoid backward), all f32 */
int sedt_sigmoid_grad(const float* g, const float* s, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------ LayerNorm (width D = 256 or 512)
 * y = (x-mean)*rstd*gamma+beta ; y2 = y + add (optional) ; saves mean/rstd.  eps = 1e-5.
 * Rows are contiguous (D elements apart) and every lane moves its D / 64 features as one vector: the row tensors (x, add, y, y2; dy, dy2,
 * dres, dres2, dx, dx_drop) must be aligned to D / 64 elements of the dtype, gamma and beta to D / 64 floats - otherwise an error, no launch. */
int sedt_layernorm_fwd(const void* x, const float* gamma, const float* beta, const void* add, void* y, void* y2,
                       float* mean, float* rstd, int rows, int D, int dtype, void* stream);
/* dx = dres + LN'(dy (+dy2)); dgamma/dbeta: f32[D] (deterministic two-stage reduction) */
int sedt_layernorm_bwd(const void* dy, const void* dy2, const void* x, const float* gamma, const float* mean,
                       const float* rstd, const void* dres, void* dx, float* dgamma, float* dbeta, float* scratch,
                       size_t scratch_bytes, int rows, int D, int dtype, void* stream);
size_t sedt_layernorm_bwd_scratch(int rows, int D);
/* same, with a second output dx_drop = dropout-backward of dx under (drop_p, seed): the gradient entering the sub-layer
 * whose dropped output fed this LayerNorm (post-norm layers, reference transformer.py:186-189) - saves the separate
 * sedt_dropout_grad launch.  dx_drop may be NULL.  dres2 (may be NULL): a second gradient added to dx - the share of another
 * consumer of x (a decoder layer's output also feeds the shared final LayerNorm, transformer.py:134-147). */
int sedt_layernorm_bwd_drop(const void* dy, const void* dy2, const void* x, const float* gamma, const float* mean,
                            const float* rstd, const void* dres, const void* dres2, void* dx, float* dgamma, float* dbeta,
                            float* scratch, size_t scratch_bytes, int rows, int D, void* dx_drop, float drop_p, uint32_t seed,
                            const uint32_t* seed_ptr, int dtype, void* stream);
/* second stage of sedt_layernorm_bwd on its own (call sedt_layernorm_bwd with dgamma = dbeta = NULL first): reduces the
 * per-workgroup partial sums in `scratch` to dgamma / dbeta.  Lets a caller move the parameter-gradient half off the
 * critical path of the backward pass (another stream). */
int sedt_layernorm_bwd_final(const float* scratch, int rows, int D, float* dgamma, float* dbeta, void* stream);

/* ------------------------------------------------------------------ attention (head dim 32)
 * rows are batch-first: q row = b*Lq + i, k/v row = b*Lk + j, head h occupies columns [h*32, h*32+32).
 * kpm: uint8 [B][Lk] (1 = padded key), amask: f32 [Lq][Lk] additive (may hold -inf), both optional.
 * probabilities are dropped with (drop_p, seed); lse [B][H][Lq] f32 saved for backward. */
int sedt_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       void* o, int64_t ldo, float* lse, const uint8_t* kpm, const float* amask, int B, int H,
                       int Lq, int Lk, float drop_p, uint32_t seed, const uint32_t* seed_ptr, int dtype, void* stream);
int sedt_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       const void* o, int64_t ldo, const void* dout, int64_t lddo, const float* lse,
                       const uint8_t* kpm, const float* amask, void* dq, int64_t lddq, void* dk, int64_t lddk,
                       void* dv, int64_t lddv, int B, int H, int Lq, int Lk, float drop_p, uint32_t seed,
                       const uint32_t* seed_ptr, int dtype, void* stream);
/* measurement and test aid, in the manner of sedt_igemm_describe: the name of the kernel instance - as rocprofv3 prints it, e.g.
 * "attn_bwd_mfma_kernel<2, 3, true>", "attn_f32_fwd_kernel<4, false, true>", "attn_fwd_kernel<__bf16>" - that sedt_attention_fwd
 * (backward = 0; dout, dq, dk, dv and their strides are ignored) or sedt_attention_bwd (backward = 1) launches for these pointers,
 * strides, lengths, dropout probability and dtype, with an additive mask present or not.  The entry point itself runs in describe
 * mode, so the answer cannot differ from the launch; nothing is dereferenced (pointers are tested for null and alignment only) and
 * nothing is launched.  A call the entry point refuses gives "" and a non-zero return (sedt_last_error has the reason). */
int sedt_attention_describe(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                            int64_t ldo, const void* dout, int64_t lddo, const void* dq, int64_t lddq, const void* dk,
                            int64_t lddk, const void* dv, int64_t lddv, int has_amask, int Lq, int Lk, float drop_p, int dtype,
                            int backward, char* out, int cap);

/* ------------------------------------------------------------------ position encoding
 * pos[b][h*W+w][c] for the (B,H,W) uint8 mask (1 = padded): sine over the time axis H only,
 * normalised, scale 2*pi, temperature 10000, eps 1e-6, D features interleaved sin/cos. */
int sedt_posenc(const uint8_t* mask, void* pos, int B, int H, int W, int D, int dtype, void* stream);
/* nearest resize of the (B,Hin,Win) padding mask to (B,Hout,Wout): F.interpolate default */
int sedt_mask_resize(const uint8_t* in, uint8_t* out, int B, int Hin, int Win, int Hout, int Wout, void* stream);

/* ------------------------------------------------------------------ backbone pieces */
/* FrozenBatchNorm fold: scale = w*rsqrt(rv+1e-5), bias = b - rm*scale, n channels */
int sedt_bn_fold(const float* w, const float* b, const float* rm, const float* rv, float* scale, float* bias, int n,
                 void* stream);
/* conv weight (Cout,Cin,KH,KW) f32 -> fwd pack [Cout][taps][Cin] and (optional) dgrad pack
 * [Cin][taps][Cout] * bnscale[Cout], both in the compute dtype */
int sedt_pack_conv(const float* w, int Cout, int Cin, int taps, const float* bnscale, void* wf, void* wb, int dtype,
                   void* stream);
/* stem: conv0 (1->3, 1x1, bias) folded into conv1 (3->64, 7x7, s2, p3):
 * prep builds Wcat[64][128] = [Weff(49) | 0(15) | Beff(49) | 0(15)]; im2col builds
 * col[B*Ho*Wo][128] = [x taps | 0 | in-bounds indicators | 0]. */
int sedt_stem_prep(const float* w0, const float* b0, const float* w1, void* wcat, int dtype, void* stream);
int sedt_stem_im2col(const float* x, void* col, int B, int H, int W, int dtype, void* stream);
/* Direct 3x3 convolution, stride 1, pad 1, over NHWC bf16 tokens x [B*H*W][C] with C = 64 channels in and out on a W = 16 wide
 * map (conv2 of the layer1 Bottlenecks, torchvision resnet50 behind sedt/backbone.py:98-111): y = act(conv(x, w) * scale + bias),
 * or, with flip = 1 and w = the dgrad pack [Cin][taps][Cout] (BN scale folded in), the input gradient masked by (mask > 0).
 * w: bf16 [64 out][9 taps][64 in]; scale / bias / mask may be null; relu: 0 / 1. */
int sedt_conv3x3_c64(const void* x, const void* w, int flip, const float* scale, const float* bias, int relu, const void* mask, void* y,
                     int B, int H, int W, int C, void* stream);
/* The whole stem in one launch (bf16, W = 64 mel bands): conv0 o conv1 7x7/s2 o FrozenBN (scale, bias) o ReLU o max-pool 3x3/s2
 * (sedt/backbone.py:98-111 + torchvision stem) from x f32 [B][H][64] to pool bf16 [B*Hp*16][64] + argmax bytes idx (may be
 * null); wcat = sedt_stem_prep's bf16 [64][128]; s1_out (optional, tests): the un-pooled activation [B*Ho*32][64]. */
int sedt_stem_pool_fwd(const float* x, const void* wcat, const float* scale, const float* bias, void* pool, uint8_t* idx,
                       void* s1_out, int B, int H, int W, void* stream);
/* weight gradient of the folded stem convolution from the POOLED gradient g (max-pool backward through the ReLU evaluated on
 * the fly): slab f32 [nslab][64][128] partial sums in wcat's layout, nslab = sedt_stem_pool_wgrad_slabs(B, H); reduce with
 * sedt_wgrad_reduce_bias(slab, nslab, 64, 1, 128, bn_scale, G, ...) and feed G to sedt_stem_conv0_grad */
int sedt_stem_pool_wgrad_slabs(int B, int H);
int sedt_stem_pool_wgrad(const float* x, const void* g, const uint8_t* idx, const void* pool, float* slab, int nslab, int B, int H,
                         int W, void* stream);
/* dw0[c] = sum w1[co,c,tap]*G[co][tap], db0[c] = sum w1[co,c,tap]*G[co][64+tap]; G f32 [64][128] */
int sedt_stem_conv0_grad(const float* G, const float* w1, float* dw0, float* db0, void* stream);
/* 3x3 stride-2 pad-1 max pooling over NHWC; idx (uint8 argmax tap) saved for backward */
int sedt_maxpool_fwd(const void* x, void* y, uint8_t* idx, int B, int H, int W, int C, int dtype, void* stream);
/* dx = (sum of dy routed by idx) * (relu_src > 0 if relu_src) */
int sedt_maxpool_bwd(const void* dy, const uint8_t* idx, const void* relu_src, void* dx, int B, int H, int W, int C,
                     int dtype, void* stream);
/* same with the ReLU mask taken from the pooled output y (NHWC at the pooled resolution; the selected element passed the
 * ReLU exactly when y > 0): pass relu_src = NULL.  Reads a quarter of the bytes and the un-pooled activation need not be kept. */
int sedt_maxpool_bwd_y(const void* dy, const uint8_t* idx, const void* relu_src, const void* y, void* dx, int B, int H, int W,
                       int C, int dtype, void* stream);
/* global average pool over NHWC pixels: out[b][c] = mean_p x[b][p][c] (f32 out) */
int sedt_avgpool(const void* x, float* out, int B, int P, int C, int dtype, void* stream);

/* ------------------------------------------------------------------ optimizer (engine.py:77-80)
 * Flat f32 buffers.  sumsq: f32[1] workspace holding the squared global grad norm (computed by
 * sedt_sumsq), clip_coef = min(1, max_norm/(sqrt(sumsq)+1e-6)) as torch.clip_grad_norm_. */
int sedt_sumsq(const float* g, int64_t n, float* sumsq, float* scratch, size_t scratch_bytes, int accumulate,
               void* stream);
size_t sedt_sumsq_scratch(int64_t n);
int sedt_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* sumsq, float max_norm,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);

/* multi-tensor form: `table` is a DEVICE array of chunks (<= 65536 elements each) covering every parameter tensor;
 * one launch updates them all.  sedt_multi_sumsq writes the squared global gradient norm to sumsq[0]
 * (partial: f32[nchunks] scratch); sedt_multi_adamw applies clip_grad_norm_(max_norm) + AdamW per chunk with the
 * chunk's own lr / weight decay (the reference's two parameter groups, train_sedt.py:234-240). */
typedef struct SedtChunk {
  void* p;
  const void* g;
  void* m;
  void* v;
  int32_t n;
  float lr;
  float wd;
  int32_t gflags; /* bit 0: g addresses bf16 elements (sedt_multi_sumsq / sedt_multi_adamw reading a bf16 flat gradient buffer) */
} SedtChunk;
/* table-driven forms of sedt_bn_fold / sedt_pack_conv: `jobs` is a DEVICE array; one launch serves every FrozenBN layer /
 * every weight tensor of the model.  Pack: one job per tensor (taps <= 9), e0 = index of the tensor's first workgroup
 * (ascending; a tensor takes ceil(Cout/32)*ceil(Cin/32) workgroups, each an LDS-staged 32x32xtaps tile); nblocks = total */
typedef struct SedtBnJob {
  const float* w;
  const float* b;
  const float* rm;
  const float* rv;
  float* scale;
  float* bias;
  int32_t n;
  int32_t pad_;
} SedtBnJob;
typedef struct SedtPackJob {
  const float* w;
  const float* bnscale; /* may be null */
  void* wf;             /* [Cout][taps][Cin] or null */
  void* wb;             /* [Cin][taps][Cout] (* bnscale) or null */
  int64_t e0;
  int32_t ne, Cout, Cin, taps;
} SedtPackJob;
int sedt_multi_bn_fold(const SedtBnJob* jobs, int njobs, void* stream);
int sedt_multi_pack(const SedtPackJob* jobs, int njobs, int nblocks, int dtype, void* stream);

/* ------------------------------------------------------------------ x-stationary ("slab") transformer kernels (csrc/slab.h)
 * A workgroup owns a slab of 32 token rows for a whole chain of sub-layers: activations stay in LDS as the B operand of
 * v_mfma_f32_32x32x16_bf16, and only the WEIGHTS move - from L2 straight into registers as A operands - in a fragment-major
 * packing: W [N][K] (nn.Linear layout; N % 32 == 0, K % 32 == 0) as 1 KB blocks, block (n / 32, k / 16) at byte
 * ((n / 32) * (K / 16) + k / 16) * 1024, inside it lane l = 32 * ((k % 16) / 8) + n % 32 owns 8 consecutive k (16 bytes).
 * sedt_pack_frag packs any number of f32 master weights into that form (wf) and / or the same form of W^T (wb: the operand of the
 * input-gradient chain) in one launch; nblocks = sum over the jobs of (N / 32) * (K / 32), blk0 = first block of a job.
 * Alignment (the jobs are a DEVICE table: the entry point cannot check it): an f32 master is read as float4, so w must be 16-byte
 * aligned; a bf16 source is read four elements at a time, so w must be 8-byte aligned; wf and wb are written 16 bytes per lane and
 * must be 16-byte aligned.  PackPlan keeps to this: packed operands start at multiples of 8 elements of a 256-byte aligned buffer, and
 * an f32 master below 16-byte alignment is not fragment-packed. */
typedef struct SedtFragJob {
  const float* w; /* f32 master [N][K]; with src_bf16 a bf16 matrix [N][K] (a packed convolution operand of sedt_multi_pack) */
  void* wf;       /* fragment-major W, bf16, or null */
  void* wb;       /* fragment-major W^T, bf16, or null */
  int32_t N, K;
  int32_t blk0, src_bf16;
} SedtFragJob;
int sedt_pack_frag(const SedtFragJob* jobs, int njobs, int nblocks, void* stream);
/* The pre-norm encoder layer (sedt/transformer.py:192-204; nn.MultiheadAttention arithmetic as in sedt_attention_fwd) in TWO launches:
 *   sedt_encoder_qkv_fwd:      xn = LayerNorm1(x); q | k = (xn + pos) Wqk^T + b; v = xn Wv^T + b
 *   sedt_encoder_attn_ffn_fwd: ctx = dropout(softmax(q k^T / sqrt(32) + key padding)) v over the clip's S keys;
 *                              x1 = x + dropout(ctx Wo^T + bo); x1n = LayerNorm2(x1);
 *                              x2 = x1 + dropout(dropout(relu(x1n W1^T + b1)) W2^T + b2)
 * x, pos, x2 [B*S][256] bf16 contiguous; qk [B*S][512], v [B*S][256] bf16; weights fragment-major (sedt_pack_frag), biases and
 * LayerNorm parameters f32; kpm [B][S] (1 = padding) or null.  Training by-products - what sedt_layernorm_bwd, sedt_attention_bwd and
 * the weight-gradient GEMMs read; all or none (null: a no-grad forward): xn, xnp [B*S][256], mean, rstd [B*S]; ctx, x1, x1n
 * [B*S][256], lse [B][8][S], mean2, rstd2 [B*S], h [B*S][FF] (the dropped ReLU output).  Dropout decisions are the counter hashes of
 * the unfused chain: attention ((b*8 + h)*S + q)*S + k under seed_attn, out-proj row*256 + col under seed_o, hidden row*FF + col
 * under seed_h, FFN output row*256 + col under seed_f (each + *seed_ptr).  Envelope (sedt_encoder_slab_ok): bf16, d_model 256,
 * 8 heads, S <= 128, FF a multiple of 512. */
/* (SedtPrefetch: declared with sedt_multi_wgrad_reduce above) */
int sedt_encoder_slab_ok(int D, int H, int S, int FF, int dtype);
/* The input-gradient chain of the same layer, two launches around sedt_attention_bwd (weights as fragment-major W^T, the `wb` of
 * sedt_pack_frag):
 *   sedt_encoder_ffn_bwd:  g2 = dropout'(gx2); gh = (g2 W2) [h > 0] / (1 - p); g_x1n = gh W1; gx1 = LayerNorm2'(g_x1n) + gx2;
 *                          g1 = dropout'(gx1); gctx = g1 Wo          (g2 may be null when drop_p == 0: it equals gx2; g1 likewise)
 *   sedt_encoder_qkv_bwd:  gx = LayerNorm1'(dq|dk Wqk + dv Wv) + gx1
 * g2, gh, g1 are the left operands of the weight-gradient GEMMs of linear2, linear1, out_proj; ln_part [slabs][512] = per-slab
 * sums of (dy * xhat | dy) whose column sums are the LayerNorm gamma / beta gradients (slabs = B * ceil(S / 32)). */

/* An identity Bottleneck of ResNet layer1 / layer2 (torchvision v1.5 block behind sedt/backbone.py:97-113; cin -> planes -> planes -> cin,
 * stride 1, no downsample branch) in ONE launch, and its input-gradient chain in one more (csrc/bneck.hip; a workgroup per strip of 8
 * image rows, the planes-channel intermediates never leave the CU).  M = B*H*W pixels, NHWC.
 *   sedt_bneck_fwd: a = relu(s1 (x W1^T) + b1); b = relu(s2 conv3x3(a, W2) + b2); y = relu(s3 (b W3^T) + b3 + x)
 *     x, y [M][cin] bf16; w1/w2/w3_frag = sedt_pack_frag (src_bf16) of the forward operands of sedt_multi_pack ([Cout][taps][Cin]);
 *     s*, b* the folded FrozenBN scale / bias.  Training by-products, each group may be null: abits_out, bbits_out [M][planes/8] = sign
 *     bits of a, b (bit c % 8 of byte c / 8) - all sedt_bneck_bwd needs of them, 1/16 of the bytes; a_out, b_out [M][planes] - what the
 *     weight-gradient GEMMs of a trainable block read; bits_out [M][cin/8] = sign bits of y.
 *   sedt_bneck_bwd: gb = (gy W3s) [b > 0]; ga = conv3x3^T(gb, W2s) [a > 0]; gx = (ga W1s + gy) [x > 0]
 *     w*t_frag = sedt_pack_frag (src_bf16) of the dgrad operands of sedt_multi_pack ([Cin][taps][Cout], BN scale folded in); gy is the
 *     gradient w.r.t. y already masked by [y > 0]; abits / bbits from the forward; xbits = sign bits of the block input, or null (no mask).
 *     gb_out, ga_out [M][planes] (both or none): the two intermediate gradients, left operands of the weight-gradient GEMMs of a
 *     trainable block (layer2; layer1 is frozen in the reference, backbone.py:60-62, and needs neither).  gx == null: the chain stops
 *     at ga (ga_out required, w1t_frag / xbits ignored) - for a block whose first convolution has another shape (layer1's block 0: the
 *     caller finishes with its own two input-gradient GEMMs).
 * Envelope (sedt_bneck_ok): bf16, stride 1, dilation 1, no downsample, and (cin, planes, W) = (256, 64, 16) or (512, 128, 8). */
int sedt_bneck_ok(int cin, int planes, int W, int stride, int dil, int has_downsample, int dtype);
int sedt_bneck_fwd(const void* x, void* y, const void* w1_frag, const void* w2_frag, const void* w3_frag, const float* s1, const float* b1,
                   const float* s2, const float* b2, const float* s3, const float* b3, void* a_out, void* b_out, uint8_t* abits_out,
                   uint8_t* bbits_out, uint8_t* bits_out, int cin, int planes, int W, int B, int H, void* stream);
int sedt_bneck_bwd(const void* gy, void* gx, const void* w3t_frag, const void* w2t_frag, const void* w1t_frag, const uint8_t* abits,
                   const uint8_t* bbits, const uint8_t* xbits, void* gb_out, void* ga_out, int cin, int planes, int W, int B, int H,
                   void* stream);

/* The same pair for an identity Bottleneck of layer3 (1024 -> 256 -> 256 -> 1024 on a map 4 columns wide; csrc/bneck3.hip): one workgroup
 * per strip of 8 rows x 4 columns = 32 pixels, every workgroup streams all 2.2 MB of the block's weights from L2 while its activations
 * stay in LDS - a ~25 us floor set by the L2 -> CU stream, which beats the three per-op launches only while the strips cover the chip
 * about once: sedt_bneck3_ok additionally wants 192 <= B * ceil(H / 8) <= 512.  Arguments as for sedt_bneck_fwd / sedt_bneck_bwd (cin,
 * planes, W implied); abits / bbits [M][32], bits [M][128]. */
int sedt_bneck3_ok(int cin, int planes, int W, int stride, int dil, int has_downsample, int B, int H, int dtype);
int sedt_bneck3_fwd(const void* x, void* y, const void* w1_frag, const void* w2_frag, const void* w3_frag, const float* s1, const float* b1,
                    const float* s2, const float* b2, const float* s3, const float* b3, void* a_out, void* b_out, uint8_t* abits_out,
                    uint8_t* bbits_out, uint8_t* bits_out, int B, int H, const SedtPrefetch* pf, void* stream);
int sedt_bneck3_bwd(const void* gy, void* gx, const void* w3t_frag, const void* w2t_frag, const void* w1t_frag, const uint8_t* abits,
                    const uint8_t* bbits, const uint8_t* xbits, void* gb_out, void* ga_out, int B, int H, const SedtPrefetch* pf,
                    void* stream);

/* The first Bottleneck of layer1 (64 -> 64 -> 64 -> 256, 1x1 projection 64 -> 256 on the skip path, stride 1, map 16 columns wide) in ONE
 * forward launch (csrc/bneck.hip: bneck0_fwd_kernel): a = relu(s1 (x W1^T) + b1); b = relu(s2 conv3x3(a, W2) + b2);
 * y = relu(s3 (b W3^T) + b3 + bf16(sd (x Wd^T) + bd)).  x [M][64], y [M][256] bf16 NHWC (M = B*H*16); w*_frag as for sedt_bneck_fwd (wd = the
 * projection); training by-products a_out / b_out [M][64], abits_out / bbits_out [M][8] (their sign bits; each pair both or none) and
 * bits_out [M][32] = sign bits of y, each may be null.  The block's backward: sedt_bneck_bwd with gx == null (gy -> gb -> ga in one
 * launch), then the two input-gradient GEMMs of conv1 and the projection.  Envelope (sedt_bneck0_ok): bf16, cin 64, planes 64, W 16,
 * stride 1, dilation 1, WITH the downsample branch. */
int sedt_bneck0_ok(int cin, int planes, int W, int stride, int dil, int has_downsample, int dtype);
int sedt_bneck0_fwd(const void* x, void* y, const void* w1_frag, const void* w2_frag, const void* w3_frag, const void* wd_frag, const float* s1,
                    const float* b1, const float* s2, const float* b2, const float* s3, const float* b3, const float* sd, const float* bd,
                    void* a_out, void* b_out, uint8_t* abits_out, uint8_t* bbits_out, uint8_t* bits_out, int B, int H, void* stream);

/* The first Bottleneck of layer2 (256 -> 128 at the input resolution, 3x3 stride 2, 128 -> 512, stride-2 1x1 projection 256 -> 512 on the
 * skip path; input map 16 columns wide, output 8) in ONE forward launch (csrc/bneck.hip: bneck2_fwd_kernel).  x [B*H*16][256], y
 * [B*H2*8][512] with H2 = (H - 1) / 2 + 1; w*_frag / s* / b* as for sedt_bneck0_fwd.  Training by-products, each may be null: a_out
 * [B*H*16][128] and b_out [B*H2*8][128] (both or none; what the per-op backward of the block reads), bits_out [B*H2*8][64] = sign bits
 * of y.  Envelope (sedt_bneck2_ok): bf16, cin 256, planes 128, W 16, stride 2, dilation 1, WITH the downsample branch. */
int sedt_bneck2_ok(int cin, int planes, int W, int stride, int dil, int has_downsample, int dtype);
int sedt_bneck2_fwd(const void* x, void* y, const void* w1_frag, const void* w2_frag, const void* w3_frag, const void* wd_frag, const float* s1,
                    const float* b1, const float* s2, const float* b2, const float* s3, const float* b3, const float* sd, const float* bd,
                    void* a_out, void* b_out, uint8_t* bits_out, int B, int H, void* stream);

/* The prediction heads on the stacked decoder output hs [L*B*Qp][256] bf16 (sedt/sedt.py:88-95, 398-409) in ONE launch each way
 * (csrc/heads_slab.hip; a workgroup per 32 rows): class logits cls [rows][C1] = hs wc^T + bc, boxes [rows][2] = sigmoid(W3 relu(W2
 * relu(W1 hs + b1) + b2) + b3), audio tags at [B][CA] = sigmoid(wa hs + ba) on query 0 of the last layer (CA = 0: no such head).
 * wc, w3, wa: the f32 master weights; W1, W2 fragment-major (sedt_pack_frag).  h1 / h2 [rows][256] bf16: the hidden activations, kept
 * for the backward (both or none).  sedt_heads_bwd: from the gradients of the three outputs (g_at may be null) the input gradient dhs,
 * the hidden-layer gradients g_h1 / g_h2 (left operands of the W1 / W2 weight-gradient GEMMs) and part [slabs][NG * 257], NG = C1 +
 * CA + 2: per 32-row slab the [NG][256] weight-gradient sums of the head outputs (class rows, then audio-tag rows, then the 2 box
 * rows) followed by their NG bias sums; the sums over the slabs are the gradients of wc | wa | w3 and bc | ba | b3.  Envelope: bf16, d = 256, C1, CA <= 16. */
int sedt_heads_slab_ok(int D, int C1, int CA, int dtype);
int sedt_heads_fwd(const void* x, const float* wc, const float* bc, const void* w1_frag, const float* b1, const void* w2_frag,
                   const float* b2, const float* w3, const float* b3, const float* wa, const float* ba, float* cls, float* box, float* at,
                   void* h1, void* h2, int L, int B, int Qp, int C1, int CA, void* stream);
size_t sedt_heads_bwd_part_floats(int L, int B, int Qp, int C1, int CA);
int sedt_heads_bwd(const void* x, const void* h1, const void* h2, const float* box, const float* at, const float* g_cls,
                   const float* g_box, const float* g_at, const float* wc, const float* w3, const float* wa, const void* w2t_frag,
                   const void* w1t_frag, void* dhs, void* g_h1, void* g_h2, float* part, int L, int B, int Qp, int C1, int CA, void* stream);

int sedt_encoder_ffn_bwd(const void* gx2, const void* h, const void* x1, const float* mean2, const float* rstd2,
                         const float* gamma2, const void* w2t_frag, const void* w1t_frag, const void* wot_frag, void* g2, void* gh,
                         void* gx1, void* g1, void* gctx, float* ln_part, int B, int S, int FF, float drop_p, uint32_t seed_f,
                         uint32_t seed_o, const uint32_t* seed_ptr, void* stream);
int sedt_encoder_qkv_bwd(const void* dqk, const void* dv, const void* x, const float* mean1, const float* rstd1,
                         const float* gamma1, const void* gx1, const void* wint_frag, void* gx, float* ln_part, int B, int S,
                         void* stream);
int sedt_encoder_qkv_fwd(const void* x, const void* pos, const float* gamma, const float* beta, const void* w_in_frag,
                         const float* b_in, void* qk, void* v, void* xn, void* xnp, float* mean, float* rstd, int B, int S,
                         const SedtPrefetch* pf, void* stream);
int sedt_encoder_attn_ffn_fwd(const void* x, const void* qk, const void* v, const uint8_t* kpm, const void* w_o_frag,
                              const float* b_o, const float* gamma2, const float* beta2, const void* w1_frag, const float* b1,
                              const void* w2_frag, const float* b2, void* x2, void* ctx, float* lse, void* x1, float* mean2,
                              float* rstd2, void* x1n, void* h, int B, int S, int FF, float drop_p, uint32_t seed_attn,
                              uint32_t seed_o, uint32_t seed_h, uint32_t seed_f, const uint32_t* seed_ptr, void* stream);

/* chunk.p[i] = chunk.g[i] for every chunk: packs all gradient tensors into one flat buffer (one launch) ahead of the RCCL
 * all-reduce of the data-parallel step.  mode bit 0: chunk.p[i] += chunk.g[i] instead (gradient accumulation over micro-batches,
 * engine.py:76, 174); bit 1: the flat buffer is bf16 (chunk.p addresses 2-byte elements; half the all-reduce bytes). */
int sedt_multi_gather(const SedtChunk* table, int nchunks, int mode, void* stream);
/* mean-teacher update of every tensor in one launch (utilities/utils.py:62-67, EMA.update):
 * chunk.m[i] = (1 - decay) * chunk.p[i] + decay * chunk.m[i]   (p = student parameter, m = shadow)
 * Non-finite guard (the reference aborts BEFORE the backward when the loss is NaN / inf: engine.py:70-73, 167-169; a captured
 * step cannot stop itself, its host only polls a flag now and then): `guard` is an optional device int32 word, the same one
 * SedtCriterion.nonfinite / sedt_feature_loss raise.  sedt_multi_sumsq also raises it when the squared gradient norm is not
 * finite and - step_ptr given - advances the device-side Adam step count unless the guard is up; sedt_multi_adamw and
 * sedt_multi_ema return without touching parameters, moments or the shadow weights while it is up.  So a bad batch leaves the
 * whole training state (student, optimizer, teacher) at its last good value until the host sees the flag and raises. */
int sedt_multi_ema(const SedtChunk* table, int nchunks, float decay, const int32_t* guard /* or null */, void* stream);
int sedt_multi_sumsq(const SedtChunk* table, int nchunks, float* partial, float* sumsq, int32_t* step_ptr /* or null: += 1 */,
                     int32_t* guard /* or null */, uint32_t* seed_word /* or null: the device dropout-seed word, += 1 */, void* stream);
int sedt_multi_adamw(const SedtChunk* table, int nchunks, const float* sumsq, float max_norm, float beta1, float beta2,
                     float eps, const int32_t* step_ptr /* device: 1-based step count */, const int32_t* guard /* or null */,
                     void* stream);

/* ------------------------------------------------------------------ device half of SetCriterion (sedt/sedt.py:161-283)
 * After the host matching the targets are dense: for dense layer d (0 = final decoder layer, d>=1 = aux layer d-1),
 * strong clip b < ns, query q: tc = target class (as f32), coef = CE weight multiplier, wbox = box-loss weight (0 =
 * unmatched), tbox = target (centre, length).  logits [L][B][Q][C+1] / boxes [L][B][Q][2] are the model's stacked head
 * outputs; layer_of[d] is the slice that dense layer d reads.  One launch writes
 *   out[4d+0..3] = loss_ce, loss_bbox, loss_giou, cardinality_error of dense layer d (unweighted, as the reference logs)
 *   out[4L] = class-error hits, out[4L+1] = matched count, out[4L+2] = loss_weak,
 *   out[4L+3] = weighted total (sum_k weight_k * loss_k), out[4L+4] = class_error, out[4L+5] = loss_weak_p
 * and the UNWEIGHTED per-term gradients: dlogits = d loss_ce_d / d logits, dboxes = d loss_bbox_d / d boxes, dboxes2 =
 * d loss_giou_d / d boxes (each layer slice holds the gradient of its own layer's loss), dat = d loss_weak / d at.
 * at / gt_weak / dat may be null together (model without audio-tag head).
 * --pooling models (sedt.py:96-119, sedt_pool_at below) add at_p [Bp][C], the pooled clip-level probabilities: loss_weak_p =
 * BCE(at_p[rows], gt_weak[rows]) (sedt.py:182-185) over the weak clips rows = [ns, n_lab), or - wp_all != 0, the reference's
 * weak_mask None - over all labelled clips [0, n_lab); an empty row range gives NaN, as the reference's mean over nothing.
 * dat_p [Bp][C] = d loss_weak_p / d at_p.  at_p / dat_p may be null together; at_p needs at (the reference forms gt there).
 * sedt_set_criterion_bwd combines them with the gradient g[4L+6] that reached `out`:
 *   glogits = (g[4d] + g[4L+3] w_ce[d]) dlogits,  gboxes = (g[4d+1] + g[4L+3] w_bbox[d]) dboxes + (g[4d+2] + ...) dboxes2,
 *   gat = (g[4L+2] + g[4L+3] w_weak) dat,  gat_p = (g[4L+5] + g[4L+3] w_weak_p) dat_p. */
#define SEDT_CRIT_MAXL 8
#define SEDT_CRIT_MAXOUT (4 * SEDT_CRIT_MAXL + 6)
#define SEDT_CRIT_MAXCARD 8192 /* limit on L * B */
typedef struct SedtCriterion {
  const float* logits;
  const float* boxes;
  const float* at;       /* [Bat][C] probabilities, rows < n_lab are labelled */
  const float* tc;       /* [L][ns][Q] */
  const float* coef;     /* [L][ns][Q] */
  const float* wbox;     /* [L][ns][Q] */
  const float* tbox;     /* [L][ns][Q][2] */
  const float* gt_weak;  /* [n_lab][C] */
  const float* tgt_len;  /* [B] */
  const float* num_boxes;    /* [1], or null: computed as sum(wbox[0]) */
  const float* empty_weight; /* [C+1] */
  float* dlogits;
  float* dboxes;
  float* dboxes2;
  float* dat;
  float* out; /* [4L+6] */
  int32_t L, B, ns, Q, C, n_lab, Bat;
  int32_t layer_of[SEDT_CRIT_MAXL];
  float w_ce[SEDT_CRIT_MAXL], w_bbox[SEDT_CRIT_MAXL], w_giou[SEDT_CRIT_MAXL];
  float w_weak;
  /* focal-loss variant (sedt/sedt.py:176, 211-218, 412-433; train_ss_sedt.py --focal_loss): fl != 0 replaces the weighted
   * cross-entropy by sigmoid_focal_loss over the C+1 logits (pos_weight = empty_weight) and the audio-tag BCE by
   * weak_focal_loss (sum over classes, mean over clips); alpha_fl < 0 disables the alpha_t factor (config.py:71-72). */
  int32_t fl;
  float alpha_fl, gamma_fl;
  /* optional device word: set to 1 (never cleared here) when the weighted total is not finite - the reference aborts on
   * such a loss (engine.py:70-73, 167-169); a graphed step polls this word instead of synchronising every step */
  int32_t* nonfinite;
  /* optional device words {ns, n_lab} that override the two fields above as the NUMBER of strong / labelled clips of this batch
   * (utilities/mixup.py:13-127 returns a new strong | weak split for every batch); ns / n_lab then are the capacities = the
   * strides of the dense tables.  Lets a captured step take batches of any split. */
  const int32_t* split;
  /* layout of logits / boxes (and of the gradients sedt_set_criterion_bwd returns): [L][B][Qs] rows, of which the Q queries
   * q0 .. q0 + Q - 1 take part in the losses (dec_at models run their heads over the audio-tag query 0 too: Qs = Q + 1, q0 = 1;
   * otherwise Qs = Q, q0 = 0).  The per-term gradient buffers dlogits / dboxes / dboxes2 stay compact ([L][B][Q]). */
  int32_t Qs, q0;
  float* total; /* optional: receives out[4L+3] as a separate scalar (its own autograd output: no select/backward-of-select) */
  const float* at_p; /* [Bp][C] pooled probabilities (--pooling), or null */
  float* dat_p;      /* [Bp][C] */
  float w_weak_p;
  int32_t wp_all, Bp;
} SedtCriterion;
size_t sedt_set_criterion_scratch(int L, int B, int Q); /* bytes of `scratch`: per-row loss terms, summed per layer in a fixed order */
int sedt_set_criterion(const SedtCriterion* args, float* scratch, void* stream);
/* g: gradient that reached out[4L+6] (or null), gtotal: gradient that reached the separate total scalar (or null) */
int sedt_set_criterion_bwd(const SedtCriterion* args, const float* g, const float* gtotal, float* glogits, float* gboxes,
                           float* gat, float* gat_p /* or null */, void* stream);

/* ------------------------------------------------------------------ --pooling variants of SEDT (sedt/sedt.py:47-61, 96-119)
 * at_p[b][c], c < C: the clip-level probability pooled over the Q event queries' class probabilities
 * y[b][q][c] = softmax(logits[b][q0 + q])[c] of the FINAL decoder layer (replaces nn.AdaptiveMaxPool2d / AdaptiveAvgPool2d((1, None)),
 * the attn_pooling closure and the weighted sum of sedt.py:98-100):
 *   SEDT_POOL_MAX  max_q y        SEDT_POOL_AVG  mean_q y
 *   SEDT_POOL_ATTN s = clamp(softmax_c(attn[b][q]), 1e-7, 1); sum_q s y / sum_q s   (attn = attn_dense_softmax(hs[-1]) [B][Q][C])
 *   SEDT_POOL_WSUM clip(sum_q y * boxes[b][q0 + q][1], 0, 1)                        (the predicted event length as weight)
 * logits [B][Qs][C+1] / boxes [B][Qs][2] are the head outputs over ALL Qs query rows (dec_at models: q0 = 1 skips the
 * audio-tag query).  sedt_pool_at_bwd: g [B][C] -> glogits [B][Qs][C+1] (zero rows outside the window), gboxes [B][Qs][2]
 * (WSUM; may be null otherwise), gattn [B][Q][C] (ATTN; may be null otherwise); max sends the gradient to the first maximal
 * query, clamp / clip pass it where the value lies inside the closed interval (torch semantics).  Q * (C+1) <= 4096. */
enum { SEDT_POOL_MAX = 0, SEDT_POOL_AVG = 1, SEDT_POOL_ATTN = 2, SEDT_POOL_WSUM = 3 };
typedef struct SedtPoolAt {
  const float* logits;
  const float* boxes; /* WSUM, else may be null */
  const float* attn;  /* ATTN, else may be null */
  int32_t B, Qs, q0, Q, C, mode;
} SedtPoolAt;
int sedt_pool_at(const SedtPoolAt* args, float* at_p /* [B][C] */, void* stream);
int sedt_pool_at_bwd(const SedtPoolAt* args, const float* g, float* glogits, float* gboxes, float* gattn, void* stream);

/* ------------------------------------------------------------------ SP-SEDT feature-reconstruction loss (sedt/sedt.py:263-283)
 * For dense layer d, strong clip b, query q matched to patch tidx (wbox > 0):
 *   row = sum_f (normalize(pred[layer_of[d]][b][q])[f] - normalize(gt[b*P + tidx])[f])^2,   normalize = x / max(|x|_2, 1e-12)
 *   out[d] = sum over matched rows / num_boxes.  dpred receives d out[d] / d pred (unweighted; zero rows where unmatched).
 * pred / dpred [L][B][Q][F] f32, gt [B*P][F] f32 (treated as a constant: the SP-SEDT backbone is frozen,
 * train_spsedt.py:50), wbox / tidx [L][ns][Q] as written by sedt_match_targets, num_boxes [1] device scalar.
 * rowloss [L*ns*Q] scratch.  Deterministic (fixed summation order).  sedt_scale_layers: x[l][...] *= g[d] + gtot[0]*w[d] with d = idx[l] (idx = inverse of layer_of: dpred is in the model's
 * layer order, the loss vector in dense order). */
int sedt_feature_loss(const float* pred, const float* gt, const float* wbox, const float* tidx, const float* num_boxes,
                      const int32_t* layer_of /* host [L] */, const float* w /* device [L] or null */, int L, int B, int ns,
                      int Q, int P, int F, float* rowloss, float* out /* [L+1]: out[L] = sum_d w[d] out[d] */, float* dpred,
                      int32_t* nonfinite /* or null: set to 1 when out[L] is NaN / inf (see SedtCriterion.nonfinite) */,
                      const float* base /* or null */, float* total_out /* or null: *total_out = out[L] + base[0] - the step's weighted total
                      with SetCriterion's (sedt_set_criterion's `total`) folded in, so the sum costs no launch of its own */, void* stream);
int sedt_scale_layers(float* x, const float* g, const float* gtot, const float* w, const int32_t* idx /* host [L] or null */,
                      int L, int64_t per_layer, void* stream);
/* out[0] = sum_i x[i] (one workgroup, fixed order): num_boxes = sum of the final layer's box weights (sedt.py:322-324) */
int sedt_sum_f32(const float* x, int n, float* out, void* stream);

/* ------------------------------------------------------------------ device-side matching (sedt/matcher.py:41-133)
 * The Hungarian assignment of every (decoder layer, strong clip) and the dense targets sedt_set_criterion reads, in one
 * launch and without leaving the device (one wave per problem; Q <= 63 queries, <= 63 targets per clip).
 * Targets arrive concatenated over the batch: lab_cat[lab_off[b] .. lab_off[b+1]) = labels of clip b (all B clips; for a
 * strong clip the first n_b labels belong to its n_b boxes), box_cat[box_off[b] .. box_off[b+1]) = (centre, length) of
 * the events of strong clip b < ns, ratio_cat (optional) aligned with lab_cat.  Cost = w_bbox*L1 + w_class*cost_class
 * - w_giou*GIoU with cost_class = -softmax(logits)[class] (fl == 0) or the focal matching cost of matcher.py:73-78
 * (fl != 0); same optimum and tie-breaking as sedt_hungarian_batch.
 * Coefficients (matcher.py:124-132): normalize != 0: 1 / (number of queries matched to the same target); else with
 * ratio_cat: the k-th matched query of a clip (ascending query index) takes ratio[k] - POSITIONAL, as the reference
 * assigns them; else 1.
 * fine_tune != 0 (matcher.py:99-121; dense layer 0 only, aux layers keep the plain assignment as sedt.py:340 does): with
 * the localisation cost w_bbox*L1 - w_giou*GIoU, a Hungarian pair survives only if the query's closest target is nearer
 * than epsilon; every other query whose closest target is nearer than epsilon is matched to that target unless
 * u > alpha * n_gt / Q, u = ft_rand[b*Q + k] for the k-th such query of clip b (ascending query index; the reference
 * draws torch.rand in that order) or, when ft_rand is null, a counter hash of (ft_seed + *seed_ptr, b, k).
 * Outputs: tc/coef/wbox/tidx [L][ns][Q], tbox [L][ns][Q][2], tgt_len [B], gt_weak [n_lab][C] (may be null),
 * assign [L][ns][Q] int32 (may be null): index of the matched target within its clip or -1.
 * max_targets: capacity per clip the caller guarantees (LDS sizing; box_off differences must not exceed it). */
typedef struct SedtMatch {
  const float* logits;   /* [L][B][Q][C+1] */
  const float* boxes;    /* [L][B][Q][2] */
  const int64_t* lab_cat;
  const int32_t* lab_off; /* [B+1] */
  const float* box_cat;
  const int32_t* box_off; /* [ns+1] */
  const float* ratio_cat; /* or null */
  float* tc;
  float* coef;
  float* wbox;
  float* tbox;
  float* tidx;
  float* tgt_len;
  float* gt_weak;
  int32_t* assign;
  int32_t L, B, ns, Q, C, n_lab, max_targets;
  int32_t layer_of[SEDT_CRIT_MAXL];
  float w_class, w_bbox, w_giou;
  int32_t fl, fine_tune, normalize;
  float alpha_fl, gamma_fl, epsilon, alpha;
  const float* ft_rand;     /* [ns][Q] or null */
  uint32_t ft_seed;
  const uint32_t* seed_ptr; /* or null */
  const int32_t* split;     /* or null: device {ns, n_lab} of this batch, see SedtCriterion.split (box_off then has ns + 1
                               entries for the capacity ns; clips >= split[0] get "no target" rows) */
  int32_t Qs, q0;           /* logits / boxes rows are [L][B][Qs]; queries q0 .. q0 + Q - 1 are matched (see SedtCriterion) */
} SedtMatch;
int sedt_match_targets(const SedtMatch* args, void* stream);

/* ------------------------------------------------------------------ PostProcess + pseudo labels on the device
 * sedt_postprocess (sedt/sedt.py:355-396): softmax over the C+1 logits of every query; optional fusion with clip-level
 * tags (tags [B][C] as f32 0/1, at_m 1/2/3 exactly as the reference: at_m 2/3 lift the best query of every class to
 * `threshold`, at_m 1/2 multiply the class scores by the tags); scores [B][Q] = max class score, labels [B][Q] (int64) =
 * its class (first maximum), boxes_out [B][Q][2] = (onset, offset) * sizes[b], or the (centre, length) input when is_semi.
 *
 * sedt_pseudo_labels (engine.py:300-348, get_pseudo_labels): tags = at >= thr[class]; PostProcess(at_m = 1, is_semi); an
 * event survives when score >= thr[label] and length > min_len; per clip the survivors are ordered by descending score
 * (ties: lower query first) and, with del_overlap, an event is dropped when an already kept event of the same class
 * overlaps it in time.  Results are written in the flat layout sedt_match_targets reads: lab_cat / box_cat compacted
 * over the clips in kept order, lab_off / box_off [B+1], counter[C] += kept events per class (int32; pseudo_labels_counter
 * of the reference).  cap = capacity of lab_cat / box_cat in events.  at may be null (no tag gating). */
int sedt_postprocess(const float* logits, const float* boxes, const float* tags, const float* sizes, int B, int Q, int C,
                     int at_m, float threshold, int is_semi, float* scores, int64_t* labels, float* boxes_out, void* stream);
int sedt_pseudo_labels(const float* logits, const float* boxes, const float* at, const float* thr, float min_len, int B,
                       int Q, int C, int del_overlap, int64_t* lab_cat, float* box_cat, int32_t* lab_off, int32_t* box_off,
                       int32_t* counter, int cap, void* stream);

/* ------------------------------------------------------------------ validation scores on the device
 * sedt_event_metrics_update (engine.py:199-297 with utilities/BoxEncoder.py:179-226 and utilities/metrics.py:43-80, 281-322): one
 * wave per clip of one fusion strategy's PostProcess outputs (scores [B][Q] f32, labels [B][Q] int64, boxes [B][Q][2] f32 seconds).
 * Decode (decode_strong): a query is kept when score >= threshold (del_overlap) or score > threshold (!del_overlap) and
 * offset - onset >= min_duration, both in f32; with del_overlap the kept events of a class are ordered by onset (ties: lower query
 * first) and swept once: an event starting before the end of the last one still standing replaces it when its score is strictly
 * higher, else is dropped.  Onsets / offsets are then clipped to [0, max_len] and compared in float64 with the clip's reference
 * events: a hit is same class, |on_r - on_e| <= t_collar and |off_r - off_e| <= max(t_collar, pct * (off_r - on_r)).  Per class,
 * tp = the maximum-cardinality matching of the hits (optimal != 0, sed_eval's 'optimal') or sed_eval's greedy pass (references in
 * table order, estimates in decoded order).
 * Reference table (uploaded once per validation set): clip k owns events [ref_off[k], ref_off[k+1]) of ref_cls (int32 class),
 * ref_on / ref_end (float64 seconds); ref_present [n_clips] int32 (null = all 1): 0 for a clip that has no row in the reference;
 * max_ref = the largest event count of a clip (<= 64).  clip_idx [B] int32: the batch's clips in the table, -1 (or >= n_clips) for a
 * clip outside it (treated like ref_present 0).
 * Counters (int64, accumulated with integer atomics; zero them per validation set):
 *   ev_counts  [n_fusion][C][3] += {tp, n_ref, n_sys} at row `fusion`, from clips in the reference only (metrics.py:58);
 *   tag_counts [n_fusion + 1][C][3] += {tp, fp, fn} of "class among the decoded events" vs "class among the reference events" at
 *   row `fusion`, from every clip (the outer merge of metrics.py:289); with at_tags [B][C] (int64 0/1, may be null) the same counts
 *   of the audio-tag head at row n_fusion.  Q <= 64, C <= 63. */
int sedt_event_metrics_update(const float* scores, const int64_t* labels, const float* boxes, const int64_t* at_tags,
                              const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off, const int32_t* ref_cls,
                              const double* ref_on,
                              const double* ref_end, int n_clips, int max_ref, int B, int Q, int C, int n_fusion, int fusion,
                              float threshold, float min_duration, double max_len, double t_collar, double pct, int del_overlap,
                              int optimal, int64_t* ev_counts, int64_t* tag_counts, void* stream);
/* sedt_event_segment_metrics_update (utilities/metrics.py:83-116, 147-157: sed_eval SegmentBasedMetrics): the same launch, the same
 * arguments and the same ev / tag counts, plus the segment-based counts of the clips in the reference at resolution time_resolution
 * (seconds, > 0).  After the decode and the hit graph, the survivors (clipped to [0, max_len], in float64) and the clip's reference
 * events are rasterised into per-class bit rows in LDS: event (c, on, off) sets segments floor(on / r) <= k < ceil(off / r), both
 * quotients float64 divisions (sed_eval's event roll), over n_seg_words words of 64 segments (1 .. 16: at most 1024 segments; the
 * host bounds ceil(max(max_len, largest reference offset) / r) by n_seg_words * 64 and keeps reference times >= 0).
 *   seg_counts [n_fusion][C][3] += {tp, n_ref, n_sys}: class-wise segments active in both / in the reference / in the estimates;
 *   sdi_counts [n_fusion][3]    += {S, D, I}: per segment over the classes, S = min(Nref, Nsys) - Ntp, D = max(0, Nref - Nsys),
 *   I = max(0, Nsys - Nref).  Integer atomics only. */
int sedt_event_segment_metrics_update(const float* scores, const int64_t* labels, const float* boxes, const int64_t* at_tags,
                                      const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off,
                                      const int32_t* ref_cls, const double* ref_on, const double* ref_end, int n_clips, int max_ref,
                                      int B, int Q, int C, int n_fusion, int fusion, float threshold, float min_duration,
                                      double max_len, double t_collar, double pct, int del_overlap, int optimal, int64_t* ev_counts,
                                      int64_t* tag_counts, double time_resolution, int n_seg_words, int64_t* seg_counts,
                                      int64_t* sdi_counts, void* stream);

/* sedt_decode_events (engine.py:218-297 with utilities/BoxEncoder.py:179-226): the predictions themselves.  One wave per (clip,
 * threshold) of one fusion strategy's PostProcess outputs (scores [B][Q] f32, labels [B][Q] int64, boxes [B][Q][2] f32 seconds);
 * thresholds [K] f32 is a DEVICE vector read by every launch (a captured graph follows an edited grid), 1 <= K <= 1024.
 * Decode, all in f32: a query is kept when score >= threshold (del_overlap) or score > threshold (!del_overlap), offset - onset >=
 * min_duration and 0 <= label < C.  With del_overlap the classes come in the order of their first kept query (the reference's dict
 * insertion order, fixed before any deletion), the events of a class by onset (ties: lower query first), swept once: an event
 * starting before the end of the last one still standing replaces it when its score is strictly higher, else is dropped.  Without
 * del_overlap: the kept queries in query order.  Onsets / offsets are then clipped to [0, max_len]; max_len must be a value float32
 * represents exactly (refused otherwise), +inf = no clip at all.  An event clipped to zero length stays.
 * out [K][B][1 + 5 Q] 32-bit words: word 0 = the event count n, then Q slots {class int32, onset f32, offset f32, score f32, query
 * int32} in output order; every slot at or past n is written as {-1, 0, 0, 0, -1} by every launch.  Plain stores, no atomics.
 * Q <= 64, C <= 63. */
int sedt_decode_events(const float* scores, const int64_t* labels, const float* boxes, const float* thresholds, int B, int Q, int C,
                       int K, float min_duration, double max_len, int del_overlap, int32_t* out, void* stream);
/* sedt_decode_events_classwise: the same kernel, the same arguments and the same records, with thresholds [K][C] f32 (a DEVICE table
 * read by every launch): operating point k compares a query with thresholds[k][label] - the reference's classwise_threshold
 * (engine.py:300-348 applies one per class to its pseudo labels; utilities/metrics.py get_f_measure_by_class takes thresholds_ per
 * class) applied to decode_strong.  The label is tested against 0 <= label < C BEFORE the lookup: a query with any other label (-1, C,
 * 2^40) is dropped and reads nothing.  Decode is class by class, so the events of class c at operating point k are those
 * sedt_decode_events gives at the uniform threshold thresholds[k][c]; a table whose rows are constant gives records bit-identical
 * to sedt_decode_events at that [K] grid. */
int sedt_decode_events_classwise(const float* scores, const int64_t* labels, const float* boxes, const float* thresholds, int B,
                                 int Q, int C, int K, float min_duration, double max_len, int del_overlap, int32_t* out, void* stream);

/* sedt_event_sweep_update (utilities/metrics.py:43-80, 281-322 at every operating point): the event-based and clip-level counts of
 * sedt_event_metrics_update for every threshold of the decoder's grid in one launch, from the buffer sedt_decode_events(_classwise)
 * just wrote.  One wave per (clip, threshold); the decode is not repeated and the records' times, already clipped to [0, max_len], are
 * not clipped again.
 * records [K][B][1 + 5 Q]: sedt_decode_events' `out`.  A record whose count is outside 0 .. Q is skipped whole; a live slot whose class
 * is outside 0 .. C - 1 is not counted; neither is ever used as an index.
 * Reference table: sedt_event_metrics_update's (ref_present, ref_off, ref_cls, ref_on, ref_end, n_clips, max_ref <= 64, clip_idx with
 * the same rule: -1, an index >= n_clips or ref_present 0 = a clip outside the table).
 * Per clip and threshold, exactly sedt_event_metrics_update's counting on the record's events: a hit is an estimate of the reference
 * event's class with |on_r - on_e| <= t_collar and |off_r - off_e| <= max(t_collar, pct * (off_r - on_r)), in float64 on the record's
 * f32 times widened, no contraction; class-wise tp is the size of a maximum-cardinality matching of hits (optimal != 0) or of
 * sed_eval's greedy pass (optimal == 0: references in table order, each takes the first free estimate of its class in record order).
 * Counters (int64, integer atomics only; zero them per validation set):
 *   ev_counts  [n_fusion][K][C][3] += {tp, n_ref, n_sys} at row `fusion`, from clips in the table only;
 *   tag_counts [n_fusion][K][C][3] += {tp, fp, fn} of "class among the record's events" vs "class among the reference events" at row
 *   `fusion`, from every clip: a clip outside the table has no reference events, so its classes count as false positives.
 * At threshold k both equal what sedt_event_metrics_update counts at thresholds[k] on the same PostProcess outputs (decode and
 * matching are class by class: under sedt_decode_events_classwise the counts of class c are those at the uniform threshold
 * thresholds[k][c]).
 * 1 <= Q <= 64, 1 <= C <= 63, 1 <= K <= 1024, max_ref <= 64, B >= 0 (B == 0 launches nothing). */
int sedt_event_sweep_update(const int32_t* records, const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off,
                            const int32_t* ref_cls, const double* ref_on, const double* ref_end, int n_clips, int max_ref, int B, int Q,
                            int C, int K, int n_fusion, int fusion, double t_collar, double pct, int optimal, int64_t* ev_counts,
                            int64_t* tag_counts, void* stream);

/* sedt_psds_update (utilities/metrics.py:120-145, 325-330: psds_eval's PSDSEval restated, utilities/psds.py holds the definition): the
 * per-operating-point confusion counts of the polyphonic sound detection score, from the buffer sedt_decode_events just wrote.  One
 * wave per (clip, threshold); the decode is not repeated.
 * records [K][B][1 + 5 Q]: sedt_decode_events' `out`.  A record whose count is outside 0 .. Q is skipped whole; a live slot whose class
 * is outside 0 .. C - 1 or whose offset - onset is not > 0 is skipped; neither is ever used as an index.
 * Reference table: sedt_event_metrics_update's (ref_present, ref_off, ref_cls, ref_on, ref_end, n_clips, max_ref <= 64, clip_idx with
 * the same rule: -1, an index >= n_clips or ref_present 0 = a clip outside the table, which adds nothing), plus ref_dur [n_clips]
 * float64: the clip's duration D_k in seconds.  A reference event whose class is outside 0 .. C - 1 or whose duration is not > 0 takes
 * part in nothing.  A clip in the table with no events is scored (its detections can only be false positives).
 * Per clip and threshold, float64 on the records' f32 values widened; inter(d, g) = min(off_d, off_g) - max(on_d, on_g) counts only
 * where > 0; every term is a plain division added to a running sum (no contraction), references in table order, detections in record
 * order; comparisons are >=:
 *   DTC   p_d = sum over the references g of d's class of inter(d, g) / dur_d;  d passes when p_d >= dtc;
 *   GTC   v_g = sum over the detections d of g's class that passed of inter(d, g) / dur_g;  v_g >= gtc: counts[c][c] += 1;
 *   CTTC  for every d that failed and every other class c': sum over the references g of c' of inter(d, g) / dur_d >= cttc:
 *         counts[class(d)][c'] += 1;  and (min(off_d, D_k) - max(on_d, 0)) / dur_d >= cttc: counts[class(d)][C] += 1 (false positive).
 * counts [n_fusion][K][C][C + 1] int64, row `fusion` accumulated with integer atomics only (zero them per validation set).
 * 1 <= Q <= 64, 1 <= C <= 63, 1 <= K <= 1024, max_ref <= 64, B >= 0 (B == 0 launches nothing); dtc, gtc, cttc not NaN. */
int sedt_psds_update(const int32_t* records, const int32_t* clip_idx, const int32_t* ref_present, const int32_t* ref_off,
                     const int32_t* ref_cls, const double* ref_on, const double* ref_end, const double* ref_dur, int n_clips,
                     int max_ref, int B, int Q, int C, int K, int n_fusion, int fusion, double dtc, double gtc, double cttc,
                     int64_t* counts, void* stream);

/* sedt_stitch_events (no counterpart in the reference, which scores 10 s dataset clips only; DESIGN.md section 4, "Recordings of any
 * length", holds the definition and tests/recording_ref.py restates it): the event records of the overlapping windows of R recordings
 * merged into one event list per (threshold, recording, class) - an event a window boundary cut in two, or one that two overlapping
 * windows both report, becomes one event.  One wave per (recording, threshold) sweeps the windows in start order with the open merged
 * events in LDS, so a recording may have any number of windows.
 * records [K][W_stride][1 + 5 Q]: sedt_decode_events' words, one row per window (rows W .. W_stride - 1 are not read); win_off [R + 1]
 * int32: recording r owns the windows win_off[r] .. win_off[r + 1] - 1, ascending by start; win_start [W] float64 seconds; rec_dur [R]
 * float64 seconds (finite); merge_gap float64 >= 0; cap >= 1: the events per (threshold, recording, class) that `out` holds.
 * Per threshold k, recording r, class c; float64 on the records' f32 values widened, plain adds and compares, no contraction:
 *   candidates  every live slot s < n_w of every window w of r whose class is c.  A record whose count is outside 0 .. Q is skipped
 *               whole, a slot whose class is outside 0 .. C - 1 or whose score is NaN is skipped; none is ever used as an index.
 *               on = min(t_w + on32, rec_dur[r]), off = min(t_w + off32, rec_dur[r]), min(a, b) = a > b ? b : a; a candidate whose
 *               off - on is not > 0 is dropped.
 *   merging     the candidates in (on, w, s) order, swept: the running event starts as the first; a candidate with on <= cur.off +
 *               merge_gap joins it (cur.off = max(cur.off, off), cur.n += 1, a STRICTLY higher score takes over cur.score, cur.window -
 *               the index inside the recording - and cur.query), any other closes it and becomes the running event.
 * count [K][R][C] int32: the number of merged events; it keeps counting past cap.
 * out [K][R][C][cap][8 words] {onset f64, offset f64, score f32, n_merged int32, window int32, query int32}, ascending by onset; the
 *   slots at or past min(count, cap) are left untouched.  8-byte aligned.
 * status [K][R] int32, 0 or ONE of: 1 win_start of the recording not ascending (or NaN); 2 at some window w the merged events of the
 *   windows before w that are still open (off + merge_gap >= t_w) plus the kept candidates of w exceed the kernel's working set of 640
 *   (inside the envelope below it cannot happen); 4 a kept candidate with on < t_w (a negative onset in a record); 8 win_off[r] ..
 *   win_off[r + 1] is not a range inside 0 .. W.  Checked in the order 8, 1, then window by window 4 before 2; the sweep stops at the
 *   first.  With a status raised the recording's lists are not to be used: count reads 0 for every class.  Nothing is written out of
 *   bounds in any case.
 * Plain stores and integer LDS adds only: bit-reproducible, independent of launch order.
 * 1 <= Q <= 64, 1 <= C <= 63, 1 <= K <= 1024, R >= 0 (R == 0 launches nothing), 0 <= W <= W_stride.  Envelope of status 2: at most 8
 * earlier windows w' with t_w' + window + merge_gap >= t_w for records whose offsets are clipped to the window length. */
int sedt_stitch_events(const int32_t* records, const int32_t* win_off, const double* win_start, const double* rec_dur, int K, int W,
                       int W_stride, int R, int Q, int C, double merge_gap, int cap, int32_t* count, int32_t* out, int32_t* status,
                       void* stream);

/* sedt_stitch_stream (no counterpart in the reference; DESIGN.md section 4, "Live streams", holds the definition and
 * tests/stream_ref.py restates it): the sweep of sedt_stitch_events ONE window per launch for S live streams, the open set of every
 * (threshold, stream) kept in `state` between launches.  Grid (S, K), one wave each; both kernels are built from the same window step
 * (csrc/stitch_sweep.h).  Per stream s:
 *   action[s]     0 skip (the wave returns at once); 1 add this window; 2 flush: everything open is final; 3 add this window, then flush
 *   row[s]        the row of records [K][B][1 + 5 Q] that holds the stream's window
 *   t_w[s], dur[s]  float64: the window's start and the duration its events are clipped against - the win_start[w] and rec_dur[r] of
 *                 sedt_stitch_events
 *   win_index[s]  the window's index inside the stream: the `window` word of its events
 * state: sedt_stitch_stream_state_bytes(K, S) bytes, 8-byte aligned, [K][S] blocks of a header {N, status, windows_seen, pad, last t_w
 *   f64, count[c] from word 6: events of class c emitted so far} of 72 words and the 640 open entries' fields array by array (onset,
 *   offset, provider's onset f64; score f32; n_merged, window, query, slot, class int32).  All zeros is a fresh stream
 *   (sedt_stream_reset, or a memset of the whole state before first use).  Only N entries are read and written; the working set in LDS
 *   and the overflow condition N + kept candidates > 640 are those of sedt_stitch_events.
 * Emission: the final events of a launch are appended to emit [K][S][emit_cap][10 words] {onset f64, offset f64, score f32, n_merged,
 *   window, query, class, pad = 0} at emit_count [K][S] (in/out; it keeps counting past emit_cap and slots at or past the cap are not
 *   touched).  The events a window's step makes final are ordered by (class, onset); with action 3 those of the flush follow those of
 *   the window's own step, again by (class, onset) - within a class the whole launch is in onset order.
 * Defining property: windows w = 0 .. n-1 of a stream fed one per launch with action 1 and a final 2 (or the last with 3) emit, grouped
 *   by class, the count, the six event words, the per-class order and the status sedt_stitch_events gives for the same records with
 *   win_start = t_w and rec_dur = dur.
 * status [K][S] int32, written for every stream whose action is not 0; a raised status is kept in the state and is sticky: from then
 *   on the stream emits nothing (emit_count does not move, the state does not change) and the status is reported again.
 *   1 t_w below the stream's previous t_w, or NaN; 2 working set overflow; 4 a kept candidate has on < t_w; 8 row outside 0 .. B-1.
 * Plain stores and integer LDS adds only, no floating-point atomics, fp contraction off: two identical sequences of launches give
 * identical bytes.  1 <= Q <= 64, 1 <= C <= 63, 1 <= K <= 1024, 1 <= S <= 65535, B >= 1, merge_gap finite and >= 0, emit_cap >= 1.
 * sedt_stream_reset: the headers and status words of the streams with which[s] != 0 (which == NULL: all) read zero afterwards. */
int64_t sedt_stitch_stream_state_bytes(int K, int S);
int sedt_stitch_stream(const int32_t* records, const int32_t* action, const int32_t* row, const double* t_w, const double* dur,
                       const int32_t* win_index, int K, int S, int B, int Q, int C, double merge_gap, int emit_cap, int32_t* state,
                       int64_t state_bytes, int32_t* emit, int32_t* emit_count, int32_t* status, void* stream);
int sedt_stream_reset(int32_t* state, int64_t state_bytes, const int32_t* which, int K, int S, int32_t* status, void* stream);

/* sedt_stream_append / sedt_stream_cut (csrc/stream.hip; no counterpart in the reference): the waveform rings of S live streams, one
 * [S][ring_samples] float32 device tensor.  Jobs are int32 tables of four words a job, given twice: `jobs_host` is checked here,
 * `jobs` is the device copy the kernel reads (it skips a job that is out of range).  Dword loads and stores only.
 *   append  job {stream, ring write position, offset into the flat staged vector src [src_len], n}: n samples into the stream's ring,
 *           wrapping at ring_samples (n <= ring_samples).  One launch for all jobs; n_jobs == 0 launches nothing.
 *   cut     job {stream, ring read position, length, destination row}: wave[row][0 .. length) from the ring across the wrap point,
 *           wave[row][length .. window) zeros; a row of wave [B][window] without a job is zeroed whole.  One launch fills all B rows.
 * Positions inside 0 .. ring_samples-1, length <= window <= ring_samples, streams and rows in range, one job per row at the most. */
int sedt_stream_append(const float* src, int64_t src_len, const int32_t* jobs_host, const int32_t* jobs, int n_jobs, float* ring, int S,
                       int ring_samples, void* stream);
int sedt_stream_cut(const float* ring, int S, int ring_samples, const int32_t* jobs_host, const int32_t* jobs, int n_jobs, float* wave, int B,
                    int window, void* stream);

/* sedt_recording_event_counts / sedt_recording_segment_counts (no counterpart in the reference, which scores 10 s dataset clips only;
 * DESIGN.md section 4, "Scoring recordings", holds the definition and tests/recording_metrics_ref.py restates it): the stitched event
 * lists of sedt_stitch_events scored against the recordings' annotations where they lie - lists in, counts out.
 * Scope: per fusion strategy, threshold k, recording r, class c.  Float64, plain subtract / multiply / divide / compare, no contraction.
 *   estimates   the first count[k][r][c] slots of the stitch output out[k][r][c] (onset = the f64 in words 0-1, offset = the f64 in
 *               words 2-3), as stitch wrote them: no second clip, no duration filter; ascending by onset and disjoint.
 *   references  the recording's annotated events of class c, sorted by the host by (onset, offset, input order); any number of them,
 *               and those of one class may overlap.  CSR over (reference recording, class): the events of class c of reference
 *               recording i are ref_on / ref_end [ref_off[i * C + c] .. ref_off[i * C + c + 1]); ref_off [n_ref_rec * C + 1] int32,
 *               n_ref_events the length of ref_on / ref_end (offsets are clamped to it).
 *   evaluated   only recordings with an entry in the reference: rec_idx[r] = -1 (or outside 0 .. n_ref_rec - 1) adds nothing anywhere -
 *               deliberately simpler than the clip-level outer merge of sedt_event_metrics_update.  A recording annotated with an
 *               empty list is evaluated: its estimates count as n_sys, as false positives and as I.
 *   event-based a hit is |on_r - on_e| <= t_collar and |off_r - off_e| <= max(t_collar, pct * (off_r - on_r)), sed_eval's test as
 *               event_hit_graph writes it; tp = the size of a maximum-cardinality matching of the hit graph of class c over the WHOLE
 *               recording, or (optimal == 0) of sed_eval's greedy pass: references in table order, each takes the first estimate
 *               in onset order that is still free and that it hits.
 *   no limit    a hit needs onsets within t_collar, so the two lists are merged by onset (at equal onsets the estimate first) and a
 *               BLOCK is closed between two consecutive items a <= b of the merged order with fl(b - a) > t_collar.  No hit
 *               crosses such a cut: for p <= a < b <= q the real difference q - p >= b - a, rounding is monotone, so fl(q - p) >=
 *               fl(b - a) > t_collar.  The matching (maximum, or greedy in the orders above) is the sum over the blocks.  Blocks
 *               are formed while both lists have items left: what remains of one list behind the last block matches nothing and is
 *               not walked.  A block holds at most 64 references and 64 estimates; a denser one raises status 2, it is never
 *               silently mis-counted.
 *   presence    per class "count[k][r][c] > 0" against "class c has a reference event in r": tag_counts {tp, fp, fn}.
 *   segments    (sedt_recording_segment_counts) at time_resolution rho an event makes its class active in the segments floor(on / rho)
 *               <= s < ceil(off / rho), both quotients float64 divisions; events of a class OR together, an empty range sets
 *               nothing.  Class-wise seg_counts {tp, n_ref, n_sys}; per segment over the classes S += min(Nref, Nsys) - Ntp,
 *               D += max(0, Nref - Nsys), I += max(0, Nsys - Nref).  The recording spans n_words[r] words of 64 segments (int32 [R];
 *               the host passes ceil(ceil(max(rec_dur[r], largest reference offset) / rho) / 64)); segments past them are not
 *               counted.  No limit on the number of segments: the sweep holds two 64-segment words per class.
 * Inputs: sedt_stitch_events' count [K][R][C], out [K][R][C][cap][8 words] (8-byte aligned), status [K][R] (`stitch_status`) and cap;
 * rec_idx [R] int32: the recording's index in the reference table.
 * Counters (int64, integer atomics only, so the sums do not depend on launch order; zero them per evaluation), row `fusion` of
 *   ev_counts [n_fusion][K][C][3], tag_counts [n_fusion][K][C][3], seg_counts [n_fusion][K][C][3], sdi_counts [n_fusion][K][3].
 * status [K][R] int32, written by every launch: 0; 1 the stitch status of (k, r) is non-zero or some count[k][r][c] > cap (the lists
 *   are not complete); 4 a list (estimates or references) is not ascending by onset or holds a non-finite time; 2 a block over
 *   capacity (event counts only) - in this order of precedence.  With a status raised the counters may hold partial sums of that
 *   recording.  count is clamped to 0 .. cap before it indexes anything: nothing is read or written out of bounds in any case.
 * 1 <= C <= 63, 1 <= K <= 1024, R >= 0 (R == 0 launches nothing), cap >= 1; t_collar finite and >= 0; time_resolution finite and > 0.
 * Events per list and segments per recording are bounded by int32 indexing only. */
int sedt_recording_event_counts(const int32_t* count, const int32_t* out, const int32_t* stitch_status, const int32_t* rec_idx,
                                const int32_t* ref_off, const double* ref_on, const double* ref_end, int n_ref_rec, int n_ref_events,
                                int K, int R, int C, int cap, int n_fusion, int fusion, double t_collar, double pct, int optimal,
                                int64_t* ev_counts, int64_t* tag_counts, int32_t* status, void* stream);
int sedt_recording_segment_counts(const int32_t* count, const int32_t* out, const int32_t* stitch_status, const int32_t* rec_idx,
                                  const int32_t* ref_off, const double* ref_on, const double* ref_end, const int32_t* n_words,
                                  int n_ref_rec, int n_ref_events, int K, int R, int C, int cap, int n_fusion, int fusion,
                                  double time_resolution, int64_t* seg_counts, int64_t* sdi_counts, int32_t* status, void* stream);

/* sedt_recording_psds_counts (no counterpart in the reference, which scores 10 s dataset clips only; DESIGN.md section 4, "PSDS on
 * recordings", holds the definition and tests/recording_psds_ref.py restates it): the PSDS confusion counts of sedt_psds_update for
 * the stitched event lists of sedt_stitch_events against the recordings' annotations - lists in, counts out, no limit on the events
 * of a list.  One wave per (recording, class, threshold).
 * Inputs: those of sedt_recording_event_counts (count, out, stitch_status, cap, rec_idx and the CSR table ref_off / ref_on / ref_end
 * with n_ref_rec and n_ref_events), plus ref_pmax [n_ref_events] float64: per (recording, class) list the running maximum of ref_end
 * (ref_pmax[j] = max of ref_end over the list's events up to and including j), and rec_dur [R] float64: the recordings' lengths in
 * seconds.
 * Definition.  Scope: per fusion strategy, threshold k, recording r with rec_idx[r] inside the table; rec_idx[r] of -1 or out of
 * range adds nothing.  Float64 with no contraction: plain subtract, divide, compare, comparisons >=.  inter(d, g) = min(off_d, off_g) -
 * max(on_d, on_g) counts only where it is > 0; every term is one division added to a running sum.
 *   detections  of class c: the first min(count, cap) slots of out[k][r][c], as stitch wrote them (ascending by onset, disjoint).  A
 *               detection whose off - on is not > 0 takes part in nothing.
 *   references  of class c': the table's list of (rec_idx[r], c'), in table order.  One whose end - on is not > 0 takes part in nothing.
 *   DTC   p_d = sum of inter(d, g) / dur_d over the references g of d's class, in table order;  d passes when p_d >= dtc;
 *   GTC   v_g = sum of inter(d, g) / dur_g over the detections of g's class that passed, in onset order;  v_g >= gtc:
 *         counts[c][c] += 1;
 *   CTTC  for every d that failed the DTC and each other class c': sum of inter(d, g) / dur_d over the references of class c' >= cttc:
 *         counts[class(d)][c'] += 1;  independently (min(off_d, rec_dur[r]) - max(on_d, 0)) / dur_d >= cttc: counts[class(d)][C] += 1
 *         (the world column, a false positive).
 * A term with inter <= 0 adds nothing, so only items that can overlap are walked, the kept terms in the stated order: the references
 * from the first j with ref_pmax[j] > on_d (binary search) while ref_on[j] < off_d; the detections from the first d with max(on_d,
 * off_d) > on_g (binary search; the detections are disjoint) while on_d < off_g.  A reference that spans the recording makes every
 * scan of its class start at it: time, not correctness.
 * pass [K][R][C][ceil(cap / 64)] uint64: workspace of the launch (the DTC pass bits of every 64 detections; the wave that writes a word
 *   is the only one that reads it).  8-byte aligned; its contents before and after the launch mean nothing.
 * counts [n_fusion][K][C][C + 1] int64, row `fusion`: sedt_psds_update's layout, accumulated with integer atomics only (zero them per
 *   evaluation): two runs give equal bytes.
 * status [K][R] int32, written by every launch: 0; 1 the stitch status of (k, r) is non-zero or some count[k][r][c] > cap; 4 a list holds
 *   a non-finite time, is not ascending by onset, or estimates overlap (an onset before the previous offset) - 1 before 4.  With a
 *   status raised the counters may hold partial sums of that recording.  count is clamped to 0 .. cap before it indexes anything, the
 *   CSR offsets are clamped to the table: nothing is read or written out of bounds in any case.
 * 1 <= C <= 63, 1 <= K <= 1024, R >= 0 (R == 0 launches nothing), cap >= 1; dtc, gtc, cttc not NaN. */
int sedt_recording_psds_counts(const int32_t* count, const int32_t* out, const int32_t* stitch_status, const int32_t* rec_idx,
                               const int32_t* ref_off, const double* ref_on, const double* ref_end, const double* ref_pmax,
                               const double* rec_dur, int n_ref_rec, int n_ref_events, int K, int R, int C, int cap, int n_fusion,
                               int fusion, double dtc, double gtc, double cttc, uint64_t* pass, int64_t* counts, int32_t* status,
                               void* stream);

/* ------------------------------------------------------------------ input side on the device (utilities/BoxTransforms.py,
 * utilities/mixup.py)
 * sedt_box_transform: the per-clip feature transforms composed as get_transforms does (BoxTransforms.py:454-490):
 *   ApplyLog (librosa.amplitude_to_db: 10 log10(max(1e-10, x^2)), clamped at clip-max - 80 dB; apply_log = 0 skips it)
 *   -> PadOrTrunc to `frames` rows (zero rows appended) -> TimeMask (rows [tm_t0, tm_t0 + tm_t) zeroed)
 *   -> FreqMask (bands [fm_f0, fm_f0 + fm_f) := their mean over the clip when fill_mean, else fill_const; only if fm_on)
 *   -> FreqShift (np.roll by fs_shift bands, wrapped bands zeroed) -> (x - mean[band]) / std[band] in float64 (Scaler.normalize;
 *   mean/std may be null: no normalisation).  The random parameters are drawn by the caller exactly as the reference's
 *   transform classes draw them; aug = B records of 8 int32 {nframes_raw, tm_t, tm_t0, fm_f, fm_f0, fm_on, fs_shift, 0}.
 *   amp [B][raw_stride][F] f32 (rows >= nframes_raw ignored), out [B][1][frames][F] f32.  One workgroup per clip, the clip
 *   stays in LDS between the passes (frames * F * 4 bytes <= 160 KB).
 * sedt_mixup: out[i] = lam * x1[src1] + (1 - lam) * x2[src2] (mode 0), x1[src1] (1) or x2[src2] (2); jobs = n_out records
 *   {int32 src1, src2, mode; float lam} (mixup.py:35, 142: the label bookkeeping stays on the host). */
int sedt_box_transform(const float* amp, int64_t raw_stride, const void* aug, const double* mean, const double* stdv, int B,
                       int frames, int F, int apply_log, int fill_mean, float fill_const, float* out, void* stream);
int sedt_mixup(const float* x1, const float* x2, const void* jobs, int n_out, int64_t clip_elems, float* out, void* stream);
/* sedt_box_transform_views: BOTH views of the mean-teacher recipe from ONE raw clip in one launch - what the reference's noisy chain
 * (get_transforms(noise_dict_params={"mean": 0., "snr": snr}, ...), train_ss_sedt.py:87-97) makes of a clip: AugmentGaussianNoise
 * (BoxTransforms.py:121-180) turns it into the pair (data, noisy data), every later transform then runs on both members with its own
 * random draw (TimeMask skips member 0).  aug = B records SedtViewAug: the sedt_box_transform record of view 0 (teacher) and of view 1
 * (student; both carry the same nframes_raw) and the noise decision of the clip.
 *   view 1 of a clip with noise_on: x + sd[band] * z, sd[band] = sqrt(mean over ALL nframes_raw raw rows of x^2 * 10^(-snr_db / 10))
 *   in f32 (a band of zeros: sd = 0, no noise), each band summed in a fixed order; then, per view with its own record, exactly the
 *   chain and the arithmetic of sedt_box_transform (the 80 dB floor hangs from that view's own maximum).  View 0, and view 1 of a
 *   clip with noise_on = 0, are bit-identical to sedt_box_transform run with that view's record.
 * z, one STANDARD normal per raw element, comes from one of two sources:
 *   injected  z != null: f32 [B][raw_stride][F], laid out like amp (rows >= nframes_raw ignored; the kernel scales it by sd) - how a
 *             test replays the reference's np.random.normal draw;
 *   drawn     z == null: counter-based.  Element (clip b of the launch, raw row t, band c) has the stream index
 *             e = offset + (b * raw_stride + t) * F + c (F and offset even); the elements 2p, 2p + 1 share one Box-Muller pair of
 *             a = rng32(s, 2p), b = rng32(s, 2p + 1), s = seed + (seed_ptr ? *seed_ptr : 0), rng32 the hash of the dropout
 *             kernels: u1 = ((a >> 8) + 1) * 2^-24 in (0, 1], u2 = (b >> 8) * 2^-24, r = sqrt(-2 ln u1),
 *             z[2p] = r cos(2 pi u2), z[2p + 1] = r sin(2 pi u2).  The top 24 bits of each hash make u1, u2 exact in f32, so the
 *             device stream equals a float64 restatement from the same integers to the rounding of logf / sincospif (|z| <= 5.77).
 *             The caller advances `offset` by B * raw_stride * F per call; seed_ptr lets a captured launch take a device word
 *             the step itself advances.
 * Grid (B, 2): one workgroup per (clip, view), the view stays in LDS between the passes like sedt_box_transform; the workgroup of
 * a noisy view reads the raw clip twice (band sums, then the chain; the second read comes from L2 / Infinity Cache).
 * amp [B][raw_stride][F] f32, out0 / out1 [B][1][frames][F] f32. */
typedef struct {
  int32_t nframes_raw;    /* rows of the raw clip actually present */
  int32_t tm_t, tm_t0;    /* time mask: rows [tm_t0, tm_t0 + tm_t) zeroed (tm_t = 0: off) */
  int32_t fm_f, fm_f0;    /* frequency mask: bands [fm_f0, fm_f0 + fm_f) overwritten if fm_on */
  int32_t fm_on;
  int32_t fs_shift;       /* frequency shift in bands (0: off) */
  int32_t pad_;
} SedtClipAug;            /* the record of sedt_box_transform */
typedef struct {
  SedtClipAug view[2];    /* 0: teacher / labelled pass, 1: student */
  int32_t noise_on;       /* 1: view 1 starts from x + sd * z, 0: from the same data as view 0 */
  int32_t pad_;
} SedtViewAug;            /* sedt_sizeof index 12 */
int sedt_box_transform_views(const float* amp, int64_t raw_stride, const void* aug, const double* mean, const double* stdv, int B,
                             int frames, int F, int apply_log, int fill_mean, float fill_const, float snr_db, const float* z,
                             uint32_t seed, const uint32_t* seed_ptr, uint64_t offset, float* out0, float* out1, void* stream);
/* sedt_scaler_update: one batch of the dataset Scaler's fit (utilities/Scaler.py:37-100, means / calculate_scaler over the data set
 * that passes through get_transforms(frames): ApplyLog -> PadOrTrunc -> ToTensor) on the device, so that the statistics are those of
 * the very features sedt_box_transform later normalises: pass 1 of that kernel (dB, the clip maximum over ALL nframes_raw[b] raw rows,
 * the 80 dB floor on the kept real rows; apply_log = 0 skips it) and nothing after it - no mask, no shift, no normalisation.
 *   stage 1 (one workgroup of 1024 per clip, the clip in LDS): clip_stats[b][0][c] = mean over the `frames` rows of v widened to
 *     float64, clip_stats[b][1][c] = mean of fl32(v * v) widened (the reference squares the f32 array, :57, before the float64 mean).
 *     Rows >= min(nframes_raw[b], frames) are PadOrTrunc's zeros: they add nothing and count in the divisor.  Thread (g, c) adds rows
 *     g, g + G, ... of band c (G = 1024 / F), then the G partials of a band are added in index order.
 *   stage 2 (a second launch of one workgroup, behind stage 1 on the same stream): acc[k][c] += clip_stats[b][k][c] for
 *     b = 0 .. B-1 in that order (the reference's `self.mean_ += mean(sample)`, :67-75), count[0] += B.
 * No floating-point atomics: acc is a function of the sequence of clips alone, however it is cut into batches.  The caller zeroes
 * acc and count before the first batch and divides by count at the end (mean_ = acc[0] / count, mean_of_square_ = acc[1] / count).
 * amp [B][raw_stride][F] f32 (rows >= nframes_raw[b] ignored; nframes_raw is clamped to raw_stride), nframes_raw int32 [B],
 * clip_stats float64 [B][2][F] scratch, acc float64 [2][F], count int64 [1], all device memory.
 * frames * F * 4 + 2 * G * F * 8 + 64 bytes <= 160 KB of LDS, F <= 1024; otherwise an error. */
int sedt_scaler_update(const float* amp, int64_t raw_stride, const int32_t* nframes_raw, int B, int frames, int F, int apply_log,
                       double* clip_stats, double* acc, int64_t* count, void* stream);
/* sedt_mel_spectrogram: waveform -> mel amplitudes, what the reference's load_and_compute_mel_spec (data_utils/SedData.py:195-217,
 * compute_log=False) gets from librosa - stft(n_fft, hop, win_length = n_window, window = hamming, center = True, pad_mode =
 * 'reflect'), magnitude, filters.mel(htk = False, norm = None), transposed - for a whole batch in ONE launch:
 *   frame t of clip b (t < nframes[b] = 1 + nsamples[b] / hop) = padded samples [t hop, t hop + n_fft), padded index q being sample
 *   q - n_fft/2 reflected at the clip's ends (j < 0 -> -j; j >= n -> 2 (n - 1) - j); times window[i] (f32 [n_fft]: the n_window-point
 *   window centred, zeros left of (n_fft - n_window) / 2 and right of it - the kernel reads only the samples under it);
 *   S = |rfft|, n_fft/2 + 1 bins, by an n_fft/2-point complex f32 FFT in LDS (radix-4 Stockham) and the real-input split;
 *   out[b][t][m] = sum_i band_w[band_off[m] + i] * S[band_bin0[m] + i], i = 0 .. band_off[m + 1] - band_off[m] - 1 in that order.
 * wave [B][wave_stride] f32 (SEDT_F32) or int16 PCM (SEDT_I16: sample = x / 32768, so an int16 batch gives the bits of the f32 batch
 * x / 32768); nsamples int32 [B] DEVICE memory (clamped to 1 .. wave_stride; the caller, who knows the lengths, refuses a clip shorter
 * than n_fft/2 + 1 samples, which would need a second reflection).  out f32 [B][out_rows][n_mels]: rows nframes[b] .. out_rows - 1
 * are written as 0, frames past out_rows are dropped.  Tables, all device memory, made once on the host in float64 and rounded
 * (utilities/mel.py mel_tables): window f32 [n_fft]; twiddle f32 [2][n_fft/2 + 1] = cos and -sin of 2 pi t / n_fft - no device
 * sincos; band_bin0 int32 [n_mels], band_off int32 [n_mels + 1], band_w f32 [n_weights] - the filterbank's non-zero run of every band.
 * A workgroup owns 4 consecutive frames of one clip; no floating-point atomics, so a clip's bits depend neither on B nor on the other
 * clips.  No allocation, no synchronisation, capturable.  Envelope (sedt_mel_ok, 1 = inside): n_fft 512, 1024 or 2048;
 * 1 <= n_window <= n_fft; hop >= 1; 1 <= n_mels <= 128.  B <= 65535. */
int sedt_mel_ok(int n_fft, int n_window, int hop, int n_mels);
int sedt_mel_spectrogram(const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* nsamples, int B, float* out,
                         int out_rows, const float* window, const float* twiddle, const int32_t* band_bin0, const int32_t* band_off,
                         const float* band_w, int n_weights, int n_fft, int n_window, int hop, int n_mels, void* stream);
/* sedt_resample: sample-rate conversion L / M = target / source rate (lowest terms) and down-mix of a batch of recordings that share
 * (L, M, taps, H, table), in ONE launch - band-limited interpolation with a Kaiser-windowed sinc in its polyphase form (definition:
 * utilities/resample.py).  For recording b with n_in frames, n_out = min(ceil(n_in L / M), cap), computed in 64-bit integers:
 *   y[n] = sum over k = -H .. taps - 1 - H, ascending, of T[(n M) mod L][k] * m[(n M) div L + k],   n = 0 .. n_out - 1,
 *   m[j] = the mean over the channels of frame j (summed in float64, rounded once; one channel: the sample itself), 0 outside
 *   0 <= j < n_in - no reflection; dst[n_out .. cap - 1] is written as 0.
 * One f32 product, then fmaf in that order: an output's bits depend on its recording, n and the table alone - not on B, on the
 * recording's place in the batch, on cap or on how outputs fall into workgroups (SEDT_RESAMPLE_BLK consecutive outputs each).
 * desc: DEVICE memory, int64 [B][SEDT_RESAMPLE_DESC_WORDS] = {source address, destination address (f32), n_in, cap, channels,
 * dtype (SEDT_F32, or SEDT_I16: a sample is worth x / 32768)}; the source is interleaved (frames, channels) and holds n_in * channels
 * elements, the destination cap floats - so results can go straight into one flat vector at chosen offsets.  The kernel clamps n_in
 * to 0 .. max_in and channels to 1 .. max_channels, the bounds the caller declares.  max_out: the largest cap of the batch (it sizes
 * the grid).  table: DEVICE f32 [taps][L], line k + H holding tap k, column r holding phase (r M) mod L (utilities/resample.py
 * device_table: lanes that own consecutive outputs read consecutive floats); made on the host in float64 and rounded once - the
 * kernel evaluates no Bessel function and no sine.  The identity plan is L = M = taps = 1, H = 0, table {1}: a mono f32 source comes
 * out bit for bit.  No allocation, no synchronisation, no atomics; capturable.
 * Envelope (sedt_resample_ok, 1 = inside): 1 <= L, M <= 4096; 1 <= taps <= 8192; 0 <= H < taps; L * taps * 4 <= 16 MiB of table;
 * ceil(SEDT_RESAMPLE_BLK * M / L) + taps + 1 <= 16384 floats of LDS; 1 <= max_channels <= 64; 1 <= max_in <= 2^40.  Outside it, or
 * with B > 65535 or a null pointer, sedt_resample returns non-zero with a message before it touches a pointer. */
#define SEDT_RESAMPLE_BLK 1024
#define SEDT_RESAMPLE_DESC_WORDS 6
int sedt_resample_ok(int L, int M, int taps, int H, int max_channels, int64_t max_in);
int sedt_resample(const int64_t* desc, int B, int64_t max_out, const float* table, int L, int M, int taps, int H, int max_channels,
                  int64_t max_in, void* stream);
/* sedt_cut_clips (no counterpart as a kernel: the reference cuts its 10 s clips and encodes their strong labels on the host,
 * data_utils/DataLoad.py and utilities/BoxEncoder.py encode_strong_df; DESIGN.md section 4, "Training on recordings"): a training batch
 * cut from annotated recordings that live on the device, in ONE launch - the windows and the windows' target tables.
 * Inputs: flat f32 [flat_len], the recordings one behind the other; rec_off / rec_len int64 [n_rec], recording r = flat[rec_off[r] ..
 * rec_off[r] + rec_len[r]); the picks pick_rec int32 [B], pick_start int64 [B] (any sample index >= 0); window samples per clip; sr.
 * Event table, per recording sorted by (onset, offset, input order): ev_off int32 [n_rec + 1], ev_on / ev_end float64 seconds, ev_cls
 * int32, ev_pmax float64 = the running maximum of ev_end inside the recording, [n_events] each (at least one element allocated).
 * wave f32 [B][window]: row b = samples pick_start[b] .. pick_start[b] + window - 1 of recording pick_rec[b], bit for bit; positions past
 *   the recording's end are 0.  The source is only 4-byte aligned: 16-byte loads where its address allows them.
 * targets, float64 with plain subtract / multiply / divide / compare (no contraction): W = window / sr, t0 = pick_start[b] / sr,
 *   t1 = t0 + W; for every event (c, on, end) of the recording in table order a = max(on, t0) - t0, z = min(end, t1) - t0; kept iff
 *   z - a > 0 and z - a >= min_event_seconds; label c (int64), box (float32(((a + z) * 0.5) / W), float32((z - a) / W)).  Events of
 *   one class that overlap are kept as annotated.  Two binary searches bound the scan (first ev_pmax > t0, first ev_on >= t1), so a
 *   recording may hold any number of events.
 * blob (8-byte aligned, 8 B + 16 + 16 B max_targets bytes): the layout of sedt.TargetTables(batch=B, ns=B, n_lab=B, max_targets,
 *   with_ratio=False) - int32 lab_off [B + 1] | box_off [B + 1] | B | B, then lab_cat int64 [B max_targets], then box_cat f32
 *   [B max_targets][2]; lab_off == box_off, exclusive scans over the clips made inside the launch.  Only live entries are written.
 * status int32 [B]: 0; 1 more than max_targets events survive in the clip - the first max_targets in table order are written; 2 the
 *   pick is not inside the table (pick_rec outside 0 .. n_rec - 1 or pick_start < 0): a row of zeros and no events.
 * Offsets, lengths and event ranges are clamped to flat_len / n_events before they index anything.  No allocation, no
 * synchronisation, no atomics; capturable.  Grid: B * ceil(window / SEDT_CLIPS_CHUNK) workgroups copy, one more owns the targets.
 * Envelope: 1 <= B <= SEDT_CLIPS_MAXB, 1 <= max_targets <= 63, 1 <= window < 2^31, sr >= 1, n_rec >= 1; outside it, with a NaN
 * min_event_seconds or a null pointer, the call returns non-zero with a message before it touches a pointer. */
#define SEDT_CLIPS_MAXB 1024
#define SEDT_CLIPS_CHUNK 2048
int sedt_cut_clips(const float* flat, int64_t flat_len, const int64_t* rec_off, const int64_t* rec_len, int n_rec,
                   const int32_t* pick_rec, const int64_t* pick_start, int B, int64_t window, int sr, const int32_t* ev_off,
                   const double* ev_on, const double* ev_end, const int32_t* ev_cls, const double* ev_pmax, int n_events, int max_targets,
                   double min_event_seconds, float* wave, void* blob, int32_t* status, void* stream);
/* sedt_bank_stats (staging half of "Soundscapes synthesized on the device"): the energy and the peak of every
 * source of a sound bank - flat f32 [flat_len], source s = flat[src_off[s] .. src_off[s] + src_len[s]), src_off / src_len int64 [n_src]
 * (clamped to flat_len before they index anything).  sumsq float64 [n_src] = the sum of x * x, every square and every addition in
 * float64; peak f32 [n_src] = max |x| (0 for an empty source; a NaN sample leaves the peak alone and makes sumsq NaN).  One workgroup
 * of 256 per source: thread t adds elements t, t + 256, ... in that order, then a fixed tree over the 256 partial sums - no atomics,
 * so two calls give the same bits.  No allocation, no synchronisation; capturable.  n_src < 1, flat_len < 0 or a null pointer:
 * non-zero with a message before a pointer is touched. */
int sedt_bank_stats(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src, double* sumsq,
                    float* peak, void* stream);
/* sedt_soundscape (no counterpart as a kernel: the reference trains on soundscapes mixed and annotated offline - URBAN-SED, DESED's
 * synthetic subset - whose annotations data_utils/collapse_event.py merged per class; DESIGN.md section 4, "Soundscapes synthesized on
 * the device"): a training batch of B clips of `window` samples MIXED from a bank of isolated sounds and background recordings that
 * live on the device, and the clips' target tables, in ONE call.
 * Inputs: the bank as for sedt_bank_stats; bg [B] and ev [ev_off[B]] DEVICE records, clip b's events ev[ev_off[b] .. ev_off[b + 1])
 * in plan order (ev_off int32 [B + 1]; at least one ev record allocated).
 * wave f32 [B][window], float32 with every operation rounded on its own (no contraction).  For sample t of clip b:
 *   acc = bg.gain * src[(bg.start + t) mod len] of source bg.src - a background shorter than the window loops; bg.src == -1: acc = 0;
 *   for every event k of the clip in plan order with onset <= t < e_k = min(onset + n, window), i = t - onset:
 *     acc = acc + ((gain * w(i)) * src[src_start + i]),  w(i) = min(w_in, w_out),
 *     w_in = i < fade ? float((double)(i + 1) / (double)(fade + 1)) : 1, w_out = n - 1 - i < fade ? float((double)(n - i) /
 *     (double)(fade + 1)) : 1 (linear ramps of `fade` samples at both ends; float64 divisions, only inside a ramp; fade < 0 is 0);
 *   peak[b] = max over t of |acc|; scale[b] = peak[b] > peak_limit ? float((double)peak_limit / (double)peak[b]) : 1;
 *   wave[b][t] = acc * scale[b], acc itself when the scale is 1.
 * targets: every valid event gives (cls, onset, e_k) in samples.  collapse != 0: the events of one class, sorted by (onset, end), are
 *   merged - an event whose onset <= the running end of its predecessor joins it and the end becomes the maximum (touching events
 *   included: data_utils/collapse_event.py collapse), on the integer sample grid.  Then sedt_cut_clips' float64 box formula with
 *   a = onset / sr, z = end / sr, W = window / sr: kept iff z - a > 0 and z - a >= min_event_seconds; label cls (int64), box
 *   (float32(((a + z) * 0.5) / W), float32((z - a) / W)); the kept ones in the order (onset, end, cls).
 * blob: exactly sedt_cut_clips' (8-byte aligned, 8 B + 16 + 16 B max_targets bytes; every clip strong).
 * status int32 [B]: 0; 1 more than max_targets kept events - the first max_targets are written; 2 (it wins over 1) a record of the
 *   clip is not inside the bank: an event with src outside 0 .. n_src - 1, src_start < 0, n < 0, src_start + n > the source's length or
 *   onset < 0; a background with src outside -1 .. n_src - 1 or start outside [0, length); or a clip with more than SEDT_SCAPE_MAXEV
 *   events (the first SEDT_SCAPE_MAXEV are used).  Such an event or background contributes nothing and yields no target.
 * Nothing is read out of range: sources are clamped to flat_len; ev_off[B] is clamped to 0 .. SEDT_SCAPE_MAXEV * B and every clip's
 * range to it.  part f32 [B][ceil(window / SEDT_SCAPE_CHUNK)] is scratch.
 * Two kernels behind one another on `stream`: (1) workgroup 0 owns the targets (one walk over the batch in tiles of
 * consecutive clips: a tile's events resolved one per thread, one wave per clip merges and orders in registers, the survivors so
 * far are the next tile's offset), B * ceil(window / SEDT_SCAPE_CHUNK) more mix one chunk each - 16-byte stores on the destination's boundaries, 16-byte loads
 * where a source address allows them - and write the chunk's max |acc| to part; (2) one workgroup per chunk reduces its clip's row of
 * part, the first writes peak / scale, and the chunk is rescaled only when scale != 1.  A maximum has no order: no floating-point
 * atomics, the bits depend on the clip's records alone.  No allocation, no synchronisation; capturable.
 * Envelope: 1 <= B <= SEDT_SCAPE_MAXB, 1 <= max_targets <= 63, 1 <= window < 2^31, sr >= 1, n_src >= 1; outside it, with a NaN
 * min_event_seconds or peak_limit, peak_limit <= 0 or a null pointer, the call returns non-zero with a message before it touches a
 * pointer. */
#define SEDT_SCAPE_MAXB 1024
#define SEDT_SCAPE_MAXEV 63
#define SEDT_SCAPE_CHUNK 2048
typedef struct {
  int32_t src, cls;                 /* source index into the bank; class index */
  int64_t src_start, n, onset;      /* samples src_start .. src_start + n - 1 of the source are laid at sample `onset` of the clip */
  float gain;
  int32_t fade;                     /* samples of the linear ramp at both ends */
} SedtScapeEvent;                   /* 40 bytes; sedt_sizeof index 13 */
typedef struct {
  int32_t src, pad;                 /* source index, -1: no background */
  int64_t start;                    /* the background's sample under sample 0 of the clip */
  float gain;
  int32_t pad2;
} SedtScapeBg;                      /* 24 bytes; sedt_sizeof index 14 */
int sedt_soundscape(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                    const SedtScapeBg* bg, const SedtScapeEvent* ev, const int32_t* ev_off, int B, int64_t window, int sr,
                    int max_targets, double min_event_seconds, int collapse, float peak_limit, float* wave, float* part, float* peak,
                    float* scale, void* blob, int32_t* status, void* stream);
/* sedt_loudness (no counterpart in the reference; DESIGN.md section 4, "Loudness (BS.1770) on the device"; tests/loudness_ref.py
 * restates it): the ITU-R BS.1770-4 programme loudness of every source of a bank, one channel with channel weight 1 - the bank as for
 * sedt_bank_stats, clamped to flat_len in the same way.  The host finishes: L = -0.691 + 10 log10(zbar) LUFS, -inf for zbar == 0.
 * coef float64 [10], DEVICE: b0 b1 b2 a1 a2 of the shelf stage, then of the high-pass stage (a0 = 1 dropped).  Each stage is
 *   transposed direct form II in float64 on the float32 samples widened, from zero state, the shelf first:
 *   o = b0 v + s0; s0 = b1 v - a1 o + s1; s1 = b2 v - a2 o.  Products and sums may be contracted into FMAs.
 * hop = H samples (100 ms).  e_h = the sum of y * y over hop h, in sample order.  n >= 4 H: J = n / H - 3 blocks of 4 H samples with
 *   75 % overlap, z_j = (e_j + e_j+1 + e_j+2 + e_j+3) / (4 H); a trailing partial hop is not used.  n < 4 H has no block in the
 *   standard: here it is ONE block over all its samples, z_0 = (e_0 + e_1 + ..) / n (0 for n = 0), J = 1, flagged short.
 * Gates in the z domain: absolute z_j > z_abs (10^((-70 + 0.691) / 10) for the standard's -70 LUFS); relative z_j > 0.1 * (the mean
 *   of z over the blocks that pass the absolute gate).  zbar float64 [n_src] = the mean of z_j over the blocks that pass both, 0 when
 *   none does, NaN when a hop energy is not finite (a NaN or infinite sample).  counts int32 [n_src][4] = J, the blocks that pass the
 *   absolute gate, those that pass both, short (0 / 1).
 * hop_map float64 [16], DEVICE, row-major [4][4]: the state of the cascade (shelf s0 s1, high-pass s0 s1) after H zero-input samples
 *   from each unit state - column k from unit state k.  The filter is linear, so the state at the start of hop h + 1 is
 *   hop_map . (the state at the start of hop h) + (the state hop h leaves when filtered from zero state): the hops are filtered in
 *   parallel, 256 per round - pass A from zero state, one thread walks the 256 end states into start states and carries the last one
 *   into the next round, pass B from the true start state sums y * y.  Exact up to rounding (DESIGN quotes the measurement).
 * work float64 [work_len]: the hop energies; source s owns src_len[s] / H + 1 doubles behind those of the sources before it, so
 *   work_len >= the sum of (src_len[s] / H + 1).  The lengths live on the device and the call does not synchronise: the entry point
 *   refuses work_len < n_src, and a source whose range does not fit into work_len is NOT measured - zbar NaN, its four counts -1,
 *   nothing written outside work (utilities/loudness.py raises on it).
 * One launch, one workgroup of 256 per source.  The gate passes are fixed-order LDS trees (thread t adds blocks t, t + 256, ...): no
 * floating-point atomics, two calls give the same bits.  No allocation, no synchronisation; capturable.  n_src < 1, flat_len < 0,
 * hop < 1, a z_abs that is not a number >= 0, work_len < n_src or a null pointer: non-zero with a message before a pointer is touched. */
int sedt_loudness(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src, const double* coef,
                  const double* hop_map, int hop, double z_abs, double* work, int64_t work_len, double* zbar, int32_t* counts,
                  void* stream);
/* sedt_scale_sources: flat[src_off[s] + i] *= gain[s] for every sample of every source (the bank as for sedt_bank_stats, clamped in the
 * same way; the sources must not overlap), in place and in one launch - the second half of a loudness normalisation.  One float32
 * multiplication per sample; 16-byte accesses on the 16-byte boundaries of a source, scalar head and tail; a source with gain 1 is
 * not written at all.  No allocation, no synchronisation; capturable.  n_src < 1, flat_len < 0 or a null pointer: non-zero with a
 * message before a pointer is touched. */
int sedt_scale_sources(float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src, const float* gain,
                       void* stream);
/* sedt_stretch (no counterpart in the reference, whose corpora were generated offline; DESIGN.md section 4, "Pitch shift and time
 * stretch on the device"; tests/stretch_ref.py restates it in float64): n_jobs excerpts of a bank, each stretched in time by its own
 * duration factor f and shifted in pitch by its own p semitones - a phase vocoder followed by band-limited resampling at a real ratio.
 * Job e reads x = flat[src_off .. src_off + n) and writes y = dst[dst_off .. dst_off + m).  With alpha = 2^(p / 12), g = f alpha:
 *   m = floor(n f + 0.5), m1 = floor(n g + 0.5), r = 1 / g - float64 on the host, carried in the record.
 *   STFT: N = n_fft, hop = N / 4, periodic Hann window (`window` f32 [N], float64 rounded once), centred with zeros outside [0, n):
 *     frame t covers samples t hop - N/2 .. t hop + N/2 - 1; T = 1 + n div hop frames of K = N/2 + 1 bins; frames T, T + 1 are zero.
 *   Vocoder: U = the number of steps u >= 0 with fl64(u r) < T (ceil(T / r) up to the rounding of the product).  s = fl64(u r),
 *     i = floor(s), a = s - i; mag = (1 - a) |D_i| + a |D_i+1|; S_u = mag exp(i phi_u); phi_0 = arg D_0; phi_u+1 = phi_u + omega_k +
 *     wrap(arg D_i+1 - arg D_i - omega_k), omega_k = 2 pi hop k / N, wrap(d) = d - 2 pi rint(d / 2 pi), arg 0 = 0.  Magnitudes, angles,
 *     the phase and its sine and cosine are float64 on the f32 spectrum widened; S is rounded to f32 once.
 *   Inverse: the inverse real FFT of S_u (the imaginary parts of bins 0 and N/2 dropped) times the window, frame u laid at u hop;
 *     sample q adds its at most four frames in ascending frame order and is divided by ws[q] = the sum of window^2 over the same
 *     frames (f32) where ws[q] > 1e-8; z = samples N/2 .. N/2 + m1 - 1 (zero where no frame reaches).
 *   Resampling: y[i] = sum over j of (s w(s (fl64(i alpha) - j))) z[j], j ascending over 0 <= j < m1, s = min(1, 1 / alpha); w is read
 *     from `wtab` f32 [512 zero_crossings + 1], wtab[q] = the Kaiser-windowed sinc at q / 512 (float64 rounded once), interpolated
 *     linearly: pos = |s (t - j)| 512 in float64, q = floor(pos), w = wtab[q] + f32(pos - q) (wtab[q + 1] - wtab[q]); q >= 512
 *     zero_crossings contributes nothing.  f32 sums.
 *   r == 1 (g = 1): T = U = 0 and z = x.  alpha == 1: m == m1 and y = z.
 * twiddle f32 [2][N/2 + 1] is sedt_mel_spectrogram's table.
 * The records exist twice: jobs_host is read by the entry point (refusals, grid sizes), jobs_dev - the same bytes in DEVICE memory -
 * by the kernels, which check every record again before they touch memory.
 * Workspace: the caller's; job e owns floats [ws_off, ws_off + F_e) of it, F_e = 2 T K + 2 U K + U N + m1 rounded up to a multiple
 *   of 4, laid out  D re [T][K] | D im [T][K] | S re [U][K] | S im [U][K] | windowed inverse frames [U][N] | z [m1].  ws_off is a
 *   multiple of 4 and the regions follow one another in job order.  sedt_stretch_workspace returns the bytes a job list needs (the
 *   end of its last region), -1 with a message for a list the entry point would refuse.
 * status int32 [n_jobs]: 0; 2 the DEVICE record does not lie inside the bank, the destination or the workspace, or is outside the
 *   envelope - nothing is read or written for it.
 * Five launches behind one another on `stream` (STFT; vocoder, one thread per job and bin; inverse FFT; overlap-add gather;
 * resampler), no atomics - the same call gives the same bits; no allocation, no synchronisation; capturable.
 * Envelope (sedt_stretch_ok): n_fft 512, 1024 or 2048; 1 <= n <= 2^26; alpha in [0.5, 2] (|p| <= 12); f = 1 / (r alpha) in [0.5, 2];
 *   m, m1, T, U as defined above.  A job outside it, n < 1, regions out of order, a workspace smaller than the list needs, a negative
 *   count or length, n_jobs > 65535, zero_crossings outside 1 .. 64 or a null pointer: non-zero with a message before anything is
 *   launched.  n_jobs == 0 returns 0 and launches nothing. */
typedef struct {
  int64_t src_off, n;               /* the excerpt: flat[src_off .. src_off + n) */
  int64_t dst_off, m;               /* the result: dst[dst_off .. dst_off + m) */
  int64_t m1;                       /* samples between the vocoder and the resampler */
  double r, alpha;                  /* the vocoder's rate 1 / (f alpha); the resampling ratio 2^(p / 12) */
  int32_t T, U;                     /* analysis frames; synthesis frames */
  int64_t ws_off;                   /* the job's first float in the workspace */
} SedtStretchJob;                   /* 72 bytes; sedt_sizeof index 15 */
int sedt_stretch_ok(int n_fft, int64_t n, int64_t m, int64_t m1, double r, double alpha, int T, int U);
int64_t sedt_stretch_workspace(const SedtStretchJob* jobs_host, int n_jobs, int n_fft);
int sedt_stretch(const float* flat, int64_t flat_len, const SedtStretchJob* jobs_host, const SedtStretchJob* jobs_dev, int n_jobs,
                 float* dst, int64_t dst_len, void* workspace, int64_t workspace_bytes, const float* window, const float* twiddle,
                 const float* wtab, int zero_crossings, int n_fft, int32_t* status, void* stream);
/* sedt_reverb (no counterpart in the reference, whose corpora were generated offline; DESIGN.md section 4, "Reverberation on the
 * device"; tests/reverb_ref.py restates it in float64): n_jobs excerpts of a bank, each convolved with a room impulse response (RIR)
 * of a staged RIR bank - uniformly partitioned overlap-save convolution.  N = n_fft, Bs = N / 2, K = N / 2 + 1.
 * The RIR bank.  rir_tab int64 [3][n_rirs]: row 0 the taps L_r (1 <= L_r <= SEDT_REVERB_MAXPART Bs), row 1 the response's first
 *   partition - the responses' P_r = ceil(L_r / Bs) partitions lie behind one another, n_parts in all -, row 2 its first tap in
 *   `taps` (read by sedt_reverb_spectra only).  sedt_reverb_spectra writes h_re / h_im f32 [n_parts][K] in ONE launch: H[r][p] = the
 *   N-point real FFT of taps [p Bs, (p + 1) Bs) of response r followed by Bs zeros (the last partition zero-padded).
 * Job e: x[i] = flat[src_off + i] w(i), 0 <= i < n, w the ramp of sedt_soundscape over n samples with the job's `fade` (one f32
 *   product; fade 0: x itself) - the fades belong to the dry sound, not to its tail; wet = dst[dst_off .. dst_off + n + L - 1), L the
 *   taps of response `rir`.
 *   Input block j, 0 <= j < nb = ceil(n / Bs) + 1, holds x[(j - 1) Bs .. (j + 1) Bs), zero outside [0, n); X[j] = its N-point real
 *     FFT, bins 0 .. N/2, f32.
 *   Output block j, 0 <= j < ceil((n + L - 1) / Bs): Y = the sum over p = 0 .. P - 1, ascending, of X[j - p] H[r][p] (complex f32
 *     products and sums; X[i] = 0 for i outside 0 .. nb - 1); the inverse real FFT of Y (the imaginary parts of bins 0 and N/2
 *     dropped); its LAST Bs samples are wet[j Bs .. (j + 1) Bs), clipped to n + L - 1.
 * twiddle f32 [2][N/2 + 1] is sedt_mel_spectrogram's table.
 * The records and the RIR table exist twice: jobs_host / rir_tab_host are read by the entry point (refusals, grid sizes), jobs_dev /
 * rir_tab_dev - the same bytes in DEVICE memory - by the kernels, which check every record again before they touch memory.
 * Workspace: the caller's; job e owns floats [ws_off, ws_off + F_e), F_e = 2 nb K rounded up to a multiple of 4, laid out
 *   X re [nb][K] | X im [nb][K].  ws_off is a multiple of 4 and the regions follow one another in job order.  sedt_reverb_workspace
 *   returns the bytes a job list needs, -1 with a message for a list the entry point would refuse.
 * status int32 [n_jobs]: 0; 2 the DEVICE record does not lie inside the bank, the destination, the workspace or the RIR table, or is
 *   outside the envelope - nothing is read or written for it.
 * group: the output blocks a workgroup of the second launch keeps in registers (1, 2, 4, 8; 0: the library's choice).  The bits do
 *   not depend on it.
 * Two launches behind one another on `stream` (the blocks' spectra; products, inverse and store), no atomics - the same call gives the
 * same bits; no allocation, no synchronisation; capturable.
 * Envelope (sedt_reverb_ok): n_fft 512, 1024 or 2048; 1 <= n <= 2^26; 0 <= fade <= 2^26; 1 <= L <= SEDT_REVERB_MAXPART n_fft / 2 - at
 *   n_fft 2048 that is 180224 taps: a response of 4 s at 44.1 kHz (176400) fits.  A job or a response outside it, regions or
 *   partitions out of order, a workspace smaller than the list needs, a negative count or length, more than 65535 jobs or responses
 *   or a null pointer: non-zero with a message before anything is launched.  n_jobs == 0 returns 0 and launches nothing. */
#define SEDT_REVERB_MAXPART 176
typedef struct {
  int64_t src_off, n;               /* the dry sound: flat[src_off .. src_off + n) */
  int64_t dst_off;                  /* the wet sound: dst[dst_off .. dst_off + n + L - 1) */
  int32_t rir, fade;                /* the response's index; samples of the linear ramp at both ends of the dry sound */
  int64_t ws_off;                   /* the job's first float in the workspace */
} SedtReverbJob;                    /* 40 bytes; sedt_sizeof index 16 */
int sedt_reverb_ok(int n_fft, int64_t n, int64_t taps, int fade);
int64_t sedt_reverb_workspace(const SedtReverbJob* jobs_host, int n_jobs, int n_fft);
int sedt_reverb_spectra(const float* taps, int64_t taps_len, const int64_t* rir_tab_host, const int64_t* rir_tab_dev, int n_rirs,
                        float* h_re, float* h_im, int64_t n_parts, const float* twiddle, int n_fft, void* stream);
int sedt_reverb(const float* flat, int64_t flat_len, const SedtReverbJob* jobs_host, const SedtReverbJob* jobs_dev, int n_jobs,
                float* dst, int64_t dst_len, void* workspace, int64_t workspace_bytes, const float* h_re, const float* h_im,
                int64_t n_parts, const int64_t* rir_tab_host, const int64_t* rir_tab_dev, int n_rirs, const float* twiddle, int n_fft,
                int group, int32_t* status, void* stream);
/* sedt_reverb_bed: the tails of the wet events of n_beds clips laid over the clips' backgrounds, one row of `window` samples per clip
 * (utilities/soundscape.py hands the row to sedt_soundscape as the clip's background).  float32 with every operation rounded on its
 * own (no contraction).  For sample t of bed c (DEVICE records; the bank as for sedt_bank_stats):
 *   acc = gain * src[(start + t) mod len] of source `src`; src == -1: acc = 0;
 *   for every tail k in tail_lo <= k < tail_hi, ascending, with head <= t - onset < total: acc = acc + (gain_k * flat[wet_off + t - onset]);
 *   dst[dst_off + t] = acc.
 * A background or a tail that does not lie inside flat contributes nothing; a bed whose row does not lie inside dst is not written.
 * One launch, one thread per sample; no atomics, no allocation, no synchronisation; capturable.  dst may be flat itself as long as
 * the rows do not overlap what is read. */
typedef struct {
  int64_t wet_off;                  /* the wet sound's first sample in flat */
  int64_t onset;                    /* its sample 0 lies at sample `onset` of the clip */
  int64_t head, total;              /* samples head .. total - 1 of it are the tail */
  float gain;
  int32_t pad;
} SedtReverbTail;                   /* 40 bytes; sedt_sizeof index 17 */
typedef struct {
  int32_t src, tail_lo;             /* the background's source index, -1: none; the clip's first tail */
  int64_t start;                    /* the background's sample under sample 0 of the clip */
  float gain;
  int32_t tail_hi;                  /* one past the clip's last tail */
  int64_t dst_off;                  /* the bed row: dst[dst_off .. dst_off + window) */
} SedtReverbBed;                    /* 32 bytes; sedt_sizeof index 18 */
int sedt_reverb_bed(const float* flat, int64_t flat_len, const int64_t* src_off, const int64_t* src_len, int n_src,
                    const SedtReverbBed* beds, int n_beds, const SedtReverbTail* tails, int n_tails, int64_t window, float* dst,
                    int64_t dst_len, void* stream);
/* sedt_relevel (no counterpart in the reference, whose corpora were mixed offline by generators that measure every PROCESSED event
 * before they apply its SNR; DESIGN.md section 4, "Levels measured after the effects"; tests/relevel_ref.py restates it in float64):
 * the level of n_jobs regions of flat - an event's bank excerpt, its stretched row, its wet row - and, from it, the gain that brings
 * the region to the job's target, written into the DEVICE records sedt_reverb_bed and sedt_soundscape read.  Nothing is read back.
 * Job e measures flat[off .. off + n), which starts at any sample:
 *   mode 0 (RMS):     level = (the sum of x * x) / n, every square and every addition in float64 in sedt_bank_stats' order - thread t
 *     adds elements t, t + 256, ..., then the fixed tree over the 256 partial sums; counts = n (clamped to 2^31 - 1), 0, 0, 0.
 *   mode 1 (BS.1770): level = zbar and counts exactly as sedt_loudness gives them for a source that is this region: coef, hop_map,
 *     hop and z_abs are its arguments, the rounds of 256 hops with the carried state, both gates and the short-region rule are its
 *     own (one shared device function: the same bits).  The job's hop energies go to work[ws_off .. ws_off + n / hop + 1).
 *   g = float32(target / sqrt(level)), the division and the root in float64.  `target` is the amplitude the region shall have with
 *     every constant folded in by the host: 10^(dB / 20) in mode 0, 10^((LUFS + 0.691) / 20) in mode 1.
 *   level finite and > 0: status 0, g is written to ev[job.ev].gain and to tails[job.tail].gain; an index of -1 is skipped.
 *   otherwise - a silent region, one under the absolute gate in every block, one that holds a NaN or infinite sample: status 1, and
 *     both records keep the gain the host wrote.
 * level float64 [n_jobs], counts int32 [n_jobs][4], status int32 [n_jobs].
 * The records exist twice: jobs_host is read by the entry point (refusals), jobs_dev - the same bytes in DEVICE memory - by the
 * kernel, which checks every record again before it touches memory: status 2, the DEVICE record does not lie inside flat, names a
 * record outside ev [n_ev] / tails [n_tails], has a target that is not a finite number > 0 or a workspace region outside work -
 * nothing but the status is written for it.  A record of ev / tails is named by at most one job of a call.
 * Workspace: the caller's float64 work [work_len]; in mode 1 job e owns n / hop + 1 doubles from ws_off on, the regions follow one
 *   another in job order; mode 0 needs none (work may be null, as coef and hop_map may).  sedt_relevel_workspace returns the DOUBLES
 *   a job list needs, -1 with a message for a list the entry point would refuse.
 * One launch, one workgroup of 256 per job; no atomics, no allocation, no synchronisation - two calls give the same bits; capturable.
 * A null pointer, a negative count or length, mode outside 0 / 1, hop < 1, a z_abs that is not a number >= 0, a job with n < 1, a
 * region outside flat, an index outside its table, a target that is not a finite number > 0, workspace regions out of order or a
 * workspace smaller than the list needs: non-zero with a message before anything is launched.  n_jobs == 0 returns 0 and launches
 * nothing. */
typedef struct {
  int64_t off, n;                   /* the region: flat[off .. off + n) */
  double target;                    /* the amplitude it shall have */
  int32_t ev, tail;                 /* the SedtScapeEvent / SedtReverbTail record that takes the gain, -1: none */
  int64_t ws_off;                   /* the job's first double in the workspace */
} SedtRelevelJob;                   /* 40 bytes; sedt_sizeof index 19 */
int64_t sedt_relevel_workspace(const SedtRelevelJob* jobs_host, int n_jobs, int mode, int hop);
int sedt_relevel(const float* flat, int64_t flat_len, const SedtRelevelJob* jobs_host, const SedtRelevelJob* jobs_dev, int n_jobs, int mode,
                 const double* coef, const double* hop_map, int hop, double z_abs, double* work, int64_t work_len, SedtScapeEvent* ev,
                 int n_ev, SedtReverbTail* tails, int n_tails, double* level, int32_t* counts, int32_t* status, void* stream);
/* sedt_mixup_targets: the LABEL half of mixup_label_unlabel (utilities/mixup.py:129-196; call site engine.py:150-153, between the
 * teacher and the student forward of semi_train) without leaving the device.  Set 1 = the labelled targets (flat tables as
 * sedt_match_targets reads them: lab1/lab_off1 [B1+1], box1/box_off1 [ns1+1], optional ratio1 aligned with lab1, optional split1 =
 * device {ns, n_lab}), set 2 = the pseudo targets sedt_pseudo_labels wrote (all B2 clips with boxes).  For clip i < mix_num:
 * more than max_events events together -> the pseudo target if it has events, else the labelled one; otherwise labels / boxes
 * concatenated (labelled first) with ratio lam[0] for the labelled and lam[1] (= 1 - lam as the host rounds it) for the pseudo
 * labels, unless two events of one class overlap in time -> the labelled target (and clip) replaces the unlabelled one.
 * Clips >= mix_num keep their pseudo target.  Outputs: merged tables (capacity cap events), ratio_out (1 where the reference has no
 * 'ratio'), jobs = B2 sedt_mixup records {i, i, mode, lam} producing the matching features from (x1 = labelled, x2 = unlabelled). */
int sedt_mixup_targets(const int64_t* lab1, const int32_t* lab_off1, const float* box1, const int32_t* box_off1, const float* ratio1,
                       const int32_t* split1, int B1, int ns1, const int64_t* lab2, const int32_t* lab_off2, const float* box2,
                       const int32_t* box_off2, int B2, const float* lam, int mix_num, int max_events, int64_t* lab_out,
                       int32_t* lab_off_out, float* box_out, int32_t* box_off_out, float* ratio_out, int cap, void* jobs,
                       void* stream);
/* sedt_mixup_plan: the LABEL half of mixup_data (utilities/mixup.py:13-127; call sites engine.py:50-53 and 128-133) for a batch whose
 * targets were built on the device - the device restatement of utilities.mixup.plan_mixup_data ("Mix-up and
 * mean-teacher training on recordings").
 * Source: src_blob in the layout sedt_cut_clips writes for B_src all-strong clips of up to max_targets_src events, of which the first B
 * are used under the static split 0 <= ns <= n_lab <= B: clip b has nl(b) labels (0 when b >= n_lab) and nb(b) boxes (0 when b >= ns:
 * a weak clip's boxes are ignored).  index int32 [B] and lam f32 [2] = {lam, 1 - lam} as the host rounds them are device-resident and
 * drawn on the host (utilities.mixup.draw_mixup_data, lam_pair).  For i < mix_num, j = index[i], n1 = nb(i), n2 = nb(j), the first row
 * that applies decides:
 *   n1 == 0 or n2 == 0, and n1 > 0      keep-1: target i, job {i, 0, 1, 0}
 *   n1 == 0 or n2 == 0, and n2 > 0      keep-2: target j, job {0, j, 2, 0}
 *   n1 == 0 and n2 == 0                 weak merge: labels of i then of j, no boxes, ratio lam x nl(i) then (1 - lam) x nl(j), job {i, j, 0, lam}
 *   n1 + n2 > max_events                keep-1
 *   two boxes of one class overlap anywhere in boxes(i) ++ boxes(j), inside clip i alone included (box k carries label k of
 *   labels(i) ++ labels(j); s = c - l / 2, e = c + l / 2 in f32; a clash iff !(e_j < s_k) && !(e_k < s_j))      keep-1
 *   none of the above                   strong merge: labels, boxes, ratios concatenated, job {i, j, 0, lam}
 * Output order: the keeps and strong merges in order of i; clips mix_num .. ns - 1; the weak merges in order of i; clips ns ..
 * n_lab - 1; clips n_lab .. B - 1.  Unchanged clips get job {b, 0, 1, 0} and ratio 1.
 * out_blob: the dynamic-split TargetTables layout of B clips with ratio - int32 lab_off [B + 1] | box_off [B + 1] | ns' | n_lab, at
 * byte 8 B + 16 lab_cat int64 [B max_targets_out], box_cat f32 [B max_targets_out][2], ratio_cat f32 [B max_targets_out]; ns' = ns -
 * #weak merges; box_off is flat beyond ns'; only live entries are written.  jobs: B sedt_mixup records.  status int32 [B], indexed by
 * the SOURCE clip a result belongs to (i for the mixed clips, keep-2 included): 0; 1 the result holds more than max_targets_out labels
 * (the first max_targets_out are written); 2 index[i] is outside 0 .. B - 1 (treated as keep-1).
 * One workgroup; no atomics, no allocation, no synchronisation; deterministic and capturable; source offsets are clamped to the
 * source tables before they index anything.  Envelope: 1 <= B <= B_src <= 1024, 0 <= ns <= n_lab <= B, 0 <= mix_num <= ns (the batch
 * then never shrinks: exactly B results on every draw), 1 <= max_events <= max_targets_out <= 63, 1 <= max_targets_src <= 63; outside
 * it or with a null pointer the call returns non-zero with a message before it touches a pointer. */
int sedt_mixup_plan(const void* src_blob, int B_src, int max_targets_src, int B, int ns, int n_lab, const int32_t* index,
                    const float* lam, int mix_num, int max_events, int max_targets_out, void* out_blob, void* jobs, int32_t* status,
                    void* stream);

/* SP-SEDT query patches (utilities/BoxTransforms.py:315-360, Query.transform_label; boxes from DataLoad.py:57-77 are turned into
 * row ranges on the host): for each of n_patches jobs {clip, s_idx, e_idx, 0} (int32 x 4, device memory) crop rows [s_idx, e_idx)
 * of data f32 [B][T][F], min-max normalise, quantise to 8 bits, resize to 128 rows with Pillow's bilinear resampling arithmetic,
 * de-normalise -> out f32 [n_patches][128][F], bit-identical to the reference pipeline; fixed != 0: copy the 128 rows as they are
 * (fixed_patch_size). */
int sedt_query_patches(const float* data, int B, int T, int F, const void* jobs, int n_patches, int fixed, float* out, void* stream);

/* ------------------------------------------------------------------ host-side matching (sedt/matcher.py:95)
 * HOST pointers.  cost [nlayers][nclips][Q][Nt] f32; clip b owns columns [col_off[b], col_off[b]+ncols[b]).
 * assign [nlayers][nclips][Q]: index (within the clip) of the target matched to query q, or -1.
 * Same optimum as scipy.optimize.linear_sum_assignment (min(Q, n_b) pairs per problem). */
int sedt_hungarian_batch(const float* cost, int nlayers, int nclips, int Q, int Nt, const int32_t* col_off,
                         const int32_t* ncols, int32_t* assign);

#ifdef __cplusplus
}
#endif
#endif
