"""The case table of tests/test_gemm_envelope_gpu.py: one row per (op, mode, shape, layout), each naming the GEMM kernel instance
the dispatcher (sedt_igemm, csrc/igemm.hip) must pick for it.  A plain module, importable without a GPU: tests/test_gemm_split_cpu.py
resolves every row's instance on the host (sedt_igemm_describe never touches the device) and checks the split-K rule over it.

Row fields (dicts, built by the helpers below):
  op      'linear' (ops.linear), 'conv_fwd', 'conv_dgrad', 'wgrad' (ops.wgrad; plain geometry = linear_wgrad with a row scale)
  mode    'bf16' | 'f32' | 'x3' (the f32 mode with the bf16x3 fast path on)
  M N K   linear: x [M, K], w [N, K];   wgrad: dY [K, M] (pixels x Cout), X [K or pixels, Ci]
  geom    (B, Hi, Wi, Ci, Co, k, stride, pad, dil) for the convolutions
  a_off / a_pad, b_off / b_pad, c_off   element offset of a view's first element / extra elements of its row stride:
          linear A = x, B = w, C = out;  wgrad A = dY, B = X
  ep      linear epilogue: 'bias', 'scale', 'relu', 'res', 'out_f32', 'tile' (the tile hint of sedt_igemm)
  rowscale, bias_out   wgrad options (bias_out: the fused column sum when the LDS-DMA kernels take the problem, else ops.colsum)
  expect  the kernel instance, as sedt_igemm_describe prints it
"""

LINEAR, CONV_FWD, CONV_DGRAD, WGRAD = 'linear', 'conv_fwd', 'conv_dgrad', 'wgrad'

GEN_BF16 = 'igemm_kernel<__bf16, 64, 64, false>'
GEN_BF16_T = 'igemm_kernel<__bf16, 64, 64, true>'
GEN_F32 = 'igemm_kernel<float, 64, 64, false>'
GEN_F32_FAST = 'igemm_kernel<float, 64, 64, false, false, true>'
GEN_F32_T = 'igemm_kernel<float, 64, 64, true>'
GEN_X3 = 'igemm_kernel<float, 64, 64, false, true>'
I3_1 = 'igemm3_kernel<64, 64, 1>'
I3_2 = 'igemm3_kernel<64, 64, 2>'
I3_3 = 'igemm3_kernel<64, 64, 3>'
W16_64 = 'igemm3_w16_kernel<64, 64, 3>'
W16_128 = 'igemm3_w16_kernel<64, 128, 3>'
W8_64x128_3 = 'igemm3_w8_kernel<64, 128, 3, 1>'
W8_128 = 'igemm3_w8_kernel<128, 128, 3, 1>'
WG3 = 'wgrad3_kernel<64>'
WG4 = 'wgrad4_kernel<3>'


def lin(name, M, N, K, expect, mode='bf16', a_off=0, a_pad=0, b_off=0, b_pad=0, c_off=0, **ep):
    return dict(name=name, op=LINEAR, mode=mode, M=M, N=N, K=K, a_off=a_off, a_pad=a_pad, b_off=b_off, b_pad=b_pad, c_off=c_off,
                ep=ep, expect=expect)


def conv(name, op, geom, expect, mode='bf16', rowscale=False, bias_out=False, **ep):
    B, Hi, Wi, Ci, Co, k, s, p, d = geom
    Ho = (Hi + 2 * p - d * (k - 1) - 1) // s + 1
    Wo = (Wi + 2 * p - d * (k - 1) - 1) // s + 1
    if op == CONV_FWD:
        M, N, K = B * Ho * Wo, Co, k * k * Ci
    elif op == CONV_DGRAD:
        M, N, K = B * Hi * Wi, Ci, k * k * Co
    else:
        M, N, K = Co, k * k * Ci, B * Ho * Wo
    return dict(name=name, op=op, mode=mode, M=M, N=N, K=K, geom=geom, Ho=Ho, Wo=Wo, a_off=0, a_pad=0, b_off=0, b_pad=0, c_off=0,
                ep=ep, rowscale=rowscale, bias_out=bias_out, expect=expect)


def wg(name, Co, Ci, rows, expect, mode='bf16', a_off=0, a_pad=0, b_off=0, b_pad=0, rowscale=False, bias_out=False):
    """weight gradient of a linear layer: dW [Co, Ci] = dY[rows, Co]^T X[rows, Ci] (ops.wgrad with a plain 1x1 geometry)"""
    c = conv(name, WGRAD, (rows, 1, 1, Ci, Co, 1, 1, 0, 1), expect, mode=mode, rowscale=rowscale, bias_out=bias_out)
    c.update(a_off=a_off, a_pad=a_pad, b_off=b_off, b_pad=b_pad)
    return c


CASES = [
    # ---- forward / dgrad LDS-DMA family (lds_plan, csrc/igemm3.hip): tile rule, ring depth, the 16-wave forms
    lin('k64_one_block', 200, 96, 64, I3_1),                                    # K == one K tile: the 1-stage ring
    lin('k256_m_tail1', 129, 192, 256, I3_2),                                   # M % 64 == 1, S = 2 below K = 320
    lin('k256_m_lt_tile', 40, 72, 256, I3_2),                                   # M and N smaller than one tile, N % 64 == 8
    lin('k256_n_tail', 256, 120, 256, I3_2),                                    # N one 8-block below a 64 / 128 tile
    lin('k448_below_512', 256, 256, 448, I3_3),                                 # K one block below the 512 threshold: 64x64, S = 3
    lin('k512_small16', 512, 192, 512, W16_64, bias=True, relu=True),           # <= 320 tiles, K / 64 even: 16-wave 64x64
    lin('k576_n64_s2', 512, 64, 576, I3_2),                                     # N <= 64 and K <= 576: the 2-stage ring
    lin('k640_n64_s3', 512, 64, 640, W16_64),                                   # ... K = 640 leaves it
    lin('k704_odd_blocks', 256, 64, 704, I3_3),                                 # K / 64 odd: no 16-wave form
    lin('k512_bn128_w16', 1024, 256, 512, W16_128, res=True),                   # N % 128 == 0, K >= 512, M <= 1024: 64x128
    lin('k576_bn128_odd', 1000, 384, 576, W8_64x128_3),                         # M % 64 == 40, K / 64 odd: 8-wave 64x128
    lin('m1088_t128_low', 1088, 256, 512, W16_64),                              # M > 1024 and 34 tiles of 64x128 < 250: 64x64
    lin('m1984_t128_248', 1984, 1024, 512, I3_3),                               # 248 tiles of 64x128: just below the 250 rule
    lin('m2048_t128_256', 2048, 1024, 512, W16_128),                            # 256 tiles of 64x128 (<= 320: 16-wave form)
    lin('m3072_t128_384', 3072, 1024, 512, W8_64x128_3),                        # 384 tiles > 320: 8-wave 64x128
    lin('m2047_t128_tail', 2047, 1024, 576, W8_64x128_3),                       # M % 64 == 63 on the 64x128 tile
    lin('k1984_below_2048', 4096, 1024, 1984, W8_64x128_3),                     # K one block below the 128x128 threshold
    lin('k2048_bm128', 4096, 1024, 2048, W8_128, bias=True),                    # 128x128 ping-pong tile, 256 tiles
    lin('k2112_bm128_tail', 4033, 1024, 2112, W8_128),                          # M % 128 == 65, K one block above 2048
    lin('k2048_bm128_few', 3968, 1024, 2048, W8_64x128_3),                      # 248 tiles of 128x128 < 256: stays 64x128
    lin('f32ep_bf16_in', 300, 128, 256, I3_2, out_f32=True, bias=True),         # f32 output of bf16 operands (f32 epilogue)
    # ---- each condition of the forward envelope broken once: the general register-staged kernel
    lin('k_mod64_40', 257, 129, 40, GEN_BF16),                                  # K % 64 != 0 (and N % 8 != 0)
    lin('k_mod64_320p8', 256, 256, 328, GEN_BF16),                              # K % 64 == 8 next to k448 / k512
    lin('n_mod8', 256, 100, 256, GEN_BF16),                                     # N % 8 != 0
    lin('a_ptr_off1', 256, 256, 256, GEN_BF16, a_off=1),                        # A not 16-byte aligned (offset 1 element)
    lin('a_ptr_off7', 192, 256, 512, GEN_BF16, a_off=7),                        # ... offset 7 elements
    lin('b_ptr_off3', 256, 192, 256, GEN_BF16, b_off=3),                        # B not 16-byte aligned
    lin('c_ptr_off5', 256, 192, 256, GEN_BF16, c_off=5),                        # C not 16-byte aligned
    lin('lda_mod8', 256, 256, 256, GEN_BF16, a_pad=4),                          # strided column view, lda % 8 == 4
    lin('ldb_mod8', 256, 256, 256, GEN_BF16, b_pad=2),                          # ldb % 8 == 2
    lin('lda_aligned_view', 320, 256, 256, I3_2, a_pad=64),                     # strided view that keeps the envelope
    # ---- f32 mode (exact f32 MFMA, register-staged kernel) and the bf16x3 fast path on the same shapes
    lin('f32_fast', 256, 256, 256, GEN_F32_FAST, mode='f32', bias=True, relu=True),
    lin('f32_tails', 257, 129, 40, GEN_F32, mode='f32'),
    lin('f32_misaligned', 256, 256, 256, GEN_F32, mode='f32', a_off=1),
    lin('f32_tile128', 256, 256, 256, 'igemm_kernel<float, 128, 128, false, false, true>', mode='f32', tile=(128, 128)),
    lin('f32_tile128x64', 200, 192, 96, 'igemm_kernel<float, 128, 64, false>', mode='f32', tile=(128, 64)),
    lin('x3_k256', 256, 256, 256, W16_128, mode='x3', bias=True),               # 3K = 768 on split operands
    lin('x3_bn128', 1024, 256, 576, W8_64x128_3, mode='x3'),                    # 3K = 1728: 27 K blocks
    lin('x3_m_tail', 129, 192, 128, I3_3, mode='x3'),
    lin('x3_k_mod64', 257, 129, 40, GEN_X3, mode='x3'),                         # outside the fast envelope: generic x3 kernel
    lin('x3_misaligned', 256, 256, 256, GEN_X3, mode='x3', a_off=1),
    # ---- convolutions (gathered operands)
    conv('fwd_3x3_c64', CONV_FWD, (2, 12, 20, 64, 128, 3, 1, 1, 1), W8_64x128_3, bias=True, relu=True),
    conv('fwd_3x3_s2', CONV_FWD, (2, 17, 15, 128, 64, 3, 2, 1, 1), W16_64),
    conv('dgrad_3x3', CONV_DGRAD, (2, 12, 20, 128, 64, 3, 1, 1, 1), W8_64x128_3),
    conv('dgrad_1x1_s1', CONV_DGRAD, (2, 8, 16, 192, 256, 1, 1, 0, 1), I3_2),
    conv('f32_fwd_3x3', CONV_FWD, (2, 12, 20, 64, 96, 3, 1, 1, 1), GEN_F32, mode='f32'),
    # ---- weight gradients: wgrad4 (128x128 / 256x128 tiles), wgrad3 (64x64), the general kernel; every split-K reduce mode
    wg('wg4_256x256', 256, 256, 4096, WG4),                                     # 256x128 tile
    wg('wg4_384x256', 384, 256, 3000, WG4),                                     # M % 256 != 0: 128x128 tile, K % 64 == 56
    wg('wg4_256x384_rs', 256, 384, 2048, WG4, rowscale=True),
    wg('wg4_128_edge', 128, 256, 2048, WG3),                                    # M == 128 < 256: wgrad3
    wg('wg4_n_mod128', 256, 264, 2048, WG3),                                    # N % 128 == 8: wgrad3
    wg('wg3_bias_fused', 256, 256, 2048, WG3, bias_out=True),                   # fused bias keeps a wgrad4 shape on wgrad3
    wg('wg3_tails', 72, 200, 1000, WG3, bias_out=True, rowscale=True),          # M % 64 == 8, N % 64 == 8, K % 64 == 40
    wg('wg3_empty_slice', 64, 64, 1600, WG3),                                   # 25 K blocks split 6 ways: the last slice is empty
    wg('wg4_split1', 512, 512, 256, WG4),                                       # split factor 1 (4 K blocks)
    wg('wg3_split6', 256, 192, 1536, WG3),                                      # 24 K blocks split 6, 12 tiles
    wg('wg3_split16', 64, 384, 4096, WG3),                                      # split 16 (a multiple of 8)
    wg('wg_stem_like', 64, 128, 100000, WG3, bias_out=True),                    # <= 2 tiles under a long K: up to 512 slices, many empty
    wg('wg_stem_odd', 64, 120, 33000, WG3, rowscale=True),                      # <= 2 tiles, N % 64 == 56
    wg('wg_gen_m_mod8', 100, 128, 1024, GEN_BF16_T, bias_out=True),             # M % 8 != 0: general kernel, bias by colsum
    wg('wg_gen_n_mod8', 128, 100, 1024, GEN_BF16_T),                            # N % 8 != 0
    wg('wg_gen_lda_mod8', 128, 128, 1024, GEN_BF16_T, a_pad=4),                 # lda % 8 != 0
    wg('wg_gen_ldb_mod8', 128, 128, 1024, GEN_BF16_T, b_pad=2),                 # ldb % 8 != 0
    wg('wg_gen_a_off', 128, 128, 1024, GEN_BF16_T, a_off=3, bias_out=True),     # dY not 16-byte aligned
    wg('wg_gen_b_off', 256, 256, 2048, GEN_BF16_T, b_off=1),                    # X not 16-byte aligned (a wgrad4 shape)
    conv('wg4_3x3_single', WGRAD, (2, 16, 16, 128, 256, 3, 1, 1, 1), WG4, rowscale=True),       # 3x3 wgrad4, launched alone (m/n-major order)
    conv('wg3_3x3_c64', WGRAD, (4, 16, 16, 64, 64, 3, 1, 1, 1), WG3, rowscale=True, bias_out=True),   # reduce mode 1 (taps, Ci % 64 == 0)
    conv('wg3_3x3_c32', WGRAD, (2, 16, 16, 32, 64, 3, 1, 1, 1), WG3),          # reduce mode 2 (Ci % 64 != 0)
    conv('wg_gen_wo_12', WGRAD, (2, 12, 12, 64, 64, 3, 1, 1, 1), GEN_BF16_T),  # 64 % Wo != 0: outside wgrad3's conv condition
    wg('f32_wgrad', 96, 160, 3000, GEN_F32_T, mode='f32', rowscale=True, bias_out=True),
]


def by_name(name):
    for c in CASES:
        if c['name'] == name:
            return c
    raise KeyError(name)


# ---- grouped launches (checked with sedt_igemm_describe(grouped=1) / sedt_igemm_group_describe)
# ReduceBatch: one wgrad4 problem (3x3, Ci % 128 == 0: channel-block-major order), one wgrad3 problem with a fused bias, one row-scaled
# problem whose split leaves an empty trailing slice
GROUP_WGRAD = [
    conv('grp_wg4_3x3_cbmajor', WGRAD, (2, 16, 16, 128, 256, 3, 1, 1, 1), 'wgrad4_group_kernel'),
    wg('grp_wg3_bias', 128, 192, 1024, 'wgrad3_group_kernel', bias_out=True),
    wg('grp_wg3_rowscale_empty', 64, 64, 1600, 'wgrad3_group_kernel', rowscale=True),
]
# linear_group: members of different M, N, K
GROUP_LINEAR = [
    ([(704, 256, 256), (300, 128, 512), (77, 64, 64)], {}, 'igemm3_group_kernel<2>'),
    ([(512, 256, 512), (256, 384, 1024)], {}, 'igemm3_group_kernel<3>'),
    ([(1024, 256, 512), (512, 256, 1024)], {'tile': (128, 128)}, 'igemm3_w8_group_kernel<128, 128, 3>'),
    ([(256, 256, 256), (256, 256, 40)], {}, ''),              # one member outside the envelope: one launch each
]


# ---------------------------------------------------------------------------------------------------------------- host-side helpers
def split_plan(M, N, K, sk, bk=64):
    """(K blocks, blocks per slice, slices that receive no K block) of a split-K launch: per = ceil(nkb / sk) as the kernels slice it"""
    nkb = (K + bk - 1) // bk
    per = (nkb + sk - 1) // sk
    used = (nkb + per - 1) // per
    return nkb, per, sk - used


def out_tiles(M, N):
    return ((M + 63) // 64) * ((N + 63) // 64)


_BASE = {'A': 1 << 36, 'B': 2 << 36, 'C': 3 << 36, 'slab': 4 << 36, 'cs': 5 << 36, 'bias': 6 << 36, 'scale': 7 << 36, 'res': 8 << 36}


def fake_args(c, lib_mod, code):
    """the SedtIgemm block ops.py builds for a single-launch bf16 / f32 row, on 256-byte aligned fake addresses plus the row's element
    offsets (the describe path reads only addresses, never memory)"""
    L = lib_mod
    a = L.SedtIgemm()
    es = 2 if c['mode'] == 'bf16' else 4
    a.M, a.N, a.K = c['M'], c['N'], c['K']
    a.KH = a.KW = a.sh = a.sw = a.dh = a.dw = 1
    a.alpha = 1.0
    a.A = _BASE['A'] + c['a_off'] * es
    a.B = _BASE['B'] + c['b_off'] * es
    ep = c['ep']
    if c['op'] == WGRAD:
        B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
        a.lda, a.ldb = Co + c['a_pad'], Ci + c['b_pad']
        a.trans, a.out_f32 = 1, 1
        if not (k == 1 and s == 1 and p == 0):
            a.conv = 1
            a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.KH, a.KW, a.sh, a.sw, a.ph, a.pw, a.dh, a.dw = Hi, Wi, Ci, c['Ho'], c['Wo'], k, k, s, s, p, p, d, d
        sk = L.load().sedt_igemm_splitk(a.M, a.N, a.K, code)
        a.splitk, a.slab, a.C, a.ldc = sk, _BASE['slab'], _BASE['slab'], a.N
        fused = (c['bias_out'] and code == 1 and a.M % 8 == 0 and a.N % 8 == 0 and a.lda % 8 == 0 and a.ldb % 8 == 0
                 and a.A % 16 == 0 and a.B % 16 == 0 and Ci % 8 == 0)
        if fused:
            a.colsum_out = _BASE['cs']
        return a
    if c['op'] == LINEAR:
        a.lda, a.ldb = c['K'] + c['a_pad'], c['K'] + c['b_pad']
    else:
        B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
        plain = k == 1 and s == 1 and p == 0
        if c['op'] == CONV_FWD:
            a.lda, a.ldb = Ci, k * k * Ci
            geo = (Hi, Wi, Ci, c['Ho'], c['Wo'])
        else:
            a.lda, a.ldb = Co, k * k * Co
            geo = (c['Ho'], c['Wo'], Co, Hi, Wi)
            a.transposed = 0 if plain else 1
        if not plain:
            a.conv = 1
            a.Hi, a.Wi, a.Ci, a.Ho, a.Wo = geo
            a.KH, a.KW, a.sh, a.sw, a.ph, a.pw, a.dh, a.dw = k, k, s, s, p, p, d, d
    a.C = _BASE['C'] + c['c_off'] * (4 if ep.get('out_f32') else es)
    a.ldc = c['N']
    a.out_f32 = 1 if ep.get('out_f32') else 0
    if ep.get('bias'):
        a.bias = _BASE['bias']
    if ep.get('scale'):
        a.scale = _BASE['scale']
    if ep.get('res'):
        a.res, a.ldr = _BASE['res'], c['N']
    if ep.get('relu'):
        a.act = L.ACT_RELU
    if ep.get('tile'):
        a.tile_m, a.tile_n = ep['tile']
    return a
