"""The dispatch sweep behind tests/golden/g22_gemm_dispatch.npz: some 27 000 GEMM argument blocks that straddle every threshold of the
host-side planning rules (csrc/igemm3.hip: envelope, tile, ring depth, program; csrc/wgrad3.hip / wgrad4.hip; sedt_igemm_splitk), each
resolved with sedt_igemm_describe / sedt_igemm_group_describe - on the CPU, on fake addresses, nothing is launched.

answers(L) returns one string per problem, in a fixed order:
  forward / dgrad problem     '<status>:<label>'
  weight gradient             '<status>:<label>|<status>:<label of grouped=1>|sk<split factor>'
  group of linears            '<status>:<label>'          ('' = the members run one launch each)
tests/golden/make_golden_dispatch.py stores them for the library of one commit; tests/test_gemm_split_cpu.py compares the current
library with that record, so a refactor of the planner cannot move a single problem to another kernel instance unnoticed.
"""
import ctypes as C
import random

import gemm_cases as G

CODE = {'f32': 0, 'bf16': 1, 'x3': 2}

# ---- linears: K around 64 (one tile), 320 (ring depth), 512 (64x128 tile, 16-wave forms), 576 (the N <= 64 depth exception), 2048 (128x128)
LIN_K = [40, 64, 128, 256, 320, 328, 448, 512, 576, 640, 704, 1024, 1984, 2048, 2112]
# N: multiples and non-multiples of 64 and 128 (100: not even a multiple of 8)
LIN_N = [64, 72, 100, 120, 128, 192, 256, 264, 384, 512, 1024, 2048]
# M: <= 1024 versus above; with N = 1024 / 256 the 64x128 tile counts 248, 256, 320, 328 / 250, 320, 322; 64x64 tile counts 320 / 336 at
# N = 1024 (M = 1280 / 1344); 128x128 tile counts 248 / 256 (M = 3968 / 4096)
LIN_M = [40, 64, 129, 200, 512, 1000, 1024, 1088, 1280, 1344, 1984, 2047, 2048, 2560, 2624, 3072, 3968, 4033, 4096, 8000, 8192, 10240,
         10304, 16000]
SUB_M, SUB_N, SUB_K = [129, 512, 1024, 2048, 2560, 4096, 8192, 10240], [64, 120, 128, 256, 1024, 2048], [64, 256, 328, 512, 576, 1024, 2048]
VARIANTS = [dict(a_off=1), dict(a_off=8), dict(b_off=3), dict(c_off=5), dict(a_pad=4), dict(a_pad=64), dict(b_pad=2), dict(b_pad=8),
            dict(out_f32=True), dict(out_f32=True, f32ep=True), dict(tile=(128, 128)), dict(tile=(128, 64)), dict(res=True, relu=True),
            dict(bias=True, relu=True), dict(scale=True, bias=True)]
VARIANTS_F32 = [dict(a_off=1), dict(b_pad=2), dict(tile=(128, 128)), dict(tile=(128, 64)), dict(res=True, relu=True), dict(out_f32=True)]

# ---- convolutions: (k, stride, pad, dilation), maps (Hi, Wi) - with 64 % Wo != 0 and Ho * Wo < 64 among the outputs -, channels (Ci, Co)
CONV_KSPD = [(3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2), (1, 2, 0, 1), (7, 2, 3, 1)]
CONV_MAPS = [(16, 16), (12, 12), (8, 4), (32, 2), (20, 12), (17, 15), (4, 16), (31, 8), (64, 4)]
CONV_CH = [(64, 64), (64, 128), (128, 64), (128, 256), (256, 256), (256, 512), (512, 128), (192, 64), (32, 64), (512, 2048)]
CONV_B = [2, 24]

# ---- plain weight gradients: dW [Co, Ci] over `rows` pixels
WG_CO = [64, 72, 128, 192, 256, 264, 384, 512, 1024, 2048]
WG_CI = [64, 100, 128, 200, 256, 264, 384, 512, 1024, 2048]
WG_ROWS = [256, 1000, 1536, 2048, 4096, 12000, 32000, 100000]

# ---- groups of linears (M, N, K): both ring depths, the 64x128 rule's M <= 1024 exception, K = 64, and one shape outside the envelope
GROUP_SHAPES = [(704, 256, 256), (300, 128, 512), (77, 64, 64), (512, 256, 512), (256, 384, 1024), (1024, 256, 512), (512, 256, 1024),
                (2048, 1024, 512), (4096, 1024, 2048), (512, 64, 576), (512, 64, 640), (256, 256, 320), (3968, 256, 512), (64, 2048, 256)]
GROUP_OUTSIDE = (256, 256, 40)


def _label(L, a, code, grouped=0):
    buf = C.create_string_buffer(160)
    r = L.load().sedt_igemm_describe(C.byref(a), code, grouped, buf, 160)
    return '%d:%s' % (r, buf.value.decode() if r == 0 else '')


def _group_label(L, jobs, code=1):
    arr = (L.SedtIgemm * len(jobs))(*jobs)
    buf = C.create_string_buffer(160)
    r = L.load().sedt_igemm_group_describe(arr, len(jobs), code, buf, 160)
    return '%d:%s' % (r, buf.value.decode() if r == 0 else '')


def _lin(L, M, N, K, mode, **kw):
    f32ep = kw.pop('f32ep', False)
    a = G.fake_args(G.lin('s', M, N, K, None, mode=mode, **kw), L, CODE[mode])
    a.f32ep = int(f32ep)
    return a


def _wgrad(L, c, code):
    a = G.fake_args(c, L, code)
    return '%s|%s|sk%d' % (_label(L, a, code), _label(L, a, code, grouped=1), a.splitk)


def _s2_parity_jobs(L, B, Hi, Wi, Ci, Co, x3, ep):
    """the four problems of ops.conv_group_jobs('s2_parity', ...): the stride-2 3x3 input gradient by output parity (omap + btap, awrap on split operands)"""
    Ho, Wo, C3 = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1, (3 * Co if x3 else Co)
    jobs = []
    for ph in (0, 1):
        nh, khs = (Hi + 1 - ph) // 2, ([1] if ph == 0 else [0, 2])
        for pw in (0, 1):
            nw, kws = (Wi + 1 - pw) // 2, ([1] if pw == 0 else [0, 2])
            if nh == 0 or nw == 0:
                continue
            taps = [(kh, kw) for kh in khs for kw in kws]
            a = _lin(L, B * nh * nw, Ci, len(taps) * C3, 'bf16', tile=(64, 64), out_f32=x3, f32ep=x3, **ep)
            a.lda, a.ldb, a.ldc = (2 * Co if x3 else Co), 9 * C3, Ci
            a.conv, a.transposed = 1, 1
            a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.KH, a.KW, a.ph, a.pw = Ho, Wo, C3, nh, nw, len(khs), len(kws), ph, pw
            a.omap, a.o_Hi, a.o_Wi, a.o_sh, a.o_sw, a.o_h0, a.o_w0 = 1, Hi, Wi, 2, 2, ph, pw
            a.btap_on, a.awrap = 1, (Co if x3 else 0)
            for t, (kh, kw) in enumerate(taps):
                a.btap[t] = (kh * 3 + kw) * C3
            jobs.append(a)
    return jobs


def _dil_halves_jobs(L, B, H, d, cin, cout, transposed, x3, ep, tile=(128, 128)):
    """the two problems of ops.conv_group_jobs('dil_halves', ...): a dilated 3x3 convolution on a map of 2 d columns, split by column half"""
    Cg = 3 * cin if x3 else cin
    jobs = []
    for half in (0, 1):
        kw0 = (1 - half) if not transposed else half
        a = _lin(L, B * H * d, cout, 6 * Cg, 'bf16', tile=tile, out_f32=x3, f32ep=x3, **ep)
        a.lda, a.ldb, a.ldc = (2 * cin if x3 else cin), 9 * Cg, cout
        a.conv, a.transposed = 1, int(transposed)
        a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.KH, a.KW, a.ph, a.pw, a.dh, a.dw = H, 2 * d, Cg, H, d, 3, 2, d, (d if transposed else 0), d, d
        a.omap, a.o_Hi, a.o_Wi, a.o_sh, a.o_sw, a.o_h0, a.o_w0 = 1, H, 2 * d, 1, 1, 0, half * d
        a.btap_on, a.awrap = 1, (cin if x3 else 0)
        for kh in range(3):
            for j in range(2):
                a.btap[kh * 2 + j] = (kh * 3 + kw0 + j) * Cg
        jobs.append(a)
    return jobs


def answers(L):
    out = []
    # linears, bf16 and f32
    for mode in ('bf16', 'f32'):
        for M in LIN_M:
            for N in LIN_N:
                for K in LIN_K:
                    out.append(_label(L, _lin(L, M, N, K, mode), CODE[mode]))
    # linear variants: misaligned and padded views, f32 output with and without the f32 epilogue, tile hints, epilogues; the split-bf16 mode
    for M in SUB_M:
        for N in SUB_N:
            for K in SUB_K:
                for kw in VARIANTS:
                    out.append(_label(L, _lin(L, M, N, K, 'bf16', **kw), 1))
                for kw in VARIANTS_F32:
                    out.append(_label(L, _lin(L, M, N, K, 'f32', **kw), 0))
                for kw in ({}, dict(a_off=1)):
                    out.append(_label(L, _lin(L, M, N, K, 'x3', **kw), 2))
    # field combinations of the stride-2 parity and dilated-halves forms: every member alone, then their grouped launch
    for B, Hi, Wi, Ci, Co in [(2, 16, 16, 64, 128), (8, 31, 8, 128, 256), (64, 16, 4, 256, 512), (2, 7, 5, 64, 64), (32, 32, 8, 128, 128)]:
        for x3 in (False, True):
            for ep in ({}, dict(res=True)):
                jobs = _s2_parity_jobs(L, B, Hi, Wi, Ci, Co, x3, ep)
                out += [_label(L, a, 1) for a in jobs] + [_group_label(L, jobs)]
                for a in jobs:                      # the same problems without the tile hint, and without the tap table
                    a.tile_m = a.tile_n = 0
                out += [_label(L, a, 1) for a in jobs] + [_group_label(L, jobs)]
                for a in jobs:
                    a.btap_on = 0
                out += [_label(L, a, 1) for a in jobs]
    for B, H, d, cin, cout in [(64, 16, 2, 512, 512), (32, 16, 2, 512, 512), (64, 16, 2, 256, 384), (2, 8, 1, 64, 128), (64, 16, 4, 128, 1024)]:
        for transposed in (False, True):
            for x3 in (False, True):
                for ep in ({}, dict(bias=True, relu=True)):
                    for tile in ((128, 128), (0, 0), (64, 64)):
                        jobs = _dil_halves_jobs(L, B, H, d, cin, cout, transposed, x3, ep, tile)
                        out += [_label(L, a, 1) for a in jobs] + [_group_label(L, jobs)]
    a = _dil_halves_jobs(L, 64, 16, 2, 512, 512, False, False, {})[0]
    a.KH, a.KW, a.K = 3, 3, 9 * 512                 # nine taps: more than the tap table holds
    out.append(_label(L, a, 1))
    # convolutions: forward, transposed (input gradient) and weight gradient
    for k, s, p, d in CONV_KSPD:
        for Hi, Wi in CONV_MAPS:
            if Hi + 2 * p < d * (k - 1) + 1 or Wi + 2 * p < d * (k - 1) + 1:
                continue
            for Ci, Co in CONV_CH:
                for B in CONV_B:
                    geom = (B, Hi, Wi, Ci, Co, k, s, p, d)
                    for mode in ('bf16', 'f32'):
                        out.append(_label(L, G.fake_args(G.conv('s', G.CONV_FWD, geom, None, mode=mode, bias=True, relu=True), L, CODE[mode]), CODE[mode]))
                        out.append(_label(L, G.fake_args(G.conv('s', G.CONV_DGRAD, geom, None, mode=mode), L, CODE[mode]), CODE[mode]))
                        out.append(_wgrad(L, G.conv('s', G.WGRAD, geom, None, mode=mode), CODE[mode]))
                    if B == CONV_B[0]:
                        out.append(_wgrad(L, G.conv('s', G.WGRAD, geom, None, bias_out=True), 1))
    # plain weight gradients, with and without the fused bias
    for Co in WG_CO:
        for Ci in WG_CI:
            for rows in WG_ROWS:
                for bias_out in (False, True):
                    out.append(_wgrad(L, G.wg('s', Co, Ci, rows, None, bias_out=bias_out), 1))
    for Co, Ci, rows in [(96, 160, 3000), (256, 256, 4096), (64, 128, 100000)]:
        out.append(_wgrad(L, G.wg('s', Co, Ci, rows, None, mode='f32'), 0))
    for kw in (dict(a_pad=4), dict(b_pad=2), dict(a_off=3), dict(b_off=1), dict(a_pad=8), dict(b_pad=8)):
        for Co, Ci in [(128, 128), (256, 256), (512, 384)]:
            out.append(_wgrad(L, G.wg('s', Co, Ci, 2048, None, **kw), 1))
    # groups of linears: every pair, then 2 to 8 members drawn from the list (mixed ring depths included), with the 128x128 tile hint, with
    # one member outside the envelope, and one group of nine
    def member(shape, **kw):
        return _lin(L, *shape, 'bf16', **kw)
    for s0 in GROUP_SHAPES:
        for s1 in GROUP_SHAPES:
            out.append(_group_label(L, [member(s0), member(s1)]))
    rng = random.Random(22)
    for n in range(2, 9):
        for _ in range(300):
            out.append(_group_label(L, [member(rng.choice(GROUP_SHAPES)) for _ in range(n)]))
        for _ in range(40):
            out.append(_group_label(L, [member(rng.choice(GROUP_SHAPES), tile=(128, 128)) for _ in range(n)]))
        for _ in range(10):
            out.append(_group_label(L, [member(rng.choice(GROUP_SHAPES), tile=rng.choice([(128, 128), (0, 0)])) for _ in range(n)]))
    for n in range(2, 9):
        out.append(_group_label(L, [member(GROUP_SHAPES[i]) for i in range(n - 1)] + [member(GROUP_OUTSIDE)]))
    out.append(_group_label(L, [member(GROUP_SHAPES[i]) for i in range(9)]))
    out.append(_group_label(L, [member(GROUP_SHAPES[0]), member(GROUP_SHAPES[1])], code=0))
    return out


def table_instances():
    """every kernel instance tests/gemm_cases.py names: the expect column and both group tables"""
    return ({c['expect'] for c in G.CASES + G.GROUP_WGRAD} | {e for _, _, e in G.GROUP_LINEAR}) - {''}
