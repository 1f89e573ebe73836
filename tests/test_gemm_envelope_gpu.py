"""GPU: every GEMM kernel instance the dispatcher (sedt_igemm, csrc/igemm.hip) can pick, at both sides of each envelope condition,
against a float64 reference with a per-element error budget (tests/gemm_check.py).

Each row of tests/gemm_cases.py names the kernel instance it must reach; the test asserts that first (lib.launch_log() 'igemm:' keys,
sedt_igemm_describe(grouped=1) / sedt_igemm_group_describe for grouped launches), then every checked element against

    |got - ref| <= c (sqrt(K) 2^-24 (|A||B|)_ij + [bf16x3] 2^-16 (|A||B|)_ij + [bf16 out] 2^-8 |ref_ij|),   c = 2,

with the allocator's free memory and every out= buffer NaN-filled before the call, so that an element no kernel wrote (a skipped tile, a
dropped or empty split-K slice) fails as non-finite.  Large forward problems are checked on sampled rows: both edges of every 64-row
tile boundary plus 64 seeded random rows, all columns.

Instances and the rows that reach them (tests/test_gemm_split_cpu.py resolves the same names on the host):
  igemm3_kernel<64, 64, 1 / 2 / 3>        k64_one_block / k256_*, f32ep_bf16_in, lda_aligned_view, dgrad_1x1_s1 / k448_below_512,
                                          k704_odd_blocks, m1984_t128_248, x3_m_tail
  igemm3_w16_kernel<64, 64, 3>            k512_small16, k640_n64_s3, m1088_t128_low, fwd_3x3_s2
  igemm3_w16_kernel<64, 128, 3>           k512_bn128_w16, m2048_t128_256, x3_k256
  igemm3_w8_kernel<64, 128, 3, 1>         k576_bn128_odd, m3072_t128_384, m2047_t128_tail, k1984_below_2048, k2048_bm128_few,
                                          fwd_3x3_c64, dgrad_3x3, x3_bn128
  igemm3_w8_kernel<128, 128, 3, 1>        k2048_bm128, k2112_bm128_tail
  igemm3_group_kernel<2 / 3>, igemm3_w8_group_kernel<128, 128, 3>   test_linear_group
  igemm3_co_kernel<64, 64, 2>             test_coscheduled_rider (a wgrad problem riding in a forward launch)
  igemm_kernel<__bf16, 64, 64, false>     k_mod64_*, n_mod8, a_ptr_off*, b_ptr_off3, c_ptr_off5, lda_mod8, ldb_mod8
  igemm_kernel<__bf16, 64, 64, true>      wg_gen_* (M % 8, N % 8, lda % 8, ldb % 8, dY / X not 16-byte aligned, 64 % Wo != 0)
  igemm_kernel<float, ...>                f32_* (FAST and general loaders, 64x64 / 128x128 / 128x64 tile hints, trans for f32_wgrad)
  igemm_kernel<float, 64, 64, false, true>  x3_k_mod64, x3_misaligned (bf16x3 outside the fast envelope)
  wgrad4_kernel<3>                        wg4_256x256 (256x128 tile), wg4_384x256 (128x128 tile, empty trailing slice),
                                          wg4_256x384_rs, wg4_split1, wg4_3x3_single (3x3, launched alone: m/n-major order)
  wgrad3_kernel<64>                       wg4_128_edge, wg4_n_mod128, wg3_*, wg_stem_like (390 slices, 77 empty), wg_stem_odd
  wgrad4_group_kernel / wgrad3_group_kernel   test_grouped_wgrad (3x3 Ci % 128 == 0: channel-block-major order; fused bias;
                                          row scale with an empty trailing slice)
  multi_wgrad_reduce_kernel               every wgrad row; reduce modes 0 (1x1), 1 (3x3, Ci % 64 == 0), 2 (Ci % 64 != 0, misaligned),
                                          3 (>= 16 slices), with and without row scale and fused bias sums

Out of scope: paths reachable only through developer switches of the SEDT_DEV build (SEDT_WGRAD4_BIAS, SEDT_IGEMM_BM256,
SEDT_WGRAD_WIDE, SEDT_WGRAD_KSLICE, SEDT_IGEMM_BREG, ...): the product library never reads the environment (csrc/common.h dev_getenv).

Largest error / bound ratio per instance measured on MI355X (printed at the end of the module with -s): 0.49-0.50 for every bf16-output
forward / dgrad instance (the output's own rounding), 0.04-0.09 for the bf16x3 fast path, 0.13-0.27 for the f32-mode general kernel
(0.16 in its bf16x3 form), 0.042 for the general bf16 wgrad, 0.0046 for the f32 wgrad, 0.016 / 0.031 for wgrad3 / wgrad4 and 0.0086 /
0.014 for their grouped forms.  The whole module runs in about 10 s.
"""
import ctypes as C
import math
import zlib
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import gemm_cases as G
from gemm_check import U_BF16, check, nan_buffer, poison, sample_index

pytestmark = pytest.mark.gpu

RATIOS = defaultdict(float)


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, ops
    assert torch.cuda.is_available()
    L.load()
    prev = L.GEMM_X3
    yield L, ops
    L.GEMM_X3 = prev
    ops.x3_cache_clear()
    if RATIOS:
        print('\nlargest error / bound ratio per instance:')
        for k in sorted(RATIOS):
            print(f'  {k:60s} {RATIOS[k]:.3g}')


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _dev_view(t, off, ld, dtype):
    """t [rows, cols] as a device view with row stride ld whose first element sits `off` elements into its allocation"""
    rows, cols = t.shape
    buf = torch.zeros(off + rows * ld, device='cuda', dtype=dtype)
    v = buf[off:].view(rows, ld)[:, :cols]
    v.copy_(t.to(dtype))
    return v


def _record(key, ratio):
    RATIOS[key] = max(RATIOS[key], ratio)


def _instances(log):
    return {k: v for k, v in log.items() if k.startswith('igemm')}


def _run_linear(L, ops, c):
    M, N, K, ep = c['M'], c['N'], c['K'], c['ep']
    dt = L.BF16 if c['mode'] == 'bf16' else L.F32
    td = torch.bfloat16 if dt == L.BF16 else torch.float32
    g = _gen(c['name'])
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    xr, wr = x.to(td).double(), w.to(td).double()
    xd, wd = _dev_view(xr, c['a_off'], K + c['a_pad'], td), _dev_view(wr, c['b_off'], K + c['b_pad'], td)
    kw, extra = {}, []
    if ep.get('bias'):
        b = torch.randn(N, generator=g)
        kw['bias'] = b.cuda()
        extra.append(b.double())
    if ep.get('res'):
        r = torch.randn(M, N, generator=g).to(td)
        kw['res'], kw['ldr'] = r.cuda(), N
    if ep.get('relu'):
        kw['act'] = L.ACT_RELU
    if ep.get('tile'):
        kw['tile'] = ep['tile']
    out_dt = torch.float32 if (ep.get('out_f32') or dt == L.F32) else td
    poison()
    out = nan_buffer(c['c_off'] + M * N, out_dt)[c['c_off']:].view(M, N)
    with L.launch_log() as log:
        ops.linear(dt, xd, wd, out=out, out_f32=bool(ep.get('out_f32')), **kw)
        torch.cuda.synchronize()
    pre = 'igemm_x3:' if (c['mode'] == 'x3' and c['expect'].startswith('igemm3')) else 'igemm:'
    assert _instances(log) == {pre + c['expect']: 1}, dict(log)
    rows = sample_index(M, 64, seed=M)
    ref = xr[rows] @ wr.t()
    ab = xr[rows].abs() @ wr.abs().t()
    if ep.get('bias'):
        ref, ab = ref + extra[0], ab + extra[0].abs()
    if ep.get('res'):
        rr = r.double()[rows]
        ref, ab = ref + rr, ab + rr.abs()
    if ep.get('relu'):
        ref = ref.clamp_min(0)
    u_out = U_BF16 if out_dt == torch.bfloat16 else 0.0
    return check(out, ref, ab, K + 2, u_out, x3=c['mode'] == 'x3', rows=rows, what=c['name'])


def _nchw(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _run_conv(L, ops, c):
    B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
    Ho, Wo = c['Ho'], c['Wo']
    dt = L.BF16 if c['mode'] == 'bf16' else L.F32
    td = torch.bfloat16 if dt == L.BF16 else torch.float32
    g = _gen(c['name'])
    geo = ops.ConvGeom(Hi, Wi, Ci, Co, k, s, p, d)
    assert (geo.Ho, geo.Wo) == (Ho, Wo)
    w = (torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(Ci * k * k)).to(td).double()
    cv = dict(stride=s, padding=p, dilation=d)
    ep = c['ep']
    kw = {}
    if c['op'] == G.CONV_FWD:
        x = torch.randn(B * Hi * Wi, Ci, generator=g).to(td).double()
        wf = w.permute(0, 2, 3, 1).reshape(Co, k * k * Ci)
        xd, wfd = x.to(td).cuda(), wf.to(td).cuda().contiguous()
        ref = _nhwc(F.conv2d(_nchw(x, B, Hi, Wi), w, **cv))
        ab = _nhwc(F.conv2d(_nchw(x, B, Hi, Wi).abs(), w.abs(), **cv))
        if ep.get('bias'):
            b = torch.randn(Co, generator=g)
            kw['bias'] = b.cuda()
            ref, ab = ref + b.double(), ab + b.double().abs()
        if ep.get('relu'):
            kw['act'] = L.ACT_RELU
            ref = ref.clamp_min(0)
        poison()
        out = nan_buffer(B * Ho * Wo * Co, td).view(B * Ho * Wo, Co)
        with L.launch_log() as log:
            ops.conv_fwd(dt, xd, B, geo, wfd, out=out, **kw)
            torch.cuda.synchronize()
        Kc = k * k * Ci
    else:
        dy = torch.randn(B * Ho * Wo, Co, generator=g).to(td).double()
        wb = w.permute(1, 2, 3, 0).reshape(Ci, k * k * Co)
        dyd, wbd = dy.to(td).cuda(), wb.to(td).cuda().contiguous()
        ref = _nhwc(conv2d_input((B, Ci, Hi, Wi), w, _nchw(dy, B, Ho, Wo), **cv))
        ab = _nhwc(conv2d_input((B, Ci, Hi, Wi), w.abs(), _nchw(dy, B, Ho, Wo).abs(), **cv))
        poison()
        out = nan_buffer(B * Hi * Wi * Ci, td).view(B * Hi * Wi, Ci)
        with L.launch_log() as log:
            ops.conv_dgrad(dt, dyd, B, geo, wbd, out=out)
            torch.cuda.synchronize()
        Kc = k * k * Co
    assert _instances(log) == {'igemm:' + c['expect']: 1}, dict(log)
    u_out = U_BF16 if td == torch.bfloat16 else 0.0
    return check(out, ref, ab, Kc + 2, u_out, what=c['name'])


def _wgrad_inputs(c, td):
    """device dY / X (with the row's layout), float64 references of dW [Co, Ci, k, k] and of the bias sums, and the call's kwargs"""
    B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
    Ho, Wo = c['Ho'], c['Wo']
    g = _gen(c['name'])
    dy = torch.randn(B * Ho * Wo, Co, generator=g).to(td).double()
    x = torch.randn(B * Hi * Wi, Ci, generator=g).to(td).double()
    dyd, xd = _dev_view(dy, c['a_off'], Co + c['a_pad'], td), _dev_view(x, c['b_off'], Ci + c['b_pad'], td)
    cv = dict(stride=s, padding=p, dilation=d)
    if k == 1 and s == 1 and p == 0:
        ref, ab = (dy.t() @ x).view(Co, Ci, 1, 1), (dy.abs().t() @ x.abs()).view(Co, Ci, 1, 1)
    else:
        ref = conv2d_weight(_nchw(x, B, Hi, Wi), (Co, Ci, k, k), _nchw(dy, B, Ho, Wo), **cv)
        ab = conv2d_weight(_nchw(x, B, Hi, Wi).abs(), (Co, Ci, k, k), _nchw(dy, B, Ho, Wo).abs(), **cv)
    kw = {}
    if c['rowscale']:
        rs = torch.rand(Co, generator=g) + 0.5
        kw['rowscale'] = rs.cuda()
        ref, ab = ref * rs.double().view(-1, 1, 1, 1), ab * rs.double().view(-1, 1, 1, 1)
    bref = (dy.sum(0), dy.abs().sum(0)) if c['bias_out'] else None
    return dyd, xd, ref.reshape(Co, -1), ab.reshape(Co, -1), bref, kw


def _check_wgrad(c, out, bias, ref, ab, bref, td):
    B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
    K = B * c['Ho'] * c['Wo']
    r = check(out.view(Co, -1), ref, ab, K + 1, 0.0, x3=c['mode'] == 'x3', what=c['name'] + ' dW')
    if bref is not None:
        r = max(r, check(bias, bref[0], bref[1], K, 0.0, what=c['name'] + ' bias'))
    return r


def _run_wgrad(L, ops, c):
    B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
    dt = L.BF16 if c['mode'] == 'bf16' else L.F32
    td = torch.bfloat16 if dt == L.BF16 else torch.float32
    dyd, xd, ref, ab, bref, kw = _wgrad_inputs(c, td)
    geo = ops.ConvGeom(Hi, Wi, Ci, Co, k, s, p, d)
    poison()
    out = nan_buffer(Co * Ci * k * k, torch.float32).view(Co, Ci, k, k)
    bias = nan_buffer(Co, torch.float32) if c['bias_out'] else None
    with L.launch_log() as log:
        ops.wgrad(dt, dyd, xd, B, geo, out=out, bias_out=bias, **kw)
        torch.cuda.synchronize()
    assert _instances(log) == {'igemm:' + c['expect']: 1}, dict(log)
    assert log['wgrad_reduce'] == 1, dict(log)
    return _check_wgrad(c, out, bias, ref, ab, bref, td)


@pytest.mark.parametrize('case', G.CASES, ids=lambda c: c['name'])
def test_envelope_case(env, case):
    L, ops = env
    L.GEMM_X3 = case['mode'] == 'x3'
    ops.x3_cache_clear()
    try:
        run = {G.LINEAR: _run_linear, G.CONV_FWD: _run_conv, G.CONV_DGRAD: _run_conv, G.WGRAD: _run_wgrad}[case['op']]
        _record(case['expect'] + ('' if case['mode'] != 'x3' else ' (bf16x3)'), run(L, ops, case))
    finally:
        L.GEMM_X3 = False
        ops.x3_cache_clear()


def test_grouped_wgrad(env):
    """one ReduceBatch: a wgrad4 problem (3x3, Ci % 128 == 0: channel-block-major tile order), a wgrad3 problem with its bias gradient
    fused, and a row-scaled problem whose split leaves its last K slice empty - one grouped GEMM launch, one reduce launch"""
    L, ops = env
    lib = L.load()
    rb = ops.ReduceBatch()
    outs = []
    for c in G.GROUP_WGRAD:
        B, Hi, Wi, Ci, Co, k, s, p, d = c['geom']
        dyd, xd, ref, ab, bref, kw = _wgrad_inputs(c, torch.bfloat16)
        out = nan_buffer(Co * Ci * k * k, torch.float32).view(Co, Ci, k, k)
        bias = nan_buffer(Co, torch.float32) if c['bias_out'] else None
        ops.wgrad(L.BF16, dyd, xd, B, ops.ConvGeom(Hi, Wi, Ci, Co, k, s, p, d), out=out, bias_out=bias, batch=rb, **kw)
        outs.append((c, out, bias, ref, ab, bref, (dyd, xd, kw)))
    poison()
    rb.collect()                                        # allocates the slabs and builds the argument blocks; launches nothing
    assert len(rb.group) == len(G.GROUP_WGRAD)
    for (a, _, code), c in zip(rb.group, G.GROUP_WGRAD):
        buf = C.create_string_buffer(160)
        assert lib.sedt_igemm_describe(C.byref(a), code, 1, buf, 160) == 0
        assert buf.value.decode() == c['expect'], c['name']
    with L.launch_log() as log:
        rb.flush()
        torch.cuda.synchronize()
    assert log['wgrad_group'] == 1 and log['multi_wgrad_reduce'] == 1 and not _instances(log), dict(log)
    for c, out, bias, ref, ab, bref, _ in outs:
        _record(c['expect'], _check_wgrad(c, out, bias, ref, ab, bref, torch.bfloat16))


@pytest.mark.parametrize('shapes,kw,expect', G.GROUP_LINEAR, ids=[e or 'fallback' for _, _, e in G.GROUP_LINEAR])
def test_linear_group(env, shapes, kw, expect):
    L, ops = env
    lib = L.load()
    items, refs = [], []
    for i, (M, N, K) in enumerate(shapes):
        g = _gen(f'group{M}x{N}x{K}')
        x = torch.randn(M, K, generator=g).bfloat16().double()
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16().double()
        out = nan_buffer(M * N, torch.bfloat16).view(M, N)
        items.append((x.bfloat16().cuda(), w.bfloat16().cuda(), dict(out=out, **kw)))
        rows = sample_index(M, 64, seed=M)
        refs.append((rows, x[rows] @ w.t(), x[rows].abs() @ w.abs().t(), K))
    args = [ops.igemm_args(x.shape[0], w.shape[0], x.shape[1], x, x.stride(0), w, w.stride(0), o['out'], o['out'].stride(0), **kw)
            for x, w, o in items]
    arr = (L.SedtIgemm * len(args))(*args)
    buf = C.create_string_buffer(160)
    assert lib.sedt_igemm_group_describe(arr, len(args), L.BF16, buf, 160) == 0
    assert buf.value.decode() == expect
    poison()
    with L.launch_log() as log:
        outs = ops.linear_group(L.BF16, items)
        torch.cuda.synchronize()
    assert log['igemm_group'] == 1, dict(log)
    for out, (rows, ref, ab, K), (M, N, K_) in zip(outs, refs, shapes):
        _record(expect or 'igemm_group fallback', check(out, ref, ab, K, U_BF16, rows=rows, what=f'group member {M}x{N}x{K_}'))


def test_coscheduled_rider(env):
    """igemm3_co_kernel: inside ops.coschedule() a layer's weight gradient waits in the pool and rides in the spare workgroups of the
    next forward launch of the 64x64 2-stage configuration; both results against float64"""
    L, ops = env
    wc = G.wg('co_rider', 64, 192, 1600, G.WG3, rowscale=True)       # (25 K blocks split 6 ways: an empty trailing slice as well)
    dyd, xd, wref, wab, _, wkw = _wgrad_inputs(wc, torch.bfloat16)
    g = _gen('co_main')
    M, N, K = 256, 256, 256
    x = torch.randn(M, K, generator=g).bfloat16().double()
    w = (torch.randn(N, K, generator=g) / 16).bfloat16().double()
    xg, wgt = x.bfloat16().cuda(), w.bfloat16().cuda()
    poison()
    dw = nan_buffer(64 * 192, torch.float32).view(64, 192, 1, 1)
    y = nan_buffer(M * N, torch.bfloat16).view(M, N)
    with ops.coschedule(), L.launch_log() as log:
        rb = ops.ReduceBatch()
        ops.wgrad(L.BF16, dyd, xd, 1600, ops.ConvGeom(1, 1, 192, 64), out=dw, batch=rb, **wkw)
        rb.flush()
        assert ops.POOL.gemms, 'the wgrad did not wait in the pool'
        ops.linear(L.BF16, xg, wgt, out=y)
        assert not ops.POOL.gemms, 'the forward launch did not take its rider'
    torch.cuda.synchronize()
    assert log['sedt_igemm_co'] == 1 and log['wgrad_group'] == 0, dict(log)
    r = check(y, x @ w.t(), x.abs() @ w.abs().t(), K, U_BF16, what='co main')
    r = max(r, check(dw.view(64, -1), wref, wab, 1601, 0.0, what='co rider'))
    _record('igemm3_co_kernel<64, 64, 2>', r)
