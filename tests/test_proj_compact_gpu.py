"""GPU: the input gradient of the stride-2 projections on the coarse grid (ops.proj_dgrad) and the residual map that carries it into
conv1's input gradient (SedtIgemm.rmap), against float64 torch.nn.grad.conv2d_input with the per-element budget of tests/gemm_check.py
(c = 2).  tests/test_proj_compact_cpu.py checks the float64 identities used here without a GPU.

(a) the map on the kernel instances the two conv1 input gradients reach at C2 size - igemm3_kernel<64, 64, 2> with K = 128 (layer2) and
    K = 256 (layer3) - plus two 8-wave instances (tile hints), the f32 epilogue of the bf16x3 mode and the general f32 kernel; map heights
    odd (125 -> 63, 63 -> 32, 7 -> 4) and even (8 -> 4), widths 16 -> 8 and 8 -> 4, 1-bit masks, partial last M tiles, NaN-poisoned outputs.
    Pixels off the coarse grid hold the bits of the same launch without a residual.
(b) StageFn backward of layer2's and layer3's block 0, new path against the developer reference path (ops.PROJ_COMPACT = False, the dense
    transposed gather): every weight gradient bit-identical (none depends on the projection's input gradient), gx of both paths inside
    the float64 budget.  The budget of (b) has one more term than gemm_check's: the projection gradient is itself stored in bf16 before
    it is added, one more rounding of 2^-8 |side| at c = 2.
    Measured on MI355X (B = 8): gx error / bound 0.497 on both paths for both blocks; largest |compact - dense| 0 for layer3's block and
    0.00781 = 2^-7 for layer2's (largest |gx| 2.98): one bf16 ulp of a gx in [1, 2).  Explanation: at B = 8 the compact problem has
    M = 4032 rows, 126 tiles of 64x128 - under the dispatcher's 250-tile threshold - and runs on a 64x64 instance that splits K between two
    teams, the dense one on the 64x128 ping-pong instance: `side` is the same sum in another order, so its last bit may differ.
(c) at C2 shape (B = 64) the launch log shows the projection GEMM with M = B Ho Wo and no transposed strided 1x1 problem; there both forms
    run on the same instance and gx is bit-identical (measured: largest difference 0 for both blocks), as are the weight gradients.

Measured error / bound ratios of (a): 0.49-0.50 for the bf16 instances (the output's own rounding), 0.085 / 0.13 for the f32 epilogue,
0.19 / 0.25 for the general f32 kernel."""
import ctypes as C
import math

import pytest
import torch

import proj_ref as R
from gemm_check import U_ACC, U_BF16, check, nan_buffer, poison, sample_index

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, ops
    assert torch.cuda.is_available()
    L.load()
    prev = L.GEMM_X3
    yield L, ops
    L.GEMM_X3 = prev
    ops.x3_cache_clear()


def _bits(t):
    """uint8 [M, N / 8] sign image of t [M, N] (bit c % 8 of byte c / 8), on t's device"""
    b = (t > 0).view(t.shape[0], -1, 8).to(torch.uint8)
    return (b << torch.arange(8, device=t.device, dtype=torch.uint8)).sum(-1).to(torch.uint8)


# name, mode, (B, Hi, Wi), N, K, tile hint, kernel instance ('' = any LDS-DMA instance of the bf16x3 fast path)
CASES = [
    ('l2_c2size', 'bf16', (64, 125, 16), 256, 128, None, 'igemm3_kernel<64, 64, 2>'),                # the launch of the C2 step itself
    ('l2_partial', 'bf16', (2, 125, 16), 256, 128, None, 'igemm3_kernel<64, 64, 2>'),                # M = 4000: last tile 32 rows
    ('l3_c2size', 'bf16', (64, 63, 8), 512, 256, None, 'igemm3_kernel<64, 64, 2>'),
    ('l3_partial', 'bf16', (2, 63, 8), 512, 256, None, 'igemm3_kernel<64, 64, 2>'),                  # M = 1008: last tile 48 rows
    ('w8_64x128_odd', 'bf16', (3, 7, 8), 256, 128, (64, 128), 'igemm3_w8_kernel<64, 128, 2, 1>'),    # M = 168: last tile 40 rows
    ('w8_128x128_even', 'bf16', (3, 8, 16), 256, 128, (128, 128), 'igemm3_w8_kernel<128, 128, 2, 1>'),
    ('w8_128x128_odd', 'bf16', (5, 7, 8), 128, 192, (128, 128), 'igemm3_w8_kernel<128, 128, 2, 1>'),   # M = 280: last tile 24 rows
    ('f32ep_odd', 'x3', (2, 7, 16), 256, 128, None, ''),
    ('f32ep_even', 'x3', (3, 8, 8), 128, 64, None, ''),                                              # M = 192
    ('gen_f32_odd', 'f32', (2, 7, 16), 64, 64, None, 'igemm_kernel<float'),
    ('gen_f32_even', 'f32', (1, 8, 8), 72, 40, None, 'igemm_kernel<float'),                          # partial tiles both ways
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_residual_map_on_every_instance(env, case, capsys):
    L, ops = env
    name, mode, (B, Hi, Wi), N, K, tile, expect = case
    dt = L.BF16 if mode == 'bf16' else L.F32
    td = torch.bfloat16 if dt == L.BF16 else torch.float32
    L.GEMM_X3 = mode == 'x3'
    ops.x3_cache_clear()
    Ho, Wo = R.out_hw(Hi, Wi, 2, 2)
    M, Mc = B * Hi * Wi, B * Ho * Wo
    g = torch.Generator().manual_seed(M * 7 + N)
    a = torch.randn(M, K, generator=g).to(td)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(td)
    side = torch.randn(Mc, N, generator=g).to(td)
    mbits = _bits(torch.randn(M, N, generator=g))
    ad, wd, sd, md = a.cuda(), w.cuda(), side.cuda(), mbits.cuda()
    kw = dict(mask=md, ldm=md.stride(0), mask_bits=True)
    if tile:
        kw['tile'] = tile
    poison()
    out = nan_buffer(M * N, td).view(M, N)
    with L.launch_log() as log:
        ops.igemm(dt, M, N, K, ad, K, wd, K, out, N, res=sd, ldr=N, res_map=(Hi, Wi, 2, 2), **kw)
        torch.cuda.synchronize()
    keys = [k for k in log if k.startswith('igemm')]
    want = ('igemm_x3:igemm3' if mode == 'x3' else 'igemm:' + expect)
    assert len(keys) == 1 and keys[0].startswith(want), dict(log)
    plain = nan_buffer(M * N, td).view(M, N)
    ops.x3_cache_clear()
    ops.igemm(dt, M, N, K, ad, K, wd, K, plain, N, **kw)             # the same launch without a residual
    torch.cuda.synchronize()
    # float64 reference on sampled rows: both edges of every 64-row tile boundary + seeded ones (all rows of the small cases)
    rows = sample_index(M, 64, seed=M)
    dense = R.scatter_dense(side, B, Hi, Wi, 2)                       # conv2d_input with the identity weight
    keep = ((mbits[rows].long()[:, :, None] >> torch.arange(8)) & 1).reshape(len(rows), N).double()
    a64, w64 = a.double()[rows], w.double()
    ref = (a64 @ w64.t() + dense[rows]) * keep
    ab = (a64.abs() @ w64.abs().t() + dense[rows].abs()) * keep
    ratio = check(out, ref, ab, K + 2, U_BF16 if td == torch.bfloat16 else 0.0, x3=mode == 'x3', rows=rows, what=name)
    # off the coarse grid: bit for bit the launch without a residual; on it the two differ wherever the residual is not masked away
    on = (dense.abs().sum(1) > 0).cuda()
    assert int(on.sum()) == Mc
    it = torch.int16 if td == torch.bfloat16 else torch.int32
    assert torch.equal(out.view(it)[~on], plain.view(it)[~on]), name
    assert not torch.equal(out[on], plain[on]), name
    with capsys.disabled():
        print(f'\n[rmap {name}: {keys[0]}, M {M} (coarse {Mc}) N {N} K {K}] worst error / bound {ratio:.3g}')


def test_entry_points_refuse_what_they_cannot_honour(env):
    L, ops = env
    a = torch.zeros(64, 64, device='cuda', dtype=torch.bfloat16)
    side = torch.zeros(16, 64, device='cuda', dtype=torch.bfloat16)
    lib = L.load()

    def args(**kw):
        return ops.igemm_args(64, 64, 64, a, 64, a, 64, a.clone(), 64, res=side, ldr=64, res_map=(8, 8, 2, 2), **kw)
    bad = args()
    bad.res_mod = 16                                                    # the map and res_mod exclude each other
    assert lib.sedt_igemm(C.byref(bad), L.BF16, None) != 0 and b'rmap' in lib.sedt_last_error()
    bad = args()
    bad.rmap = C.c_int32(7 | 8 << 12 | 2 << 24 | 2 << 28).value          # 64 rows are not a whole number of 7 x 8 images
    assert lib.sedt_igemm(C.byref(bad), L.BF16, None) != 0 and b'whole number of images' in lib.sedt_last_error()
    bad = args()
    bad.trans = 1
    assert lib.sedt_igemm(C.byref(bad), L.BF16, None) != 0 and b'rmap' in lib.sedt_last_error()          # a weight gradient has no pixel rows
    assert lib.sedt_wgrad_group(C.byref(bad), 1, L.BF16, None) != 0 and b'residual map' in lib.sedt_last_error()
    pair = (L.SedtIgemm * 2)(args(), bad)
    assert lib.sedt_igemm_group(pair, 2, L.BF16, None) != 0


def _block0(which, seed):
    """block 0 of layer2 / layer3 as a one-block stage with seeded weights and non-trivial FrozenBN statistics, and its pack plan"""
    from sound_event_detection_transformer_amd import packing
    from sound_event_detection_transformer_amd.lib import BF16
    from sound_event_detection_transformer_amd.sedt.backbone import ResNet50Body
    torch.manual_seed(seed)
    body = ResNet50Body(True).cuda()
    b = {2: body.layer2, 3: body.layer3}[which][0]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in (b.bn1, b.bn2, b.bn3, b.downsample[1]):
            bn.weight.copy_(1 + 0.2 * torch.randn(bn.weight.shape, generator=g))
            bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(bn.bias.shape, generator=g))
            bn.running_var.copy_(1 + 0.3 * torch.rand(bn.bias.shape, generator=g))
    for p in b.parameters():
        p.requires_grad_(True)
    convs = [(b.conv1.weight, b.bn1.tensors()), (b.conv2.weight, b.bn2.tensors()), (b.conv3.weight, b.bn3.tensors()),
             (b.downsample[0].weight, b.downsample[1].tensors())]
    cfr = [b.conv1.weight, b.conv2.weight, b.conv3.weight, b.downsample[0].weight]
    plan = packing.PackPlan(BF16, torch.device('cuda'), convs, [], (), (), cfr)
    return b, plan


def _backward(ops, blk, plan, x, gy, B, H, W, compact, record=None):
    """one forward + backward of the one-block stage; returns (gx, {name: weight gradient}).  record: a list that receives
    (M, N, K, A, B, C, kwargs) of every ops.igemm call of the backward"""
    from sound_event_detection_transformer_amd import functional as Fn
    from sound_event_detection_transformer_amd.lib import BF16
    keep, keep_igemm = ops.PROJ_COMPACT, ops.igemm
    ops.PROJ_COMPACT = compact
    try:
        xin = x.clone().requires_grad_(True)
        for p in blk.parameters():
            p.grad = None
        meta = dict(dt=BF16, B=B, H=H, W=W, blocks=[blk.cfg], mask_input=True, grad_premasked=True, x_bits=_bits(x), holder={})
        with plan:
            y = Fn.StageFn.apply(xin, meta, *blk.tensors())
            if record is not None:
                def spy(dtype, M, N, K, A, lda, Bm, ldb, Cout, ldc, **kw):
                    record.append((M, N, K, A, Bm, Cout, kw))
                    return keep_igemm(dtype, M, N, K, A, lda, Bm, ldb, Cout, ldc, **kw)
                ops.igemm = spy
            y.backward(gy * (y.detach() > 0))
        torch.cuda.synchronize()
        return xin.grad, {n: p.grad.clone() for n, p in blk.named_parameters() if p.grad is not None}
    finally:
        ops.PROJ_COMPACT, ops.igemm = keep, keep_igemm


SHAPES = {2: (125, 16, 256, 128), 3: (63, 8, 512, 256)}       # layer: (H, W, cin, planes) of block 0 at C2's 500 x 64 input


@pytest.mark.parametrize('which', [2, 3])
def test_block0_backward_new_path_against_the_reference_path(env, which, capsys):
    L, ops = env
    L.GEMM_X3 = False
    B = 8
    H, W, cin, pl = SHAPES[which]
    Ho, Wo = R.out_hw(H, W, 2, 2)
    blk, plan = _block0(which, 11 + which)
    g = torch.Generator().manual_seed(100 * which + B)
    x = torch.randn(B * H * W, cin, generator=g).cuda().bfloat16().relu()
    gy = torch.randn(B * Ho * Wo, 4 * pl, generator=g).cuda().bfloat16()
    rec = []
    with L.launch_log() as log:
        gx_new, w_new = _backward(ops, blk, plan, x, gy, B, H, W, True, rec)
    assert log['proj_dgrad:%dx%dx%d' % (B * Ho * Wo, cin, 4 * pl)] == 1 and log['conv_dgrad_gather:k1s2'] == 0, dict(log)
    with L.launch_log() as log:
        gx_ref, w_ref = _backward(ops, blk, plan, x, gy, B, H, W, False)
    assert log['conv_dgrad_gather:k1s2'] == 1 and not any(k.startswith('proj_dgrad') for k in log), dict(log)
    # every weight gradient (conv1, conv2, conv3, the projection) is bit-identical: none of them reads `side`
    assert set(w_new) == set(w_ref) and len(w_new) == 4
    for n in w_new:
        assert torch.equal(w_new[n], w_ref[n]), n
    # the two launches that make gx, as the new path issued them: side_c = gp wdb^T (plain GEMM), gx = (ga w1b^T + side_c on its grid) [x > 0]
    (Mp, Np, Kp, gp, wdb, side_c, kwp), (M1, N1, K1, ga, w1b, out1, kw1) = rec[-2], rec[-1]
    assert (Mp, Np, Kp) == (B * Ho * Wo, cin, 4 * pl) and 'conv' not in kwp and kw1['res'] is side_c and kw1['res_map'] == (H, W, 2, 2)
    assert (M1, N1, K1) == (B * H * W, cin, pl) and torch.equal(out1, gx_new)          # (autograd hands x.grad out as a copy)
    gp64, wd64, ga64, w164 = gp.double().cpu(), wdb.double().cpu().view(cin, 4 * pl), ga.double().cpu(), w1b.double().cpu().view(cin, pl)
    side64 = R.dense_proj_dgrad(gp64, wd64.t().contiguous(), B, H, W, 2)
    side_ab = R.dense_proj_dgrad(gp64.abs(), wd64.abs().t().contiguous(), B, H, W, 2)
    keep = (x > 0).double().cpu()
    ref = (ga64 @ w164.t() + side64) * keep
    Kt = pl + 4 * pl
    # |A||B| of both contractions, and the bf16 rounding of the stored `side` expressed in the accumulation term's units
    ab = (ga64.abs() @ w164.abs().t() + side_ab + side64.abs() * (U_BF16 / (math.sqrt(Kt + 2) * U_ACC))) * keep
    r_new = check(gx_new, ref, ab, Kt + 2, U_BF16, what=f'layer{which} block 0 gx, compact')
    r_ref = check(gx_ref, ref, ab, Kt + 2, U_BF16, what=f'layer{which} block 0 gx, dense reference path')
    diff = float((gx_new.double() - gx_ref.double()).abs().max())
    with capsys.disabled():
        print(f'\n[layer{which} block 0 backward, B = {B}] gx error / bound: compact {r_new:.3g}, dense {r_ref:.3g}; largest |compact - dense| '
              f'{diff:.3g} (largest |gx| {float(gx_ref.abs().max()):.3g}); weight gradients bit-identical')
    # both paths round the same sums to bf16 once: a last-bit difference of `side` (one bf16 ulp, <= 2^-7 |side|) may also move the rounding
    # of the sum it enters by one ulp of gx; anything beyond that would need an explanation
    assert diff <= 2.0 ** -7 * (float(side64.abs().max()) + float(gx_ref.abs().max()))


@pytest.mark.parametrize('which', [2, 3])
def test_c2_shape_launches_the_projection_gemm_on_the_coarse_grid(env, which, capsys):
    L, ops = env
    L.GEMM_X3 = False
    B = 64
    H, W, cin, pl = SHAPES[which]
    Ho, Wo = R.out_hw(H, W, 2, 2)
    blk, plan = _block0(which, 5)
    g = torch.Generator().manual_seed(which)
    x = torch.randn(B * H * W, cin, generator=g).cuda().bfloat16().relu()
    gy = torch.randn(B * Ho * Wo, 4 * pl, generator=g).cuda().bfloat16()
    rec = []
    with L.launch_log() as log:
        gx, w_new = _backward(ops, blk, plan, x, gy, B, H, W, True, rec)
    assert torch.isfinite(gx.float()).all()
    assert log['proj_dgrad:%dx%dx%d' % (B * Ho * Wo, cin, 4 * pl)] == 1, dict(log)                   # M = B Ho Wo: 32256 / 8192
    assert log['conv_dgrad_gather:k1s2'] == 0, dict(log)                                             # no transposed strided 1x1 problem
    assert not any(kw.get('transposed') and kw['conv'][5] == 1 for *_, kw in rec if kw.get('conv') is not None), 'a 1x1 gather was launched'
    assert log['igemm:igemm3_kernel<64, 64, 2>'] >= 1, dict(log)                                     # the consumer's instance
    # ... and the dense reference path at this size: same weight gradients, gx equal up to the last bit of `side`
    with L.launch_log() as log:
        gx_ref, w_ref = _backward(ops, blk, plan, x, gy, B, H, W, False)
    assert log['conv_dgrad_gather:k1s2'] == 1, dict(log)
    assert all(torch.equal(w_new[n], w_ref[n]) for n in w_ref) and set(w_new) == set(w_ref)
    diff, top = float((gx.double() - gx_ref.double()).abs().max()), float(gx_ref.abs().max())
    with capsys.disabled():
        print(f'\n[layer{which} block 0 backward, B = {B}] largest |compact - dense| of gx {diff:.3g} (largest |gx| {top:.3g})')
    assert diff <= 2.0 ** -6 * top
