"""GPU: the fused backbone kernels at both sides of their strip / tile edges against a float64 reference, element by element.

Kernels: bneck_kernel (layer1 / layer2 identity blocks, forward and input-gradient chain), bneck0_fwd_kernel, bneck2_fwd_kernel
(csrc/bneck.hip), bneck3_kernel (csrc/bneck3.hip), stem_pool_fwd_kernel / stem_pool_wgrad_kernel (csrc/stem.hip), conv3x3_c64_kernel
(csrc/conv3x3_c64.hip).  The rows are tests/backbone_cases.py; each asserts the dispatch path first (the *_ok envelopes, the entry
point named by lib.launch_log()), then:

  * every output element is finite - the allocator's free memory is NaN-filled before each kernel call (tests/gemm_check.py:
    poison), so an element no kernel wrote fails;
  * sign-bit and argmax bytes equal those of the tensors the kernel wrote, exactly; pooled values are exact given the kernel's own
    un-pooled tile;
  * every element of every stage output of the sampled clips (tests/backbone_cases.py: sample_clips - first, last, middle, both sides
    of workgroup boundaries) within the bound of tests/conv_check.py, the stage's float64 reference reading the kernel's own bf16 output
    of the stage before (a, b from want_ab; gb, ga from want_g) and the kernel's own sign bits as masks;
  * the forms that do not expose their intermediates (sign bits only, no sign bits of y, no-grad, frozen backward, chain_only, the
    layer3 L2 prefetch, the stem without argmax / un-pooled tile) are bit-identical to the form that does.

Inputs: every clip has its own magnitude (x1/16 / x4 alternating, plus an offset), so a halo row or a strip read from the neighbouring
clip fails by a large factor; FrozenBN scales and biases differ per channel, so a shifted channel index shows.  The references run in
float64 on the GPU (unfold + matmul).  The largest error / bound ratio per kernel, form and stage is printed at the end of the module (-s);
measured on MI355X: 0.49-0.50 for every bf16 output of every kernel (the output's own rounding), 0.079 for the stem's f32 weight
gradient.  The module runs in about 11 s.
"""
import zlib
from collections import defaultdict

import pytest
import torch

import backbone_cases as BC
import conv_check as CC
from gemm_check import poison

pytestmark = pytest.mark.gpu

RATIOS = defaultdict(float)
GEOM = {'l1': (1, 256, 64, 16), 'l2': (2, 512, 128, 8), 'l3': (3, 1024, 256, 4)}      # layer, C, P, W
ENTRY = {'l1': 'bneck_fwd', 'l2': 'bneck_fwd', 'l3': 'bneck3_fwd'}


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, ops
    assert torch.cuda.is_available()
    L.load()
    yield L, ops
    if RATIOS:
        print('\nlargest error / bound ratio per kernel, form and stage:')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _clip_gain(B, pattern, flip=False):
    """per-clip (gain, offset) [B, 1]: alternating x1/16 and x4, offsets 0 / 0.5 / 1 ('plain': 1, 0)"""
    b = torch.arange(B)
    if pattern == 'plain':
        return torch.ones(B, 1), torch.zeros(B, 1)
    gain = torch.where((b + int(flip)) % 2 == 1, torch.tensor(4.0), torch.tensor(1.0 / 16))
    return gain.view(B, 1), (0.5 * (b % 3)).view(B, 1).float()


def _act(case, n_per_clip, C, gen, relu=True, flip=False):
    """[B * n_per_clip, C] bf16 on the GPU with the case's per-clip magnitudes (>= 0 when relu: a block input is a ReLU output)"""
    gain, off = _clip_gain(case.B, case.pattern, flip)
    t = torch.randn(case.B, n_per_clip * C, generator=gen)
    t = (t + off) * gain if relu else t * gain
    if relu:
        t = t.clamp_min(0)
    return t.view(-1, C).cuda().bfloat16()


def _rows(clips, per_clip):
    return torch.cat([torch.arange(c * per_clip, (c + 1) * per_clip) for c in clips])


def _rec(key, r):
    RATIOS[key] = max(RATIOS[key], r)


_LAYERS = {}


def _layer(which):
    """layer `which` of the backbone with seeded weights and per-channel FrozenBN statistics, packed (plan kept alive): the block
    operands {block index: dict} the fused entry points take, and their float64 restatements"""
    if which in _LAYERS:
        return _LAYERS[which]
    from sound_event_detection_transformer_amd import packing
    from sound_event_detection_transformer_amd.lib import BF16
    from sound_event_detection_transformer_amd.sedt.backbone import ResNet50Body
    torch.manual_seed(100 + which)
    body = ResNet50Body(True).cuda()
    layer = {1: body.layer1, 2: body.layer2, 3: body.layer3}[which]
    g = torch.Generator().manual_seed(200 + which)
    with torch.no_grad():
        for b in layer:
            for bn in (b.bn1, b.bn2, b.bn3) + ((b.downsample[1],) if b.downsample is not None else ()):
                n = bn.weight.shape[0]
                bn.weight.copy_(1 + 0.3 * torch.randn(n, generator=g))
                bn.bias.copy_(0.2 * torch.randn(n, generator=g) + 0.05 * torch.arange(n) / n)      # distinct per channel
                bn.running_mean.copy_(0.1 * torch.randn(n, generator=g))
                bn.running_var.copy_(1 + 0.5 * torch.rand(n, generator=g))
    convs, cfr = [], []
    for b in layer[:3]:
        ws = [b.conv1.weight, b.conv2.weight, b.conv3.weight]
        convs += [(b.conv1.weight, b.bn1.tensors()), (b.conv2.weight, b.bn2.tensors()), (b.conv3.weight, b.bn3.tensors())]
        if b.downsample is not None:
            convs.append((b.downsample[0].weight, b.downsample[1].tensors()))
            ws.append(b.downsample[0].weight)
        cfr += ws
    plan = packing.PackPlan(BF16, torch.device('cuda'), convs, [], (), (), cfr)
    blocks = {}
    with plan:
        for i, b in enumerate(layer[:3]):
            ws = [b.conv1.weight, b.conv2.weight, b.conv3.weight] + ([b.downsample[0].weight] if b.downsample is not None else [])
            cf = [packing.lookup_conv_frag(w) for w in ws]
            sb = [tuple(packing.lookup(w)[2:]) for w in ws]
            blocks[i] = dict(cfg=b.cfg, wf=[c[0] for c in cf], wt=[c[1] for c in cf], sb=sb,
                             wq=[CC.q(w.detach()) for w in ws],                                          # forward operands bf16(w)
                             ws=[CC.q(w.detach() * s.view(-1, 1, 1, 1)) for w, (s, _) in zip(ws, sb)])   # dgrad operands bf16(w s)
    torch.cuda.synchronize()
    _LAYERS[which] = (layer, plan, blocks)
    return _LAYERS[which]


# ------------------------------------------------------------------------------------------------ identity Bottlenecks (l1 / l2 / l3)
@pytest.mark.parametrize('case', BC.BY_FAM['l1'] + BC.BY_FAM['l2'] + BC.BY_FAM['l3'], ids=lambda c: c.name)
def test_identity_bottleneck(env, case):
    L, ops = env
    which, C, P, W = GEOM[case.fam]
    B, H = case.B, case.H
    _, _, blocks = _layer(which)
    blk = blocks[1]
    # ---- dispatch: layer1 / layer2 always on bneck_kernel; layer3 on bneck3_kernel inside the window only (called directly either way)
    if case.fam == 'l3':
        assert ops.bneck_ok(ops.BF16, blk['cfg'], W, B, H) == (case.path == 'bneck3'), case
    else:
        assert case.path == 'bneck' and ops.bneck_ok(ops.BF16, blk['cfg'], W)
    gen = _gen(case.name)
    x = _act(case, H * W, C, gen)
    gy = _act(case, H * W, C, gen, relu=False, flip=True)
    wf, wt, sb = blk['wf'], blk['wt'], blk['sb']
    nxt = blocks[2]['wf'] if case.fam == 'l3' else None

    def fwd(**kw):
        poison()
        with L.launch_log() as log:
            r = ops.bneck_fwd(x, B, H, W, wf, sb, **kw)
            torch.cuda.synchronize()
        assert log[ENTRY[case.fam]] == 1 and sum(log.values()) == 1, dict(log)
        return r

    y, a, b, bits, abits, bbits = fwd(want_ab=True)
    # sign bits: exactly those of the tensors written
    assert torch.equal(bits, CC.bits_of(y)) and torch.equal(abits, CC.bits_of(a)) and torch.equal(bbits, CC.bits_of(b))
    # forms without the intermediates: bit-identical
    y1, a1, b1, bits1, ab1, bb1 = fwd()
    assert a1 is None and torch.equal(y1, y) and torch.equal(bits1, bits) and torch.equal(ab1, abits) and torch.equal(bb1, bbits)
    y2, _, _, bits2, ab2, bb2 = fwd(want_bits=False)
    assert bits2 is None and torch.equal(y2, y) and torch.equal(ab2, abits) and torch.equal(bb2, bbits)
    y3, a3, _, bits3, ab3, _ = fwd(train=False)
    assert a3 is None and bits3 is None and ab3 is None and torch.equal(y3, y)
    if nxt is not None:
        y4, a4, b4, bits4, ab4, bb4 = fwd(want_ab=True, nxt=nxt)
        assert all(torch.equal(u, v) for u, v in ((y4, y), (a4, a), (b4, b), (bits4, bits), (ab4, abits), (bb4, bbits)))

    # ---- float64 reference of the sampled clips, stage-conditioned
    clips = BC.sample_clips(case.fam, B, H)
    rows = _rows(clips, H * W)
    rc = rows.cuda()
    n = len(clips)
    X = CC.nchw(x[rc], n, H, W)
    A, Bt = CC.nchw(a[rc], n, H, W), CC.nchw(b[rc], n, H, W)
    w1, w2, w3 = blk['wq']
    ref = CC.bottleneck(X, w1, w2, w3, sb, A=A, Bt=Bt)
    for st, got, K in (('a', a, C), ('b', b, 9 * P), ('y', y, P)):
        v, ab = ref[st]
        _rec(f'{case.fam} fwd {st}', CC.bound_check(got, CC.tok(v).cpu(), CC.tok(ab).cpu(), K, rows=rows, what=f'{case.name} {st}'))

    # ---- input-gradient chain: gy masked by [y > 0] (the consumer's promise), masks = the kernel's own sign bits
    gym = gy * (y > 0)
    xbits = CC.bits_of(x)

    def bwd(xb=xbits, **kw):
        poison()
        with L.launch_log() as log:
            r = ops.bneck_bwd(gym, B, H, W, wt, abits, bbits, xb, **kw)
            torch.cuda.synchronize()
        assert log['bneck3_bwd' if case.fam == 'l3' else 'bneck_bwd'] == 1 and sum(log.values()) == 1, dict(log)
        return r

    gx, gb, ga = bwd(want_g=True)
    gx1, gb1, ga1 = bwd()
    assert gb1 is None and ga1 is None and torch.equal(gx1, gx)            # frozen layer1: no intermediate gradients, same gx
    gxn, _, _ = bwd(want_g=True, xb=None)                                    # no input mask
    assert torch.equal(gxn * (x > 0), gx)
    if case.fam == 'l1':
        gxc, gbc, gac = bwd(chain_only=True)                                 # layer1 block 0's chain: stop at ga
        assert gxc is None and gbc is None and torch.equal(gac, ga)
    if nxt is not None:
        gx4, gb4, ga4 = bwd(want_g=True, nxt=blocks[2]['wt'])
        assert torch.equal(gx4, gx) and torch.equal(gb4, gb) and torch.equal(ga4, ga)
    w1s, w2s, w3s = blk['ws']
    GY = CC.nchw(gym[rc], n, H, W)
    GB, GA = CC.nchw(gb[rc], n, H, W), CC.nchw(ga[rc], n, H, W)
    v, ab = CC.conv_t(GY, w3s)
    m = (Bt > 0).double()
    _rec(f'{case.fam} bwd gb', CC.bound_check(gb, CC.tok(v * m).cpu(), CC.tok(ab * m).cpu(), C, rows=rows, what=f'{case.name} gb'))
    v, ab = CC.conv_t(GB, w2s, pad=1)
    m = (A > 0).double()
    _rec(f'{case.fam} bwd ga', CC.bound_check(ga, CC.tok(v * m).cpu(), CC.tok(ab * m).cpu(), 9 * P, rows=rows, what=f'{case.name} ga'))
    v, ab = CC.conv_t(GA, w1s)
    v, ab = v + GY, ab + GY.abs()
    _rec(f'{case.fam} bwd gx (no mask)', CC.bound_check(gxn, CC.tok(v).cpu(), CC.tok(ab).cpu(), P, rows=rows, what=f'{case.name} gx'))


# ------------------------------------------------------------------------------------------------ layer1 block 0, layer2 block 0
@pytest.mark.parametrize('case', BC.BY_FAM['b0'] + BC.BY_FAM['b2'], ids=lambda c: c.name)
def test_first_block_forward(env, case):
    L, ops = env
    B, H = case.B, case.H
    s2 = case.fam == 'b2'
    which, Ci, P, C = (2, 256, 128, 512) if s2 else (1, 64, 64, 256)
    _, _, blocks = _layer(which)
    blk = blocks[0]
    assert case.path == ('bneck2' if s2 else 'bneck0')
    assert ops.block_form(ops.BF16, blk['cfg'], 16) == case.path and ops.block_form(ops.BF16, blocks[1]['cfg'], 16 if not s2 else 8) != case.path
    H2, W2 = ((H - 1) // 2 + 1, 8) if s2 else (H, 16)
    gen = _gen(case.name)
    x = _act(case, H * 16, Ci, gen)
    entry = 'bneck2_fwd' if s2 else 'bneck0_fwd'

    def fwd(**kw):
        poison()
        with L.launch_log() as log:
            r = ops.block_fwd(case.path, x, B, H, 16, blk['wf'], blk['sb'], **kw)
            torch.cuda.synchronize()
        assert log[entry] == 1 and sum(log.values()) == 1, dict(log)
        return r

    if s2:
        y, a, b, bits, abits, bbits = fwd()
        assert abits is None and bbits is None
        assert y.shape[0] == B * H2 * 8 and a.shape[0] == B * H * 16 and b.shape[0] == B * H2 * 8
        y1, a1, b1, bits1, _, _ = fwd(want_bits=False)
        assert bits1 is None and torch.equal(y1, y) and torch.equal(a1, a) and torch.equal(b1, b)
        y2, a2, _, bits2, _, _ = fwd(train=False)
        assert a2 is None and bits2 is None and torch.equal(y2, y)
    else:
        y, a, b, bits, abits, bbits = fwd(want_ab=True)
        assert torch.equal(abits, CC.bits_of(a)) and torch.equal(bbits, CC.bits_of(b))
        y1, a1, _, bits1, ab1, bb1 = fwd()
        assert a1 is None and torch.equal(y1, y) and torch.equal(bits1, bits) and torch.equal(ab1, abits) and torch.equal(bb1, bbits)
        y2, _, _, bits2, ab2, _ = fwd(want_bits=False)
        assert bits2 is None and torch.equal(y2, y) and torch.equal(ab2, abits)
        y3, a3, _, bits3, ab3, _ = fwd(train=False)
        assert a3 is None and bits3 is None and ab3 is None and torch.equal(y3, y)
    assert torch.equal(bits, CC.bits_of(y))

    clips = BC.sample_clips(case.fam, B, H)
    n = len(clips)
    rin, rout = _rows(clips, H * 16), _rows(clips, H2 * W2)
    X = CC.nchw(x[rin.cuda()], n, H, 16)
    A, Bt = CC.nchw(a[rin.cuda()], n, H, 16), CC.nchw(b[rout.cuda()], n, H2, W2)
    w1, w2, w3, wd = blk['wq']
    ref = CC.bottleneck(X, w1, w2, w3, blk['sb'], stride=2 if s2 else 1, skip=wd, A=A, Bt=Bt)
    assert ref['y'][0].shape[2:] == (H2, W2)
    name = case.fam
    for st, got, K, rows in (('a', a, Ci, rin), ('b', b, 9 * P, rout)):
        v, ab = ref[st]
        _rec(f'{name} fwd {st}', CC.bound_check(got, CC.tok(v).cpu(), CC.tok(ab).cpu(), K, rows=rows, what=f'{case.name} {st}'))
    v, ab = ref['y']
    extra = CC.U_BF16 * CC.tok(ref['i'][0]).abs().cpu()                   # the kernel adds bf16(sd acc + bd)
    _rec(f'{name} fwd y', CC.bound_check(y, CC.tok(v).cpu(), CC.tok(ab).cpu(), max(P, Ci), extra=extra, rows=rout,
                                         what=f'{case.name} y'))


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize('case', BC.BY_FAM['stem'], ids=lambda c: c.name)
def test_stem_pool(env, case):
    import torch.nn.functional as F
    L, ops = env
    B, H, W = case.B, case.H, 64
    assert case.path == 'stem' and ops.stem_pool_ok(ops.BF16, W)
    gen = _gen(case.name)
    gain, off = _clip_gain(B, case.pattern)
    x = ((torch.randn(B, H * W, generator=gen) + off) * gain).view(B, H, W).cuda().contiguous()
    w0, b0 = 0.5 * torch.randn(3, 1, 1, 1, generator=gen), 0.5 * torch.randn(3, generator=gen)
    w1 = torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5
    sc = (0.5 + torch.rand(64, generator=gen)).cuda()
    bi = (0.1 * torch.randn(64, generator=gen) + 0.05 * torch.arange(64) / 64).cuda()
    wcat = ops.stem_prep(ops.BF16, w0.cuda(), b0.cuda(), w1.cuda())
    Ho = (H - 1) // 2 + 1
    Hp = (Ho - 1) // 2 + 1

    def fwd(**kw):
        poison()
        with L.launch_log() as log:
            r = ops.stem_pool_fwd(x, wcat, sc, bi, B, H, W, **kw)
            torch.cuda.synchronize()
        assert log['stem_pool_fwd'] == 1 and sum(log.values()) == 1, dict(log)
        return r

    pool, idx, Hp_, Wp, s1 = fwd(want_s1=True)
    assert (Hp_, Wp) == (Hp, 16) and pool.shape == (B * Hp * 16, 64) and s1.shape == (B * Ho * 32, 64)
    assert torch.isfinite(s1.float()).all() and torch.isfinite(pool.float()).all()
    p1, i1, _, _ = fwd()
    p2, i2, _, _ = fwd(want_idx=False)
    assert torch.equal(p1, pool) and torch.equal(i1, idx) and i2 is None and torch.equal(p2, pool)
    # pooling: exact given the kernel's own un-pooled tile (every clip)
    pm, code = CC.pool3s2(s1.view(B, Ho, 32, 64))
    assert torch.equal(pool.double().view(B, Hp, 16, 64), pm), f'{case.name}: pooled values'
    assert torch.equal(idx.view(B, Hp, 16, 64), code), f'{case.name}: argmax bytes'

    # un-pooled activation of the sampled clips: relu(sc (wcat . [bf16 patch | in-bounds indicator]) + bi), K = 128 packed taps
    def cols(xs):
        nb = xs.shape[0]
        pt = F.unfold(CC.q(xs).view(nb, 1, H, W), 7, padding=3, stride=2)                            # [nb, 49, Ho*32]
        ib = F.unfold(torch.ones(nb, 1, H, W, dtype=torch.float64, device=xs.device), 7, padding=3, stride=2)
        z = torch.zeros(nb, 15, pt.shape[2], dtype=torch.float64, device=xs.device)
        return torch.cat([pt, z, ib, z], 1)                                                            # [nb, 128, Ho*32]

    wc = wcat.double()
    clips = BC.sample_clips('stem', B, H)
    cl = cols(x[torch.tensor(clips).cuda()])
    acc, ab = torch.matmul(wc, cl), torch.matmul(wc.abs(), cl.abs())                                  # [n, 64, L]
    v = CC.relu(sc.double().view(1, -1, 1) * acc + bi.double().view(1, -1, 1))
    ab = sc.double().abs().view(1, -1, 1) * ab + bi.double().abs().view(1, -1, 1)
    rows = _rows(clips, Ho * 32)
    _rec('stem fwd s1', CC.bound_check(s1, v.transpose(1, 2).reshape(-1, 64).cpu(), ab.transpose(1, 2).reshape(-1, 64).cpu(), 128,
                                       rows=rows, what=f'{case.name} s1'))

    # ---- weight gradient of the folded 7x7 from the pooled gradient: every clip (the slabs sum over all of them)
    ns = L.load().sedt_stem_pool_wgrad_slabs(B, H)
    assert ns == min(B * ((Ho + 3) // 4), 512)
    gy = _act(case, Hp * 16, 64, gen, relu=False, flip=True)
    poison()
    with L.launch_log() as log:
        G = ops.stem_pool_wgrad(x, gy, idx, pool, sc, B, H, W)
        torch.cuda.synchronize()
    assert log['stem_pool_wgrad'] == 1, dict(log)
    gp = (gy.double() * (pool > 0)).view(B, Hp, 16, 64)
    code = idx.view(B, Hp, 16, 64).long()
    hh = torch.arange(Hp, device='cuda').view(1, Hp, 1, 1)
    ww = torch.arange(16, device='cuda').view(1, 1, 16, 1)
    ho, wo = 2 * hh - 1 + code // 3, 2 * ww - 1 + code % 3
    bb = torch.arange(B, device='cuda').view(B, 1, 1, 1).expand_as(code)
    cc = torch.arange(64, device='cuda').view(1, 1, 1, 64).expand_as(code)
    gs = torch.zeros(B, Ho, 32, 64, dtype=torch.float64, device='cuda')
    gs.index_put_((bb.reshape(-1), ho.reshape(-1), wo.reshape(-1), cc.reshape(-1)), gp.reshape(-1), accumulate=True)
    gs = CC.q(gs).view(B, Ho * 32, 64)                                      # rounded to bf16 as the unfused chain stores it
    Gr = torch.zeros(64, 128, dtype=torch.float64, device='cuda')
    Ga = torch.zeros_like(Gr)
    for c0 in range(0, B, 8):
        cl = cols(x[c0:c0 + 8])
        Gr += torch.einsum('bpc,bkp->ck', gs[c0:c0 + 8], cl)
        Ga += torch.einsum('bpc,bkp->ck', gs[c0:c0 + 8].abs(), cl.abs())
    s = sc.double().view(-1, 1)
    _rec('stem wgrad G', CC.bound_check(G, (s * Gr).cpu(), (s.abs() * Ga).cpu(), B * Ho * 32, u_out=0.0, what=f'{case.name} G'))
    assert torch.equal(G[:, 49:64], torch.zeros_like(G[:, 49:64])) and torch.equal(G[:, 113:], torch.zeros_like(G[:, 113:]))


# ------------------------------------------------------------------------------------------------ conv3x3_c64
@pytest.mark.parametrize('case', BC.BY_FAM['c64'], ids=lambda c: c.name)
def test_conv3x3_c64(env, case):
    L, ops = env
    B, H, W, C = case.B, case.H, 16, 64
    gen = _gen(case.name)
    g = ops.ConvGeom(H, W, C, C, 3, 1, 1, 1)
    x = _act(case, H * W, C, gen, relu=False)
    gy = _act(case, H * W, C, gen, relu=False, flip=True)
    msrc = torch.randn(B * H * W, C, generator=gen).cuda().bfloat16()
    w = (torch.randn(C, C, 3, 3, generator=gen) / 24.0).cuda()
    sc = (0.5 + torch.rand(C, generator=gen)).cuda()
    bi = (0.1 * torch.randn(C, generator=gen) + 0.05 * torch.arange(C) / C).cuda()
    wf, wb = ops.pack_conv(ops.BF16, w, sc)
    clips = BC.sample_clips('c64', B, H)
    rows = _rows(clips, H * W)
    rc = rows.cuda()
    n = len(clips)
    X, GY = CC.nchw(x[rc], n, H, W), CC.nchw(gy[rc], n, H, W)
    ws = CC.q(w * sc.view(-1, 1, 1, 1))

    def run(fn, t, **ep):
        out = torch.empty((B * H * W, C), device='cuda', dtype=torch.bfloat16)
        kind, w_ = ('fwd', wf) if fn is ops.conv_fwd else ('dgrad', wb)
        assert ops.conv_form(kind, ops.BF16, t, g, w_, out, ep)[0] == 'direct3x3', (case.name, sorted(ep))
        poison()
        out.fill_(float('nan'))
        with L.launch_log() as log:
            r = fn(ops.BF16, t, B, g, wf if fn is ops.conv_fwd else wb, out=out, **ep)
            torch.cuda.synchronize()
        assert log['conv3x3_c64'] == 1 and sum(log.values()) == 1, dict(log)
        return r

    fwd_ref = CC.conv(X, CC.q(w), 1, 1)
    for form, ep in (('fwd bn relu', dict(scale=sc, bias=bi, act=ops.ACT_RELU)), ('fwd bn', dict(scale=sc, bias=bi)), ('fwd plain', {})):
        y = run(ops.conv_fwd, x, **ep)
        v, ab = CC.affine(fwd_ref, sc, bi) if 'scale' in ep else fwd_ref
        if 'act' in ep:
            v = CC.relu(v)
        _rec(f'c64 {form}', CC.bound_check(y, CC.tok(v).cpu(), CC.tok(ab).cpu(), 576, rows=rows, what=f'{case.name} {form}'))
    d_ref = CC.conv_t(GY, ws, pad=1)
    m = (CC.nchw(msrc[rc], n, H, W) > 0).double()
    for form, ep in (('dgrad mask', dict(mask=msrc, ldm=C)), ('dgrad', {})):
        dx = run(ops.conv_dgrad, gy, **ep)
        v, ab = d_ref
        if ep:
            v, ab = v * m, ab * m
        _rec(f'c64 {form}', CC.bound_check(dx, CC.tok(v).cpu(), CC.tok(ab).cpu(), 576, rows=rows, what=f'{case.name} {form}'))
