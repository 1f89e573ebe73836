"""CPU: functional.block_plan and ops.block_form, the one place that decides how a Bottleneck runs, forward and backward.

The library's envelope calls (sedt_bneck*_ok) are host-only, so everything here runs without a GPU.  Every expectation below is written
out by hand from the dispatch rules ("Where a Bottleneck's launch form is chosen"), none is produced by the code under test.

C2 is the benchmark's configuration: B = 64 clips of 500 x 64, so the stages see 125 x 16, 125 x 16 -> 63 x 8, 63 x 8 -> 32 x 4 and 32 x 4.
"""
import pytest


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import _build, lib as L, ops, functional as Fn
    _build.build()
    L.load()
    return L, ops, Fn


@pytest.fixture
def level(env):
    """sets ops.FUSED_BNECK / ops.RELU_BITS for one test"""
    ops = env[1]
    keep = ops.FUSED_BNECK, ops.RELU_BITS

    def set_(fused=5, relu_bits=True):
        ops.FUSED_BNECK, ops.RELU_BITS = fused, relu_bits
    yield set_
    ops.FUSED_BNECK, ops.RELU_BITS = keep


# (cin, planes, stride, dilation, projection) of the 16 Bottlenecks of ResNet-50 with a dilated layer4, and the map each one reads at C2
I1, I2, I3, I4 = (256, 64, 1, 1, False), (512, 128, 1, 1, False), (1024, 256, 1, 1, False), (2048, 512, 1, 2, False)
P1, P2, P3, P4 = (64, 64, 1, 1, True), (256, 128, 2, 1, True), (512, 256, 2, 1, True), (1024, 512, 1, 1, True)
C2 = [  # stage, trainable, [(block, H, W)]
    ('layer1', False, [(P1, 125, 16), (I1, 125, 16), (I1, 125, 16)]),
    ('layer2', True, [(P2, 125, 16), (I2, 63, 8), (I2, 63, 8), (I2, 63, 8)]),
    ('layer3', True, [(P3, 63, 8)] + [(I3, 32, 4)] * 5),
    ('layer4', True, [(P4, 32, 4), (I4, 32, 4), (I4, 32, 4)]),
]
C2_FWD = {'layer1': ['bneck0', 'bneck', 'bneck'], 'layer2': ['bneck2', 'bneck', 'bneck', 'bneck'],
          'layer3': [None] + ['bneck3'] * 5, 'layer4': [None] * 3}
# default backbone: layer1 frozen, layer2..4 train, the stem's conv0 trains (so layer1's input needs a gradient)
C2_BWD = {'layer1': ['chain', 'fused', 'fused'], 'layer2': ['per_op', 'fused', 'fused', 'fused'],
          'layer3': ['per_op'] + ['fused'] * 5, 'layer4': ['per_op'] * 3}


def _plan(env, blk, B, H, W, first=False, mask_input=True, contiguous=True, have_xbits=True, train=True, need_x_grad=True,
          trainable=True, have_frags=True, relu_bits=True, dt=None):
    L, ops, Fn = env
    n = 4 if blk[4] else 3
    w_rg = trainable if isinstance(trainable, (list, tuple)) else [trainable] * n
    return Fn.block_plan(L.BF16 if dt is None else dt, Fn.BlockCfg(*blk), B, H, W, first, mask_input, contiguous, have_xbits, train,
                         need_x_grad, list(w_rg), have_frags, relu_bits)


def _stage_plans(env, B=64, frozen_all=False, relu_bits=True, need_x_grad=True):
    """the plans of the 16 blocks in model order, with the flags sedt/backbone.py hands StageFn: layer1's input comes from the stem without
    sign bits and unmasked; every later block input has its sign bits while RELU_BITS is on"""
    out = {}
    for li, (name, trains, blocks) in enumerate(C2):
        plans = []
        for bi, (blk, H, W) in enumerate(blocks):
            first = bi == 0
            plans.append(_plan(env, blk, B, H, W, first=first, mask_input=li > 0, have_xbits=relu_bits and not (li == 0 and first),
                               need_x_grad=need_x_grad if li == 0 else True, trainable=trains and not frozen_all, relu_bits=relu_bits))
        out[name] = plans
    return out


def test_c2_forward_and_backward_forms(env, level):
    level()
    plans = _stage_plans(env)
    for name, _, blocks in C2:
        assert [p.fwd for p in plans[name]] == C2_FWD[name], name
        assert [p.bwd for p in plans[name]] == C2_BWD[name], name
        assert all(p.want_bits and p.want_gx for p in plans[name])
    # layer1 is frozen: sign bits only, no weight gradient, no intermediate gradient out of the fused chain
    assert all(not p.want_ab and not p.want_g and not any(p.wgrads) for p in plans['layer1'])
    assert [p.mask_x for p in plans['layer1']] == [False, True, True]
    # the trainable stages keep a and b and take every weight gradient; the fused backward hands out gb, ga
    for name in ('layer2', 'layer3', 'layer4'):
        assert all(p.want_ab and p.mask_x and all(p.wgrads) for p in plans[name]), name
        assert [p.want_g for p in plans[name]] == [b == 'fused' for b in C2_BWD[name]]
    assert [len(p.wgrads) for p in plans['layer2']] == [4, 3, 3, 3]
    # the counts the headline dispatch tests assert of one C2 step
    fwd = [p.fwd for ps in plans.values() for p in ps]
    assert (fwd.count('bneck0'), fwd.count('bneck2'), fwd.count('bneck'), fwd.count('bneck3')) == (1, 1, 5, 5)
    bwd = [(p.fwd, p.bwd) for ps in plans.values() for p in ps]
    assert sum(1 for f, b in bwd if b == 'chain' or (b == 'fused' and f == 'bneck')) == 6          # bneck_bwd
    assert bwd.count(('bneck3', 'fused')) == 5                                                      # bneck3_bwd


@pytest.mark.parametrize('lvl,want', [
    (0, [None, None, None, None, None]),
    (1, [None, 'bneck', None, None, None]),
    (2, [None, 'bneck', None, 'bneck', None]),
    (3, ['bneck0', 'bneck', None, 'bneck', None]),
    (4, ['bneck0', 'bneck', 'bneck2', 'bneck', None]),
    (5, ['bneck0', 'bneck', 'bneck2', 'bneck', 'bneck3']),
])
def test_each_fused_bneck_level(env, level, lvl, want):
    L, ops, Fn = env
    level(fused=lvl)
    at = [(P1, 125, 16), (I1, 125, 16), (P2, 125, 16), (I2, 63, 8), (I3, 32, 4)]
    assert [ops.block_form(L.BF16, Fn.BlockCfg(*b), W, 64, H) for b, H, W in at] == want
    assert [_plan(env, b, 64, H, W).fwd for b, H, W in at] == want
    assert [ops.bneck_ok(L.BF16, Fn.BlockCfg(*b), W, 64, H) for b, H, W in at] == [w in ('bneck', 'bneck3') for w in want]
    # the blocks no form takes, at any level
    for b, H, W in [(P3, 63, 8), (P4, 32, 4), (I4, 32, 4)]:
        assert ops.block_form(L.BF16, Fn.BlockCfg(*b), W, 64, H) is None


def test_refusals_take_the_per_op_chain(env, level):
    L, ops, Fn = env
    level()
    for blk, H, W in [(P1, 125, 16), (I1, 125, 16), (P2, 125, 16), (I2, 63, 8), (I3, 32, 4)]:
        assert _plan(env, blk, 64, H, W).fwd is not None
        for kw in (dict(dt=L.F32), dict(have_frags=False), dict(contiguous=False)):
            p = _plan(env, blk, 64, H, W, **kw)
            # per-op both ways, a and b kept, every weight gradient taken
            assert (p.fwd, p.bwd, p.want_ab, p.want_g, all(p.wgrads)) == (None, 'per_op', True, False, True), (blk, kw)
        assert ops.block_form(L.F32, Fn.BlockCfg(*blk), W, 64, H) is None
    # an identity block on another map than its form's
    assert ops.block_form(L.BF16, Fn.BlockCfg(*I1), 8, 64, 125) is None and ops.block_form(L.BF16, Fn.BlockCfg(*I2), 16, 64, 63) is None
    # a dilated or strided twin of an identity block
    assert ops.block_form(L.BF16, Fn.BlockCfg(256, 64, 1, 2, False), 16, 64, 125) is None
    assert ops.block_form(L.BF16, Fn.BlockCfg(256, 64, 2, 1, False), 16, 64, 125) is None


@pytest.mark.parametrize('B,H,want', [(191, 8, None), (192, 8, 'bneck3'), (512, 8, 'bneck3'), (513, 8, None),
                                      (47, 32, None), (48, 32, 'bneck3'), (64, 32, 'bneck3'), (32, 32, None)])
def test_layer3_strip_window(env, level, B, H, want):
    """bneck3 runs while 192 <= B * ceil(H / 8) <= 512"""
    L, ops, Fn = env
    level()
    assert ops.block_form(L.BF16, Fn.BlockCfg(*I3), 4, B, H) == want
    p = _plan(env, I3, B, H, 4)
    assert (p.fwd, p.bwd, p.want_g, p.want_ab) == (want, 'fused' if want else 'per_op', want is not None, True)


def test_relu_bits_off(env, level):
    """no sign bits of any block input: the fused identity forward keeps a and b and the backward is per-op, frozen or not"""
    level(relu_bits=False)
    plans = _stage_plans(env, relu_bits=False)
    assert {n: [p.fwd for p in ps] for n, ps in plans.items()} == C2_FWD
    assert [p.bwd for p in plans['layer1']] == ['chain', 'per_op', 'per_op']
    assert [p.want_ab for p in plans['layer1']] == [False, True, True]
    for name in ('layer2', 'layer3', 'layer4'):
        assert all(p.bwd == 'per_op' and p.want_ab and not p.want_g for p in plans[name]), name
    assert not any(p.want_bits for ps in plans.values() for p in ps)
    # a first identity block whose input gradient is not masked needs no bits: still fused
    p = _plan(env, I1, 64, 125, 16, first=True, mask_input=False, have_xbits=False, trainable=False, relu_bits=False)
    assert (p.fwd, p.bwd, p.want_ab, p.mask_x) == ('bneck', 'fused', False, False)


def test_frozen_backbone(env, level):
    level()
    plans = _stage_plans(env, frozen_all=True)
    assert {n: [p.fwd for p in ps] for n, ps in plans.items()} == C2_FWD
    assert [p.bwd for p in plans['layer1']] == ['chain', 'fused', 'fused']
    assert [p.bwd for p in plans['layer2']] == ['per_op', 'fused', 'fused', 'fused']
    assert [p.bwd for p in plans['layer3']] == ['per_op'] + ['fused'] * 5
    assert [p.bwd for p in plans['layer4']] == ['per_op'] * 3
    for name in ('layer2', 'layer3'):
        assert all(not p.want_ab and not p.want_g for p in plans[name][1:]), name           # identity blocks: sign bits only
        assert plans[name][0].want_ab                                                       # block 0: bneck2 / per-op keep a and b
    assert not any(any(p.wgrads) for ps in plans.values() for p in ps)
    assert all(p.want_gx and p.want_bits for ps in plans.values() for p in ps)


def test_stage_input_without_gradient(env, level):
    level()
    # a frozen first block whose input needs no gradient: nothing to compute, whatever its forward form
    for blk, H, W in [(P1, 125, 16), (P2, 125, 16), (P3, 63, 8), (I1, 125, 16)]:
        p = _plan(env, blk, 64, H, W, first=True, need_x_grad=False, trainable=False)
        assert (p.bwd, p.want_gx, p.want_g, any(p.wgrads)) == ('skip', False, False, False), blk
    assert not _plan(env, P1, 64, 125, 16, first=True, need_x_grad=False, trainable=False).want_ab
    assert _plan(env, P2, 64, 125, 16, first=True, need_x_grad=False, trainable=False).want_ab     # bneck2 has no bit planes: keeps a, b
    # a trainable one: weight gradients only, through the per-op backward, so the fused forward keeps a and b
    for blk, H, W, fwd in [(P1, 125, 16, 'bneck0'), (P2, 125, 16, 'bneck2'), (P3, 63, 8, None), (I1, 125, 16, 'bneck'), (I3, 32, 4, 'bneck3')]:
        p = _plan(env, blk, 64, H, W, first=True, need_x_grad=False, trainable=True)
        assert (p.fwd, p.bwd, p.want_gx, p.want_ab, p.want_g, all(p.wgrads)) == (fwd, 'per_op', False, True, False, True), blk
    # a later block always hands a gradient on
    assert _plan(env, I1, 64, 125, 16, first=False, need_x_grad=False, trainable=False).bwd == 'fused'
    # bneck0: the chain only for a frozen block; one trainable weight is enough for the per-op backward
    p = _plan(env, P1, 64, 125, 16, first=True, mask_input=False, have_xbits=False, trainable=[False, False, False, True])
    assert (p.fwd, p.bwd, p.want_ab, p.wgrads) == ('bneck0', 'per_op', True, (False, False, False, True))
    p = _plan(env, P1, 64, 125, 16, first=True, mask_input=False, have_xbits=False, trainable=False)
    assert (p.fwd, p.bwd, p.want_ab, p.mask_x) == ('bneck0', 'chain', False, False)


def test_no_input_needs_a_gradient(env, level):
    """evaluation / the teacher's pass: no sign bits, no a / b out of a fused forward, nothing to do backward"""
    level()
    for blk, H, W, fwd in [(P1, 125, 16, 'bneck0'), (I1, 125, 16, 'bneck'), (P2, 125, 16, 'bneck2'), (I2, 63, 8, 'bneck'),
                           (I3, 32, 4, 'bneck3')]:
        for first in (True, False):
            p = _plan(env, blk, 64, H, W, first=first, train=False, need_x_grad=False, have_xbits=False)
            assert (p.fwd, p.want_ab, p.want_bits, p.bwd, p.want_g, any(p.wgrads)) == (fwd, False, False, 'skip', False, False), (blk, first)
    p = _plan(env, P3, 64, 63, 8, first=True, train=False, need_x_grad=False, have_xbits=False)
    assert (p.fwd, p.want_bits, p.bwd) == (None, False, 'skip')


def test_conv_frags_list_of_a_default_model(env, monkeypatch):
    """the weights a model's plan lays out fragment-major: the identity blocks of layer1..layer3 in order (three weights each), then the
    four weights of layer1's and of layer2's block 0"""
    from sound_event_detection_transformer_amd import packing
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    got = {}
    monkeypatch.setattr(packing, 'PlanSet', lambda factory: factory())
    monkeypatch.setattr(packing, 'PackPlan', lambda dt, dev, convs, lin, bn_only, frags, cfr: got.setdefault('cfr', cfr))
    model, _, _ = build_model(default_args(enc_layers=3, num_queries=10, dec_at=True))
    model.pack_plan()
    body = model.backbone[0].body
    want = [w for layer in (body.layer1, body.layer2, body.layer3) for b in layer if b.downsample is None
            for w in (b.conv1.weight, b.conv2.weight, b.conv3.weight)]
    for b0 in (body.layer1[0], body.layer2[0]):
        want += [b0.conv1.weight, b0.conv2.weight, b0.conv3.weight, b0.downsample[0].weight]
    assert len(want) == 3 * (2 + 3 + 5) + 8
    assert len(got['cfr']) == len(want) and all(a is b for a, b in zip(got['cfr'], want))
    L, ops, Fn = env
    assert [ops.fusable_form(Fn.BlockCfg(*b)) for b in (P1, I1, P2, I2, P3, I3, P4, I4)] == \
        ['bneck0', 'bneck', 'bneck2', 'bneck', None, 'bneck3', None, None]
