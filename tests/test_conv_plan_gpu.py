"""GPU: the recording path of ops.conv_fwd / ops.conv_dgrad (ops.PROFILE, what bench.py's roofline rows rest on), at the smallest shape
inside the envelope of each special launch form.

A recorded call runs the generic kernel on the whole nine-tap problem and notes the planned form as the entry's hint.  So: (a) its output
equals, bit for bit, that of the un-recorded call with the form's switch off - the same kernel on the same argument block; (b) it records
exactly one entry, the nine-tap problem, hinted with the kind and share of the plan; (c) for the grouped forms the hinted label is the
kernel the un-recorded call launches the builder's blocks on; (d) an exception inside a recorded call leaves nothing behind: the next
recorded linear carries no hint.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = 1
SHARE = {'direct3x3': 1.0, 's2_parity': 0.25, 'dil_halves': 2.0 / 3.0}
LOG_KEY = {'direct3x3': 'conv3x3_c64', 's2_parity': 'igemm_group_s2', 'dil_halves': 'igemm_group_dil'}
# form -> (switch, B, (Hi, Wi, Ci, Co, k, stride, pad, dilation) per kind): layer1's conv2 on a 2 x 16 map; the 7 x 5 stride-2 map of
# tests/test_ops_gpu.py; layer4's 32 x 4 map at dilation 2 and 64 clips, as there (the halves need 96 tiles of 128x128)
FORMS = {'direct3x3': ('CONV3_DIRECT', 1, {'fwd': (2, 16, 64, 64, 3, 1, 1, 1), 'dgrad': (2, 16, 64, 64, 3, 1, 1, 1)}),
         's2_parity': ('S2_PARITY', 1, {'dgrad': (7, 5, 64, 64, 3, 2, 1, 1)}),
         'dil_halves': ('DIL_HALVES', 64, {'fwd': (32, 4, 512, 512, 3, 1, 2, 2), 'dgrad': (32, 4, 512, 512, 3, 1, 2, 2)})}


@pytest.fixture(scope='module')
def ops():
    from sound_event_detection_transformer_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _problem(ops, form, kind):
    _, B, geoms = FORMS[form]
    g = ops.ConvGeom(*geoms[kind])
    gen = torch.Generator().manual_seed(len(form) * 7 + len(kind))
    w = (torch.randn(g.Co, g.Ci, 3, 3, generator=gen) / (9 * g.Ci) ** 0.5).cuda()
    sc, bi = (1 + 0.1 * torch.randn(g.Co, generator=gen)).cuda(), (0.1 * torch.randn(g.Co, generator=gen)).cuda()
    wf, wb = ops.pack_conv(BF16, w, bnscale=sc)
    if kind == 'fwd':
        t = torch.randn(B * g.Hi * g.Wi, g.Ci, generator=gen).cuda().bfloat16()
        return g, B, t, wf, (B * g.Ho * g.Wo, g.Co, 9 * g.Ci), dict(scale=sc, bias=bi, act=ops.ACT_RELU)
    t = torch.randn(B * g.Ho * g.Wo, g.Co, generator=gen).cuda().bfloat16()
    ep = {}
    if form != 'direct3x3':                                  # the 1-bit ReLU mask of the dgrad chain, indexed by the dx pixel
        bits = torch.randint(0, 256, (B * g.Hi * g.Wi, g.Ci // 8), generator=gen, dtype=torch.uint8).cuda()
        ep = dict(mask=bits, ldm=bits.stride(0), mask_bits=True)
    return g, B, t, wb, (B * g.Hi * g.Wi, g.Ci, 9 * g.Co), ep


@pytest.mark.parametrize('form,kind', [(f, k) for f in FORMS for k in FORMS[f][2]])
def test_a_recorded_convolution_runs_the_generic_kernel_and_hints_the_plan(ops, form, kind):
    from sound_event_detection_transformer_amd import lib as L
    g, B, t, w, shape, ep = _problem(ops, form, kind)
    fn = ops.conv_fwd if kind == 'fwd' else ops.conv_dgrad
    out = torch.empty(shape[:2], device='cuda', dtype=torch.bfloat16)
    plan = ops.conv_form(kind, BF16, t, g, w, out, ep)
    assert plan == (form, False, SHARE[form])
    label = None if form == 'direct3x3' else ops._group_label(ops.conv_group_jobs(form, kind, t, B, g, w, out, ep, False))
    with L.launch_log() as log:                              # the un-recorded call launches the planned form, once
        fn(BF16, t, B, g, w, **ep)
    assert log[LOG_KEY[form]] == 1 and log['sedt_igemm'] == 0, dict(log)
    ops.PROFILE = []
    try:
        with L.launch_log() as log:
            recorded = fn(BF16, t, B, g, w, **ep)
        entries = ops.PROFILE
    finally:
        ops.PROFILE = None
    assert log['sedt_igemm'] == 1 and log[LOG_KEY[form]] == 0, dict(log)
    switch = FORMS[form][0]
    keep = getattr(ops, switch)
    setattr(ops, switch, False)
    try:
        assert ops.conv_form(kind, BF16, t, g, w, out, ep) == ('gemm', False, 1.0)
        plain = fn(BF16, t, B, g, w, **ep)
    finally:
        setattr(ops, switch, keep)
    torch.cuda.synchronize()
    assert torch.equal(recorded, plain) and bool(torch.isfinite(plain.float()).all()) and float(plain.float().abs().max()) > 0     # (a)
    assert len(entries) == 1                                                                                                         # (b)
    _, code, recorded_shape, _, hint = entries[0]
    assert code == BF16 and recorded_shape == shape + (0, 1)
    if form == 'direct3x3':
        assert hint == 'conv3x3_c64_kernel'
    else:
        assert label and hint == ('group', label, SHARE[form])                                                                      # (c)


def test_an_exception_inside_a_recorded_call_leaves_no_hint_behind(ops):
    """(d) two recorded calls that raise on the host, before any launch, while a hint is in play: the halves form with a sign-bit output
    of the wrong dtype (igemm_args' assert, met while the hint's blocks are built), the direct form with its output on the host (refused
    inside igemm, after the hint was made)"""
    g, B, t, w, shape, ep = _problem(ops, 'dil_halves', 'fwd')
    g1, B1, t1, w1, shape1, ep1 = _problem(ops, 'direct3x3', 'fwd')
    x = torch.randn(64, 64).cuda().bfloat16()
    ops.PROFILE = []
    try:
        with pytest.raises(AssertionError):
            ops.conv_fwd(BF16, t, B, g, w, bits_out=torch.empty((shape[0], shape[1] // 8), device='cuda', dtype=torch.int32), **ep)
        with pytest.raises(RuntimeError, match='GPU tensors'):
            ops.conv_fwd(BF16, t1, B1, g1, w1, out=torch.empty(shape1[:2], dtype=torch.bfloat16), **ep1)
        assert ops.PROFILE == []
        ops.linear(BF16, x, x)
        entries = ops.PROFILE
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    assert len(entries) == 1 and entries[0][2] == (64, 64, 64, 0, 0) and entries[0][4] is None
