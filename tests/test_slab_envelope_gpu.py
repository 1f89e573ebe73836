"""GPU: the x-stationary slab kernels (csrc/slab.h, csrc/enc_slab.hip, csrc/heads_slab.hip) at their slab edges, element by element
against float64 (tests/slab_check.py: references, bounds and their derivation; tests/slab_cases.py: the rows).

The C entry points are called through lib.load() directly (ops.* allocates its own outputs and gates by SLAB_MIN_WGS); the weights are
packed by packing.PackPlan / lookup_frag, which tests/test_slab_gpu.py::test_pack_frag_layout pins.  Per row: every output and by-product
lives in a NaN-filled buffer with guard elements before and after, which must keep their bits; every element must be finite and within
its bound; the dropped positions of x1 / x2 equal the residual bit for bit, h / gh / g_h1 / g_h2 are exactly zero where their mask is,
the zero patterns of g2 / g1 equal the restated keep masks; a second launch is bit-identical; the inference instance (no by-products)
gives the training instance's qk, v, x2 (encoder) and cls, box, at (heads) bit for bit.  The dropout seeds of every row go through a
device seed word; test_seed_word_* shows that word k + seeds s equals seeds s + k with a null pointer.  Refused calls return
non-zero with sedt_last_error naming the entry point, leave every output's NaN fill untouched and agree with sedt_encoder_slab_ok /
sedt_heads_slab_ok; none of them reaches a launch.  Nothing is skipped and no case is sampled.

The largest error / bound ratio per kernel and output is printed at the end of the module with -s, with the module's run time.  The
table has NOT been recorded on an MI355X yet: copy it here from the first device run (tests/test_slab_check_cpu.py's torch emulations
sit at 0.5 on the bf16 outputs - their own rounding - and below 0.3 on the f32 ones).
"""
import time
from collections import defaultdict

import numpy as np
import pytest
import torch

import slab_cases as SC
import slab_check as K
from gemm_check import nan_buffer

pytestmark = pytest.mark.gpu

RATIOS = defaultdict(float)
T0 = [None]
GUARD = 64            # guard elements before and after every output (a multiple of the kernels' 16-byte vectors)
D = 256


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L
    assert torch.cuda.is_available()
    lib = L.load()
    T0[0] = time.time()
    yield L, lib
    if RATIOS:
        print('\nlargest error / bound ratio per kernel and output:')
        for k in sorted(RATIOS):
            print(f'  {k:32s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - T0[0]:.1f} s')


class Guarded(object):
    """an output of `shape` inside a NaN-filled buffer with GUARD elements before and after"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = nan_buffer(n + 2 * GUARD, dtype)
        self.view = self.buf[GUARD:GUARD + n].view(*shape)
        self.fill = self.bits().clone()

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.element_size() == 2 else torch.int32)

    def assert_guards(self, what):
        b = self.bits()
        same = torch.equal(b[:GUARD], self.fill[:GUARD]) and torch.equal(b[-GUARD:], self.fill[-GUARD:])
        assert same, f'{what}: elements outside the output were written'

    def untouched(self):
        return torch.equal(self.bits(), self.fill)


def _word(v):
    return torch.from_numpy(np.array([v & 0xffffffff], np.uint32).view(np.int32)).cuda()


bf, f32 = torch.bfloat16, torch.float32


# ==================================================================================================== encoder
ENC_OUT = dict(qk=(2 * D, bf), v=(D, bf), xn=(D, bf), xnp=(D, bf), mean=(0, f32), rstd=(0, f32), x2=(D, bf), ctx=(D, bf), x1=(D, bf),
               mean2=(0, f32), rstd2=(0, f32), x1n=(D, bf), g2=(D, bf), gx1=(D, bf), g1=(D, bf), gctx=(D, bf), gx=(D, bf))


def _enc_buffers(B, S, FF):
    M, nsl = B * S, B * ((S + 31) // 32)
    g = {n: Guarded((M, w) if w else (M,), dt) for n, (w, dt) in ENC_OUT.items()}
    g.update(lse=Guarded((B * 8 * S,), f32), h=Guarded((M, FF), bf), gh=Guarded((M, FF), bf), ln_part2=Guarded((nsl, 2 * D), f32),
             ln_part1=Guarded((nsl, 2 * D), f32))
    return g


class EncCase(object):
    """a row's operands on the device and its packed weights"""

    def __init__(self, L, c):
        from sound_event_detection_transformer_amd import packing
        self.c, self.t = c, K.enc_inputs(c)
        t = self.t
        self.t64 = K._dev(t, 'cuda')
        self.act = {n: t[n].to(bf).cuda().contiguous() for n in ('x', 'pos', 'gx2', 'dqk', 'dv')}
        self.par = {n: t[n].float().cuda().contiguous() for n in ('gamma1', 'beta1', 'gamma2', 'beta2', 'b_in', 'b_o', 'b1', 'b2')}
        self.w = {n: torch.nn.Parameter(t[n].float().cuda()) for n in ('w_in', 'w_o', 'w1', 'w2')}
        lin = list(self.w.values())
        self.plan = packing.PackPlan(L.BF16, torch.device('cuda'), [], lin, (), lin)
        with self.plan:
            self.frag = {n: packing.lookup_frag(w) for n, w in self.w.items()}        # (W, W^T) fragment-major
        self.kpm = None if t['kpm'] is None else t['kpm'].to(torch.uint8).cuda().contiguous()
        self.word = _word(t['word'])


def _enc_run(L, lib, ec, g, train=True, seeds=None, seed_ptr='word', S=None, FF=None, p=None, status=False, which=('qkv', 'ffn', 'ffn_bwd', 'qkv_bwd'),
             partial=False):
    """the four launches of a row into the Guarded buffers g; status=True returns the entry points' return values instead of raising"""
    c, a, w, fr = ec.c, ec.act, ec.par, ec.frag
    B = c['B']
    S, FF, p = c['S'] if S is None else S, c['FF'] if FF is None else FF, c['p'] if p is None else p
    seeds = ec.t['seeds'] if seeds is None else seeds
    sp = ec.word if isinstance(seed_ptr, str) else seed_ptr
    P, st = L.p, L.stream_ptr()

    def o(n, on=True):
        return P(g[n].view) if on else None
    res = {}
    if 'qkv' in which:
        res['encoder_qkv_fwd'] = lib.sedt_encoder_qkv_fwd(P(a['x']), P(a['pos']), P(w['gamma1']), P(w['beta1']), P(fr['w_in'][0]), P(w['b_in']), o('qk'),
                                                         o('v'), o('xn', train), o('xnp', train and not partial), o('mean', train),
                                                         o('rstd', train), B, S, None, st)
    if 'ffn' in which:
        res['encoder_attn_ffn_fwd'] = lib.sedt_encoder_attn_ffn_fwd(
            P(a['x']), o('qk'), o('v'), P(ec.kpm), P(fr['w_o'][0]), P(w['b_o']), P(w['gamma2']), P(w['beta2']), P(fr['w1'][0]), P(w['b1']),
            P(fr['w2'][0]), P(w['b2']), o('x2'), o('ctx', train), o('lse', train and not partial), o('x1', train), o('mean2', train),
            o('rstd2', train), o('x1n', train), o('h', train), B, S, FF, p, seeds[0], seeds[1], seeds[2], seeds[3], P(sp), st)
    if 'ffn_bwd' in which:
        res['encoder_ffn_bwd'] = lib.sedt_encoder_ffn_bwd(P(a['gx2']), o('h'), o('x1'), o('mean2'), o('rstd2'), P(w['gamma2']), P(fr['w2'][1]),
                                                         P(fr['w1'][1]), P(fr['w_o'][1]), o('g2'), o('gh'), o('gx1'), o('g1'), o('gctx'),
                                                         o('ln_part2'), B, S, FF, p, seeds[3], seeds[1], P(sp), st)
    if 'qkv_bwd' in which:
        res['encoder_qkv_bwd'] = lib.sedt_encoder_qkv_bwd(P(a['dqk']), P(a['dv']), P(a['x']), o('mean'), o('rstd'), P(w['gamma1']), o('gx1'),
                                                         P(fr['w_in'][1]), o('gx'), o('ln_part1'), B, S, st)
    if status:
        return res
    for n, r in res.items():
        L.check(r, n)
    torch.cuda.synchronize()


@pytest.mark.parametrize('c', SC.ENC, ids=[c['name'] for c in SC.ENC])
def test_encoder_slab_envelope(env, c):
    L, lib = env
    B, S, FF = c['B'], c['S'], c['FF']
    assert lib.sedt_encoder_slab_ok(D, 8, S, FF, L.BF16) == 1
    ec = EncCase(L, c)
    g = _enc_buffers(B, S, FF)
    _enc_run(L, lib, ec, g)
    for n, b in g.items():
        b.assert_guards(f"{c['name']} {n}")
    for k, r in K.check_enc_all(c, ec.t64, {n: b.view for n, b in g.items()}).items():
        RATIOS[k] = max(RATIOS[k], r)
    # a second launch is bit-identical
    g2 = _enc_buffers(B, S, FF)
    _enc_run(L, lib, ec, g2)
    for n in g:
        assert torch.equal(g[n].bits(), g2[n].bits()), f'second run differs in {n}'
    # the inference instances: no by-product is written, qk / v / x2 equal the training instances' bit for bit
    gi = _enc_buffers(B, S, FF)
    _enc_run(L, lib, ec, gi, train=False, which=('qkv', 'ffn'))
    for n in gi:
        if n in ('qk', 'v', 'x2'):
            assert torch.equal(gi[n].bits(), g[n].bits()), f'inference differs from training in {n}'
        else:
            assert gi[n].untouched(), f'the inference instance wrote {n}'


@pytest.mark.parametrize('name', ['enc_b3_s33_ff1536_p0.1_tail_steps', 'enc_b2_s64_ff512_p0.1_key0_steps'])
def test_seed_word_encoder(env, name):
    """seed_ptr -> a device word of value k: the outputs equal those of seeds + k with a null pointer, bit for bit"""
    L, lib = env
    c = next(c for c in SC.ENC if c['name'] == name)
    ec = EncCase(L, c)
    ga, gb = _enc_buffers(c['B'], c['S'], c['FF']), _enc_buffers(c['B'], c['S'], c['FF'])
    k = 0xfffffff3                                            # seeds + k wrap past 2^32
    _enc_run(L, lib, ec, ga, seed_ptr=_word(k))
    _enc_run(L, lib, ec, gb, seeds=tuple((s + k) & 0xffffffff for s in ec.t['seeds']), seed_ptr=None)
    for n in ga:
        assert torch.equal(ga[n].bits(), gb[n].bits()), n
    gc = _enc_buffers(c['B'], c['S'], c['FF'])
    _enc_run(L, lib, ec, gc, seed_ptr=None)                   # (and the word does matter: other masks without it)
    assert not torch.equal(ga['x2'].bits(), gc['x2'].bits()) and not torch.equal(ga['g2'].bits(), gc['g2'].bits())


@pytest.mark.parametrize('r', SC.ENC_REFUSALS, ids=['_'.join(f'{k}{v}' for k, v in r.items()) for r in SC.ENC_REFUSALS])
def test_encoder_refusals(env, r):
    """the buffers are sized for the largest refused shape, so even a refusal that failed to refuse would stay inside them"""
    L, lib = env
    c = dict(name='enc_refusal', B=1, S=129, FF=1024, p=0.1, kpm=None, kind='steps')
    ec = EncCase(L, c)
    g = _enc_buffers(1, 129, 1024)
    S, FF, p = r.get('S', 32), r.get('FF', 512), r.get('p', 0.1)
    if 'S' in r or 'FF' in r:
        assert lib.sedt_encoder_slab_ok(D, 8, S, FF, L.BF16) == 0
        which = ('qkv', 'ffn', 'ffn_bwd', 'qkv_bwd') if 'S' in r else ('ffn', 'ffn_bwd')
    else:
        assert lib.sedt_encoder_slab_ok(D, 8, S, FF, L.BF16) == 1          # (drop_p and the by-product set are the entry points' own checks)
        which = ('ffn', 'ffn_bwd') if 'p' in r else ('qkv', 'ffn')
    for entry in which:
        name = {'qkv': 'encoder_qkv_fwd', 'ffn': 'encoder_attn_ffn_fwd', 'ffn_bwd': 'encoder_ffn_bwd', 'qkv_bwd': 'encoder_qkv_bwd'}[entry]
        res = _enc_run(L, lib, ec, g, S=S, FF=FF, p=p, status=True, which=(entry,), partial=bool(r.get('partial')))
        assert res[name] != 0 and name.encode() in lib.sedt_last_error(), (name, res, lib.sedt_last_error())
    torch.cuda.synchronize()
    for n, b in g.items():
        assert b.untouched(), f'a refused call wrote {n}'


# ==================================================================================================== heads
def _heads_buffers(lib, c, C1=None, CA=None):
    L_, B, Qp = c['L'], c['B'], c['Qp']
    C1, CA = c['C1'] if C1 is None else C1, c['CA'] if CA is None else CA
    R = L_ * B * Qp
    g = dict(cls=Guarded((R, C1), f32), box=Guarded((R, 2), f32), h1=Guarded((R, D), bf), h2=Guarded((R, D), bf), dhs=Guarded((R, D), bf),
             g_h1=Guarded((R, D), bf), g_h2=Guarded((R, D), bf))
    nf = (R + 31) // 32 * (C1 + CA + 2) * 257
    assert lib.sedt_heads_bwd_part_floats(L_, B, Qp, C1, CA) == nf
    g['part'] = Guarded(((R + 31) // 32, (C1 + CA + 2) * 257), f32)
    if CA:
        g['at'] = Guarded((B, CA), f32)
    return g


class HeadsCase(object):
    def __init__(self, L, c):
        from sound_event_detection_transformer_amd import packing
        self.c, self.t = c, K.heads_inputs(c)
        t = self.t
        self.t64 = K._dev(t, 'cuda')
        self.x = t['x'].to(bf).cuda().contiguous()
        self.par = {n: (None if t[n] is None else t[n].float().cuda().contiguous())
                    for n in ('wc', 'bc', 'b1', 'b2', 'w3', 'b3', 'wa', 'ba', 'g_cls', 'g_box', 'g_at')}
        self.w = {n: torch.nn.Parameter(t[n].float().cuda()) for n in ('w1', 'w2')}
        lin = list(self.w.values())
        self.plan = packing.PackPlan(L.BF16, torch.device('cuda'), [], lin, (), lin)
        with self.plan:
            self.frag = {n: packing.lookup_frag(w) for n, w in self.w.items()}


def _heads_run(L, lib, hc, g, train=True, C1=None, CA=None, status=False, which=('fwd', 'bwd'), wa_null=False, h1_only=False):
    c, w, fr = hc.c, hc.par, hc.frag
    C1, CA = c['C1'] if C1 is None else C1, c['CA'] if CA is None else CA
    P, st = L.p, L.stream_ptr()

    def o(n, on=True):
        return P(g[n].view) if (on and n in g) else None
    res = {}
    if 'fwd' in which:
        res['heads_fwd'] = lib.sedt_heads_fwd(P(hc.x), P(w['wc']), P(w['bc']), P(fr['w1'][0]), P(w['b1']), P(fr['w2'][0]), P(w['b2']), P(w['w3']),
                                             P(w['b3']), None if wa_null else P(w['wa']), P(w['ba']), o('cls'), o('box'), o('at'), o('h1', train),
                                             o('h2', train and not h1_only), c['L'], c['B'], c['Qp'], C1, CA, st)
    if 'bwd' in which:
        res['heads_bwd'] = lib.sedt_heads_bwd(P(hc.x), o('h1'), o('h2'), o('box'), o('at'), P(w['g_cls']), P(w['g_box']), P(w['g_at']), P(w['wc']),
                                             P(w['w3']), None if wa_null else P(w['wa']), P(fr['w2'][1]), P(fr['w1'][1]), o('dhs'), o('g_h1'),
                                             o('g_h2'), o('part'), c['L'], c['B'], c['Qp'], C1, CA, st)
    if status:
        return res
    for n, r in res.items():
        L.check(r, n)
    torch.cuda.synchronize()


@pytest.mark.parametrize('c', SC.HEADS, ids=[c['name'] for c in SC.HEADS])
def test_heads_slab_envelope(env, c):
    L, lib = env
    assert lib.sedt_heads_slab_ok(D, c['C1'], c['CA'], L.BF16) == 1
    hc = HeadsCase(L, c)
    g = _heads_buffers(lib, c)
    _heads_run(L, lib, hc, g)
    for n, b in g.items():
        b.assert_guards(f"{c['name']} {n}")
    for k, r in K.check_heads_all(c, hc.t64, {n: b.view for n, b in g.items()}).items():
        RATIOS[k] = max(RATIOS[k], r)
    g2 = _heads_buffers(lib, c)
    _heads_run(L, lib, hc, g2)
    for n in g:
        assert torch.equal(g[n].bits(), g2[n].bits()), f'second run differs in {n}'
    gi = _heads_buffers(lib, c)
    _heads_run(L, lib, hc, gi, train=False, which=('fwd',))
    for n in gi:
        if n in ('cls', 'box', 'at'):
            assert torch.equal(gi[n].bits(), g[n].bits()), f'inference differs from training in {n}'
        else:
            assert gi[n].untouched(), f'the inference call wrote {n}'


@pytest.mark.parametrize('r', SC.HEADS_REFUSALS, ids=['_'.join(f'{k}{v}' for k, v in r.items()) for r in SC.HEADS_REFUSALS])
def test_heads_refusals(env, r):
    """operands and outputs are sized for C1 = CA = 17, so even a refusal that failed to refuse would stay inside them"""
    L, lib = env
    c = dict(name='heads_refusal', L=2, B=2, Qp=11, C1=17, CA=17, g_at=True)
    hc = HeadsCase(L, c)
    g = _heads_buffers(lib, c)
    C1, CA = r.get('C1', 11), r.get('CA', 10)
    if 'C1' in r or 'CA' in r:
        assert lib.sedt_heads_slab_ok(D, C1, CA, L.BF16) == 0
    else:
        assert lib.sedt_heads_slab_ok(D, C1, CA, L.BF16) == 1              # (null operands are the entry points' own checks)
    which = ('fwd',) if r.get('h1_only') else ('fwd', 'bwd')
    for entry in which:
        res = _heads_run(L, lib, hc, g, C1=C1, CA=CA, status=True, which=(entry,), wa_null=bool(r.get('wa_null')), h1_only=bool(r.get('h1_only')))
        name = 'heads_' + entry
        assert res[name] != 0 and name.encode() in lib.sedt_last_error(), (name, res, lib.sedt_last_error())
    torch.cuda.synchronize()
    for n, b in g.items():
        assert b.untouched(), f'a refused call wrote {n}'
