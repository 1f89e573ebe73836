"""GPU: the bf16 attention backward (csrc/attn_mfma.hip, attn_bwd_mfma_kernel) at the hand-off between its two phases.  The kernel
walks the score matrix once, a wave per 32 keys (dK, dV), leaves dS as a bf16 LDS image [query tile][key][32 queries], and after one
workgroup barrier a wave per 32 queries forms dQ = dS K from that image.  So dQ is made from what OTHER waves stored, and the waves
change roles: with fewer key tiles than query tiles some waves store nothing and still take a query tile, with fewer query tiles some
store and then have no dQ to form.

Everything goes through sedt_attention_fwd / sedt_attention_bwd (ops.attention_*), and the float64 reference, the bounds (u_p = u_out =
2^-8) and the numpy keep mask are those of tests/attn_check.py, exactly as test_attention_envelope applies them to the backward:
the reference reads the kernel's own o and lse.  dq, dk and dv always sit inside NaN-filled buffers with a guard row above and below
and guard columns on both sides, which must keep their bits, and every element inside must be finite.

  test_wave_roles          (Lq, Lk) over 1 x 4, 4 x 1, 2 x 3, 3 x 2, 1 x 1 (one element, one full tile), 4 x 4 (full and ragged) tiles,
                           p in {0, 0.1, 0.5}; four of the shapes also with the additive mask
  test_single_foreign_wave only one live key per clip (key padding 'one', then key 126 of 127): all of dQ comes from one key tile that
                           one wave stored - the first wave's, then the last wave's
  test_no_stray_access     lengths off the 32-grid: guards untouched, nothing non-finite inside (padded image entries are zeros)
  test_run_to_run          two calls, byte-equal outputs
  test_shape_switch        (128, 128) then (11, 11) back to back on one stream equal the same calls issued alone

Largest error / bound ratio on MI355X (printed per case with -s): dq 0.39, dk 0.44, dv 0.46.  The two-pass kernel this one replaced was
run on the same cases: within every bound, with the same three figures.
"""
import numpy as np
import pytest
import torch

import attn_check as K
from gemm_check import U_BF16, nan_buffer, poison

pytestmark = pytest.mark.gpu

GUARD = 32


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, ops
    assert torch.cuda.is_available()
    L.load()
    poison(64)
    return L, ops


class Out(object):
    """an output [rows, W] bf16 inside a NaN-filled buffer: a guard row above and below, GUARD columns left and right"""

    def __init__(self, rows, W):
        ld = W + 2 * GUARD
        self.buf = nan_buffer((rows + 2) * ld, torch.bfloat16)
        self.view = self.buf.view(rows + 2, ld)[1:rows + 1, GUARD:GUARD + W]
        self.fill = self.buf.view(torch.int16).clone()
        inner = torch.zeros_like(self.fill, dtype=torch.bool)
        inner.view(rows + 2, ld)[1:rows + 1, GUARD:GUARD + W] = True
        self.outer = ~inner

    def bits(self):
        return self.buf.view(torch.int16)

    def assert_guards(self, what):
        changed = (self.bits() != self.fill) & self.outer
        assert not bool(changed.any()), f'{what}: {int(changed.sum())} elements outside the output were written'


def _case(Lq, Lk, p, amask=False, kpm=None, B=2, H=3, tag=''):
    return dict(name=f'onepass_q{Lq}_k{Lk}_p{p}_{"am" if amask else "na"}_{kpm}{tag}', dt='bf16', B=B, H=H, Lq=Lq, Lk=Lk, kpm=kpm,
                amask=amask, p=p, gain=1, layout='packed')


class Problem(object):
    """a case's operands on the device (contiguous [B L, H 32] bf16), the kernel's own forward (o, lse) and the float64 reference"""

    def __init__(self, env, c, live_key=None):
        L, ops = env
        self.c, self.ops, self.dt = c, ops, L.BF16
        B, H, Lq, Lk, p = c['B'], c['H'], c['Lq'], c['Lk'], c['p']
        inp = K.case_inputs(c)
        if live_key is not None:                               # every key but one padded, the same one in every clip
            assert c['kpm'] is None and not c['amask']
            inp['kpm'] = torch.ones(B, Lk, dtype=torch.bool)
            inp['kpm'][:, live_key] = False
        self.inp = inp
        bf = torch.bfloat16
        self.q, self.k, self.v, self.do = (K.rows(inp[n]).to(bf).cuda().contiguous() for n in ('q', 'k', 'v', 'do'))
        self.kw = dict(kpm=None if inp['kpm'] is None else inp['kpm'].to(torch.uint8).cuda(),
                       amask=None if inp['amask'] is None else inp['amask'].cuda().contiguous(), drop_p=p, seed=inp['seed'],
                       seed_ptr=torch.from_numpy(np.array([inp['word']], np.uint32).view(np.int32)).cuda())
        self.o, self.lse = ops.attention_fwd(self.dt, self.q, self.k, self.v, B, H, Lq, Lk, **self.kw)
        want = f"attn_bwd_mfma_kernel<{(Lq + 31) // 32}, {(Lk + 31) // 32}, {'true' if c['amask'] else 'false'}>"
        g = self.outputs()
        inst = ops.attention_instance(self.dt, self.q, self.k, self.v, self.o, Lq, Lk, self.kw['amask'], p, self.do, *(x.view for x in g))
        assert inst == want, f"{c['name']}: the backward would run on {inst!r}, not on {want!r}"

    def outputs(self):
        c = self.c
        return tuple(Out(c['B'] * n, c['H'] * 32) for n in (c['Lq'], c['Lk'], c['Lk']))

    def backward(self, outs=None):
        """one launch into fresh (or the given) guarded buffers, not synchronised"""
        c = self.c
        outs = outs or self.outputs()
        self.ops.attention_bwd(self.dt, self.q, self.k, self.v, self.o, self.do, self.lse, c['B'], c['H'], c['Lq'], c['Lk'],
                               *(x.view for x in outs), **self.kw)
        return outs

    def check(self, outs):
        c, inp = self.c, self.inp
        B, H, Lq, Lk = c['B'], c['H'], c['Lq'], c['Lk']
        torch.cuda.synchronize()
        g64 = {n: inp[n].cuda() for n in ('q', 'k', 'v', 'do')}
        rb = K.attention_bwd_ref(g64['q'], g64['k'], g64['v'], g64['do'], K.heads(self.o, B, H, Lq), self.lse.double(),
                                 None if inp['kpm'] is None else inp['kpm'].cuda(), None if inp['amask'] is None else inp['amask'].double().cuda(),
                                 inp['keep'].cuda(), c['p'], U_BF16, U_BF16)
        ratios = {}
        for g_, n, Ln in zip(outs, ('dq', 'dk', 'dv'), (Lq, Lk, Lk)):
            g_.assert_guards(f"{c['name']} {n}")
            ratios[n] = K.check(K.heads(g_.view, B, H, Ln), rb[n], rb['bound_' + n], f"{c['name']} {n}")
        print(f"\n{c['name']}: error / bound " + ' '.join(f'{n} {r:.3g}' for n, r in ratios.items()))
        return rb


def _equal(a, b, what):
    for x, y, n in zip(a, b, ('dq', 'dk', 'dv')):
        assert torch.equal(x.bits(), y.bits()), f'{what}: {n} differs'


SHAPES = [(11, 128), (128, 11), (33, 96), (96, 33), (1, 1), (32, 32), (128, 128), (97, 127)]
ROLES = [(Lq, Lk, p, False) for Lq, Lk in SHAPES for p in (0.0, 0.1, 0.5)] + \
        [(11, 128, 0.1, True), (96, 33, 0.5, True), (128, 128, 0.0, True), (97, 127, 0.1, True)]


@pytest.mark.parametrize('Lq,Lk,p,am', ROLES, ids=[f'q{a}_k{b}_p{p}_{"am" if m else "na"}' for a, b, p, m in ROLES])
def test_wave_roles(env, Lq, Lk, p, am):
    pr = Problem(env, _case(Lq, Lk, p, am))
    pr.check(pr.backward())


@pytest.mark.parametrize('Lq,Lk,live', [(128, 128, None), (128, 127, 126)], ids=['first_tile', 'last_tile'])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_single_foreign_wave(env, Lq, Lk, live, p):
    """one live key per clip: every query's dQ is that key's row of K times the one dS value that the key's wave stored; the three other
    key tiles of the image hold zeros.  (With a single live key P = 1 and dS = dP - delta is zero but for the rounding of o, so the
    reference is near zero and the bound is that of |dP| + |delta|: what would show here is a wrong or stale tile, not a small error.)"""
    pr = Problem(env, _case(Lq, Lk, p, kpm='one' if live is None else None, B=3, H=2, tag=f'_live{live}'), live_key=live)
    kpm = pr.inp['kpm']
    assert bool(((~kpm).sum(1) == 1).all())
    tiles = set(int((~kpm[b]).nonzero()[0]) // 32 for b in range(kpm.shape[0]))
    assert tiles == ({0} if live is None else {3}), tiles
    pr.check(pr.backward())


@pytest.mark.parametrize('Lq,Lk,p,am', [(97, 127, 0.1, False), (33, 11, 0.5, True), (11, 33, 0.0, False), (1, 65, 0.1, False)],
                         ids=['q97_k127', 'q33_k11_am', 'q11_k33', 'q1_k65'])
def test_no_stray_access(env, Lq, Lk, p, am):
    """lengths off the 32-grid: the padded rows and columns of the dS image feed dQ zeros, not NaN, and nothing outside the Lq / Lk
    rows of the outputs is written"""
    poison(64)
    pr = Problem(env, _case(Lq, Lk, p, am, kpm='tail' if Lk > 9 and not am else None, tag='_stray'))
    outs = pr.backward()
    torch.cuda.synchronize()
    for g_, n in zip(outs, ('dq', 'dk', 'dv')):
        g_.assert_guards(n)
        inner = g_.bits()[~g_.outer]
        assert not bool((inner == g_.fill[~g_.outer]).all()), f'{n}: not written'
        assert bool(torch.isfinite(g_.view.float()).all()), f'{n}: non-finite elements inside the output'
    pr.check(outs)


@pytest.mark.parametrize('Lq,Lk,p', [(128, 128, 0.1), (11, 128, 0.0)])
def test_run_to_run(env, Lq, Lk, p):
    pr = Problem(env, _case(Lq, Lk, p, tag='_rr'))
    a, b = pr.backward(), pr.backward()
    torch.cuda.synchronize()
    _equal(a, b, 'second run')
    pr.check(a)


def test_shape_switch(env):
    """a large instance then a small one with nothing in between: the small one must not see the large one's dS image"""
    big, small = Problem(env, _case(128, 128, 0.1, tag='_sw')), Problem(env, _case(11, 11, 0.1, tag='_sw'))
    torch.cuda.synchronize()
    alone_big = big.backward()
    torch.cuda.synchronize()
    alone_small = small.backward()
    torch.cuda.synchronize()
    ob, os_ = big.outputs(), small.outputs()
    torch.cuda.synchronize()
    big.backward(ob)
    small.backward(os_)
    torch.cuda.synchronize()
    _equal(ob, alone_big, 'back to back, (128, 128)')
    _equal(os_, alone_small, 'back to back, (11, 11)')
    big.check(ob)
    small.check(os_)
