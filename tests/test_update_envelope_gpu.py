"""GPU: the kernels that write the trained weights (csrc/misc.hip: multi_sumsq + sumsq_final, multi_adamw, multi_ema, multi_gather and
the single-tensor sumsq_partial / adamw_clip) at their chunk edges, element by element against float64 (tests/update_check.py:
references, bounds and their derivation; tests/update_cases.py: the rows).

The C entry points are called through lib.load() with SedtChunk tables built here from optim._DT, so that the addresses, the step word
and the guard word are the row's to choose.  A row is one byte image (update_check.Layout): every tensor, partial sum and word sits in
one NaN-filled device buffer at its byte offset from a 16-byte boundary, with 32 guard elements on either side.  Per row: no byte
outside the written tensors changes (guards, read-only operands, words the launch does not own); every element inside is finite and
within its bound (AdamW stage by stage: m' and v' from the inputs and the kernel's own sumsq[0], p' from the kernel's own m' and v');
lr = 0 chunks keep p's bits; gather results equal the one IEEE result bit for bit, ties to even included; a second launch from the same
image is bit-identical; the table in reversed chunk order gives the same bytes and `partial` reversed (a clipped AdamW row, whose
coefficient depends on the order sumsq[0] was added in, is checked against its bounds again instead); a row whose norm is below
max_norm equals the unclipped launch bit for bit.  Then the guard / step / seed words of multi_sumsq (update_cases.GUARD_ROWS), the
update kernels under a raised guard, null words, the refused calls (non-zero, sedt_last_error names the entry point, no byte changes),
the two single-tensor entry points, and - one section, one process - FusedAdamW over a three-segment layout and EMA.update on
misaligned slices.  Nothing is skipped and no case is sampled.

Not exercised: multi_adamw_kernel<false>, which only the developer switch SEDT_ADAMW_NT=0 reaches (the library reads it once per
process); multi_pack, multi_bn_fold and multi_wgrad_reduce have their own tests (tests/test_prep_envelope_gpu.py).

The largest error / bound ratio per kernel and output is printed at the end of the module with -s, with the module's run time.
The table has NOT been recorded on an MI355X yet (not measured): copy it here from the first device run.  The float32 numpy
restatements of tests/test_update_check_cpu.py sit at: multi_sumsq partial 0.05, sumsq[0] 0.014, multi_adamw m 0.13, v 0.13, p 0.27,
multi_ema shadow 0.33, gather exact.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import update_cases as UC
import update_check as K
from gemm_check import nan_buffer

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)
T0 = [None]
F = np.float32
B1, B2 = UC.BETAS


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
            print(f'  {k:40s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - T0[0]:.1f} s')


def _note(r, prefix=''):
    for k, v in r.items():
        RATIOS[prefix + k] = max(RATIOS[prefix + k], v)


def _vp(a):
    return None if a is None else C.c_void_p(int(a))


class Dev(object):
    """a row's image on the device and the SedtChunk table that addresses it"""

    def __init__(self, case, lay, img, reverse=False):
        from sound_event_detection_transformer_amd.optim import _DT
        self.case, self.lay = case, lay
        self.buf = torch.from_numpy(img.copy()).cuda()
        self.base = self.buf.data_ptr()
        assert self.base % 16 == 0 and self.buf.numel() >= lay.nbytes
        fl = K.fields(case)
        t = np.zeros(len(case['chunks']), _DT)
        for ci, ch in enumerate(case['chunks']):
            for f in fl:
                t[f][ci] = self.base + lay.addr((ci, f))
            t['n'][ci], t['lr'][ci], t['wd'][ci] = ch['n'], ch['lr'], ch['wd']
            t['pad'][ci] = 1 if (ch['bf'] and case['kind'] in ('adamw', 'sumsq')) else 0
        if reverse:
            t = t[::-1]
        self.n = len(t)
        self.tab = torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).copy()).cuda()

    def w(self, name):
        return self.base + self.lay.addr((name, 'w'))

    def image(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()


def _sumsq(L, lib, d, step=True, guard=True, seed=True):
    return lib.sedt_multi_sumsq(L.p(d.tab), d.n, _vp(d.w('partial')), _vp(d.w('sumsq')), _vp(d.w('step') if step else None),
                                _vp(d.w('guard') if guard else None), _vp(d.w('seed') if seed else None), L.stream_ptr())


def _adamw(L, lib, d, max_norm, guard=True, sumsq=True, step=True, n=None, tab=True):
    return lib.sedt_multi_adamw(L.p(d.tab) if tab else None, d.n if n is None else n, _vp(d.w('sumsq') if sumsq else None),
                                float(max_norm), B1, B2, UC.EPS, _vp(d.w('step') if step else None), _vp(d.w('guard') if guard else None),
                                L.stream_ptr())


def _ema(L, lib, d, decay, guard=True, n=None, tab=True):
    return lib.sedt_multi_ema(L.p(d.tab) if tab else None, d.n if n is None else n, float(decay), _vp(d.w('guard') if guard else None),
                              L.stream_ptr())


def _gather(L, lib, d, mode, n=None, tab=True):
    return lib.sedt_multi_gather(L.p(d.tab) if tab else None, d.n if n is None else n, mode, L.stream_ptr())


def _launch(L, lib, case, lay, img, reverse=False, clip=True):
    """the row's launch(es) on a fresh copy of the image; returns the image afterwards"""
    d = Dev(case, lay, img, reverse)
    k = case['kind']
    if k == 'sumsq':
        L.check(_sumsq(L, lib, d), 'multi_sumsq')
    elif k == 'adamw':
        if case['max_norm'] is not None and clip:
            L.check(_sumsq(L, lib, d), 'multi_sumsq')
            L.check(_adamw(L, lib, d, case['max_norm']), 'multi_adamw')
        else:
            L.check(_adamw(L, lib, d, 0.0, sumsq=False), 'multi_adamw')
    elif k == 'ema':
        L.check(_ema(L, lib, d, case['decay']), 'multi_ema')
    else:
        L.check(_gather(L, lib, d, case['mode']), 'multi_gather')
    return d.image()


@pytest.mark.parametrize('c', UC.ALL, ids=[c['name'] for c in UC.ALL])
def test_update_envelope(env, c):
    L, lib = env
    lay = K.Layout(c)
    img = K.make_image(c, lay)
    after = _launch(L, lib, c, lay, img)
    _note(K.check_row(c, lay, img, after))
    # a second launch from the same initial state is bit-identical
    assert np.array_equal(after, _launch(L, lib, c, lay, img)), 'a second launch differs'
    # the table in reversed chunk order
    rev = _launch(L, lib, c, lay, img, reverse=True)
    pr = lay.word(rev, 'partial')
    pr[:] = pr[::-1].copy()
    if c['kind'] == 'adamw' and c['max_norm'] is not None:
        assert np.array_equal(lay.word(rev, 'partial').view(np.uint32), lay.word(after, 'partial').view(np.uint32)), 'partial is not reversed'
        _note(K.check_row(c, lay, img, rev))
    else:
        sq = lay.word(rev, 'sumsq')                    # sumsq[0] is added in another order: within its bound, not bit-identical
        if c['kind'] == 'sumsq':
            _note(K.check_row(c, lay, img, rev))
            sq[0] = lay.word(after, 'sumsq')[0]
        assert np.array_equal(after, rev), 'the reversed table gives other bytes'
    if c['name'] in UC.BELOW:
        # norm < max_norm: the coefficient is exactly 1, every tensor equals the unclipped launch's bit for bit
        start = img.copy()
        lay.word(start, 'step')[0] = c['step']
        plain = _launch(L, lib, c, lay, start, clip=False)
        assert float(lay.word(after, 'sumsq')[0]) ** 0.5 < c['max_norm']
        for key in lay.writable:
            assert np.array_equal(lay.bits(after, key), lay.bits(plain, key)), f'{key}: clipping with coef = 1 changed bits'


# ==================================================================================================== guard, step and seed words
GCASE = dict(name='guard_rows', kind='adamw', step=4, max_norm=0.1, gscale=1.0, moments='nonzero',
             chunks=[dict(n=n, off=o, bf=False, lr=UC.LR, wd=UC.WD, tag=f'n{n}') for n, o in ((5, (0, 0, 0, 0)), (1025, (4, 8, 12, 4)), (8, (0, 0, 0, 0)))])


def _guard_image(lay, what, guard):
    img = K.make_image(GCASE, lay, guard=guard or 0)
    g = [lay.get(img, (ci, 'g')) for ci in range(3)]
    if what == 'inf':
        g[1][7] = np.inf
    elif what == 'nan':
        g[1][1024] = np.nan
    elif what == '1e20':
        g[0][:] = 1e20
    elif what in ('sum_overflow', '2.9e38'):
        for a in g:
            a[:] = 0
        if what == 'sum_overflow':
            g[0][0] = g[1][0] = 1.5e19              # two finite squares (and partials) of 2.25e38: only their sum overflows
        else:
            g[1][3] = F(np.sqrt(2.9e38))
    for ci in range(3):
        lay.put(img, (ci, 'g'), g[ci])
    return img


@pytest.mark.parametrize('row', UC.GUARD_ROWS, ids=[r[0] for r in UC.GUARD_ROWS])
def test_guard_step_and_seed_words(env, row):
    L, lib = env
    name, what, guard, up, advance = row
    lay = K.Layout(GCASE)
    img = _guard_image(lay, what, guard)
    d = Dev(GCASE, lay, img)
    L.check(_sumsq(L, lib, d, guard=guard is not None), 'multi_sumsq')
    after = d.image()
    K.check_image_frame(lay, img, after, name)                       # only the words changed
    assert all(np.array_equal(lay.bits(img, key), lay.bits(after, key)) for key in lay.writable)
    step0, seed0 = int(lay.word(img, 'step')[0]), int(lay.word(img, 'seed')[0])
    assert int(lay.word(after, 'step')[0]) == step0 + (1 if advance else 0), 'step word'
    assert int(lay.word(after, 'seed')[0]) == seed0 + 1, 'the seed word always advances'
    assert (int(lay.word(after, 'guard')[0]) != 0) == up, 'guard word'
    if guard is None:
        assert int(lay.word(after, 'guard')[0]) == 0
    s = float(lay.word(after, 'sumsq')[0])                           # written in every row, whatever the guard says
    gs = [lay.get(img, (ci, 'g')) for ci in range(3)]
    if what in ('finite', '2.9e38'):
        assert np.isfinite(s) and s <= 3.0e38
        _note(K.sumsq_check(gs, lay.word(after, 'partial'), s, name))
    elif what == 'nan':
        assert np.isnan(s)
    else:
        assert np.isinf(s) and s > 0
        if what == 'sum_overflow':
            assert np.all(np.isfinite(lay.word(after, 'partial')))
    if up:
        # under a raised guard multi_adamw and multi_ema leave every bit of p, m, v and the shadow alone
        L.check(_adamw(L, lib, d, 0.1), 'multi_adamw')
        L.check(_adamw(L, lib, d, 0.0, sumsq=False), 'multi_adamw')
        L.check(_ema(L, lib, d, 0.999), 'multi_ema')                  # (p = student, m = shadow of the same table)
        assert np.array_equal(after, d.image()), 'an update kernel wrote under a raised guard'


def test_null_words_are_accepted(env):
    L, lib = env
    lay = K.Layout(GCASE)
    img = _guard_image(lay, 'finite', 0)
    d = Dev(GCASE, lay, img)
    L.check(_sumsq(L, lib, d, step=False, guard=False, seed=False), 'multi_sumsq')
    after = d.image()
    K.check_image_frame(lay, img, after, 'null words', untouched=('step', 'guard', 'seed'))
    _note(K.sumsq_check([lay.get(img, (ci, 'g')) for ci in range(3)], lay.word(after, 'partial'), lay.word(after, 'sumsq')[0], 'null words'))
    # null guard on the update kernels: they run
    L.check(_adamw(L, lib, d, 0.1, guard=False), 'multi_adamw')
    L.check(_ema(L, lib, d, 0.999, guard=False), 'multi_ema')
    a2 = d.image()
    assert all(not np.array_equal(lay.bits(a2, (ci, f)), lay.bits(after, (ci, f))) for ci in range(3) for f in 'pmv')


REFUSED = [
    ('multi_sumsq', 'nchunks0'), ('multi_adamw', 'nchunks0'), ('multi_ema', 'nchunks0'), ('multi_gather', 'nchunks0'),
    ('multi_sumsq', 'null_table'), ('multi_adamw', 'null_table'), ('multi_ema', 'null_table'), ('multi_gather', 'null_table'),
    ('multi_gather', 'mode4'), ('multi_gather', 'mode-1'), ('multi_ema', 'decay-0.01'), ('multi_ema', 'decay1.5'), ('multi_ema', 'decaynan'),
    ('multi_adamw', 'clip_null_sumsq'), ('multi_adamw', 'null_step'),
]


@pytest.mark.parametrize('entry,how', REFUSED, ids=[f'{e}_{h}' for e, h in REFUSED])
def test_refused_calls(env, entry, how):
    L, lib = env
    lay = K.Layout(GCASE)
    img = _guard_image(lay, 'finite', 0)
    lay.word(img, 'sumsq')[0] = 1.0
    d = Dev(GCASE, lay, img)
    n = 0 if how == 'nchunks0' else None
    tab = how != 'null_table'
    if entry == 'multi_sumsq':
        rc = lib.sedt_multi_sumsq(L.p(d.tab) if tab else None, 0 if n == 0 else d.n, _vp(d.w('partial')), _vp(d.w('sumsq')), _vp(d.w('step')),
                                  _vp(d.w('guard')), _vp(d.w('seed')), L.stream_ptr())
    elif entry == 'multi_adamw':
        rc = _adamw(L, lib, d, 0.1, sumsq=how != 'clip_null_sumsq', step=how != 'null_step', n=n, tab=tab)
    elif entry == 'multi_ema':
        rc = _ema(L, lib, d, float(how[5:]) if how.startswith('decay') else 0.999, n=n, tab=tab)
    else:
        rc = _gather(L, lib, d, int(how[4:]) if how.startswith('mode') else 0, n=n, tab=tab)
    assert rc != 0 and entry.encode() in lib.sedt_last_error(), (rc, lib.sedt_last_error())
    assert np.array_equal(img, d.image()), 'a refused call wrote'


# ==================================================================================================== single-tensor entry points
def _guarded(n):
    buf = nan_buffer(n + 2 * K.GUARD, torch.float32)
    return buf, buf[K.GUARD:K.GUARD + n]


def _guards_intact(buf, what):
    g = torch.cat([buf[:K.GUARD], buf[-K.GUARD:]]).view(torch.int32)
    assert torch.equal(g, nan_buffer(2 * K.GUARD, torch.float32).view(torch.int32)), f'{what}: elements outside the tensor were written'


def _one_chunk(kind, n, off, **kw):
    return dict(name=f'{kind}1_n{n}', kind=kind, gscale=1.0, chunks=[dict(n=n, off=off, bf=False, lr=UC.LR, wd=UC.WD, tag=f'n{n}')], **kw)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('n', UC.SUMSQ1_N)
def test_single_tensor_sumsq(env, n, accumulate):
    L, lib = env
    c = _one_chunk('sumsq', n, (0, 4, 0, 0))
    lay = K.Layout(c)
    img = K.make_image(c, lay)
    lay.word(img, 'sumsq')[0] = 3.0 if accumulate else np.nan
    d = Dev(c, lay, img)
    nb = lib.sedt_sumsq_scratch(n)
    assert nb == 4 * min(1024, max(1, -(-n // 2048)))
    sbuf, scratch = _guarded(nb // 4)
    g_ptr = _vp(d.base + lay.addr((0, 'g')))
    if n == UC.SUMSQ1_N[0]:                                          # a scratch one float short is refused
        assert lib.sedt_sumsq(g_ptr, n, _vp(d.w('sumsq')), L.p(scratch), nb - 4, accumulate, L.stream_ptr()) != 0
        assert b'sumsq' in lib.sedt_last_error() and np.array_equal(img, d.image())
    L.check(lib.sedt_sumsq(g_ptr, n, _vp(d.w('sumsq')), L.p(scratch), nb, accumulate, L.stream_ptr()), 'sumsq')
    after = d.image()
    K.check_image_frame(lay, img, after, c['name'], untouched=('partial', 'step', 'guard', 'seed'))
    _guards_intact(sbuf, c['name'])
    assert bool(torch.isfinite(scratch).all())
    _note(K.sumsq1_check(lay.get(img, (0, 'g')), lay.word(after, 'sumsq')[0], 3.0, accumulate, c['name']))


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('n', UC.ADAMW1_N)
def test_single_tensor_adamw_clip(env, n, clip):
    L, lib = env
    step = 2
    c = _one_chunk('adamw', n, (4, 8, 12, 4), step=step, max_norm=None, moments='nonzero')
    lay = K.Layout(c)
    img = K.make_image(c, lay)
    d = Dev(c, lay, img)
    ptr = {f: _vp(d.base + lay.addr((0, f))) for f in 'pgmv'}
    coef = (1.0, 0.0)
    if clip:
        sbuf, scratch = _guarded(1)
        L.check(lib.sedt_sumsq(ptr['g'], n, _vp(d.w('sumsq')), L.p(scratch), 4, 0, L.stream_ptr()), 'sumsq')
    L.check(lib.sedt_adamw_clip(ptr['p'], ptr['g'], ptr['m'], ptr['v'], n, _vp(d.w('sumsq')) if clip else None, 0.1 if clip else 0.0,
                                UC.LR, B1, B2, UC.EPS, UC.WD, step, L.stream_ptr()), 'adamw_clip')
    after = d.image()
    K.check_image_frame(lay, img, after, c['name'], untouched=('partial', 'step', 'guard', 'seed') + (() if clip else ('sumsq',)))
    if clip:
        s = lay.word(after, 'sumsq')[0]
        _note(K.sumsq1_check(lay.get(img, (0, 'g')), s, 0.0, 0, c['name']))
        coef = K.clip_coef(s, 0.1)
        assert coef[0] < 1.0
    x = {f: lay.get(img, (0, f)) for f in 'pgmv'}
    got = {f: lay.get(after, (0, f)) for f in 'pmv'}
    _note(K.adamw_check(x, got, UC.LR, UC.WD, K.hyper32(c), coef, step, c['name']), 'adamw_clip ')


# ==================================================================================================== host side (one process)
SIZES = (1, 7, 9, 4096, 65537)


def _host_setup(flat_dtype=None, seed=0):
    """five parameters in three segments and two parameter groups; the 7- and 65537-element parameters and the 9- and 4096-element
    gradients are contiguous slices of a larger storage at an odd element offset"""
    from sound_event_detection_transformer_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i, n in enumerate(SIZES):
        if n in (7, 65537):
            store = torch.randn(n + 8, generator=g).cuda()
            p = torch.nn.Parameter(store[3:3 + n])
            assert p.data_ptr() % 16 != 0
        else:
            p = torch.nn.Parameter(torch.randn(n, generator=g).cuda())
        ps.append(p)
    opt = FusedAdamW([{'params': ps[:3]}, {'params': ps[3:], 'lr': 3 * UC.LR, 'weight_decay': 0.0}], lr=UC.LR, betas=UC.BETAS, eps=UC.EPS,
                     weight_decay=UC.WD)
    opt.set_segments([[ps[0], ps[1]], [ps[2], ps[3]], [ps[4]]])
    if flat_dtype is not None:
        opt.enable_flat_grads(flat_dtype)
    return ps, opt, g


def _set_grads(ps, g, scale=1.0):
    for p in ps:
        n = p.numel()
        if n in (9, 4096):
            store = (scale * torch.randn(n + 8, generator=g)).cuda()
            p.grad = store[1:1 + n]
            assert p.grad.data_ptr() % 16 != 0 and p.grad.is_contiguous()
        else:
            p.grad = (scale * torch.randn(n, generator=g)).cuda()
    return [p.grad.clone() for p in ps]


def _slots(opt):
    """[(first element, elements)] of every parameter in the flat layout, and a mask of the padding slots between them"""
    out, e0 = [], 0
    for p, pad in zip(opt._ps, opt._pad):
        out.append((e0, p.numel()))
        e0 += pad
    pad = np.ones(e0, bool)
    for a, n in out:
        pad[a:a + n] = False
    return out, pad


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).cpu().numpy().view(np.uint32)


def _check_flat(opt, want, what):
    """want: per parameter the expected bits of its slot (None: still zero); the padding slots stay zero"""
    flat = _bits(opt._flat_g)
    slots, pad = _slots(opt)
    assert not flat[pad].any(), f'{what}: a padding slot was written'
    for (a, n), w in zip(slots, want):
        if w is None:
            assert not flat[a:a + n].any(), f'{what}: a slot outside the requested part was written'
        else:
            assert np.array_equal(flat[a:a + n], w), f'{what}: slot at {a} is not the exact result'


def _f(t):
    return t.detach().float().cpu().numpy()


def test_host_gather_modes(env):
    L, lib = env
    # plain, then accumulate=True on top of it
    ps, opt, g = _host_setup()
    g1 = _set_grads(ps, g)
    opt.gather_grads()
    order = opt._ps
    g1 = {id(p): _f(x) for p, x in zip(ps, g1)}
    _check_flat(opt, [K.gather_ref_bits(g1[id(p)], None, 0) for p in order], 'gather')
    g2 = {id(p): _f(x) for p, x in zip(ps, _set_grads(ps, g))}
    opt.gather_grads(accumulate=True)
    _check_flat(opt, [K.gather_ref_bits(g2[id(p)], g1[id(p)].view(np.uint32), 1) for p in order], 'gather accumulate')
    # part = k fills segment k alone
    for k in range(3):
        ps, opt, g = _host_setup()
        gk = {id(p): _f(x) for p, x in zip(ps, _set_grads(ps, g))}
        view = opt.gather_grads(part=k)
        seg = set(id(p) for p in opt.segment_params(k))
        assert view.numel() == sum((p.numel() + 7) // 8 * 8 for p in opt.segment_params(k))
        _check_flat(opt, [K.gather_ref_bits(gk[id(p)], None, 0) if id(p) in seg else None for p in opt._ps], f'gather part={k}')
    # a bf16 flat buffer: round to nearest even, and float(old) + g rounded again when accumulating
    ps, opt, g = _host_setup(torch.bfloat16)
    g1 = {id(p): _f(x) for p, x in zip(ps, _set_grads(ps, g))}
    opt.gather_grads()
    _check_flat(opt, [K.gather_ref_bits(g1[id(p)], None, 2) for p in opt._ps], 'gather bf16')
    g2 = {id(p): _f(x) for p, x in zip(ps, _set_grads(ps, g))}
    opt.gather_grads(accumulate=True)
    _check_flat(opt, [K.gather_ref_bits(g2[id(p)], K.f2bf(g1[id(p)]), 3) for p in opt._ps], 'gather bf16 accumulate')
    assert opt.flat_views() is None
    # gradients already living in their flat_views() slots are left alone: no launch when all do, the others are copied when some do
    ps, opt, g = _host_setup()
    views = opt.flat_views()
    for p in ps:
        views[p.data_ptr()].copy_(torch.randn(p.shape, generator=g))
        p.grad = views[p.data_ptr()]
    before = _bits(opt._flat_g).copy()
    with L.launch_log() as log:
        opt.gather_grads()
    assert log['multi_gather'] == 0 and np.array_equal(_bits(opt._flat_g), before)
    keep = ps[1]
    _set_grads([p for p in ps if p is not keep], g)
    held = _bits(keep.grad).copy()
    with L.launch_log() as log:
        opt.gather_grads()
    assert log['multi_gather'] == 1
    _check_flat(opt, [held if p is keep else K.gather_ref_bits(_f(p.grad), None, 0) for p in opt._ps], 'gather beside a delivered gradient')


@pytest.mark.parametrize('flat_dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_host_step_from_flat(env, flat_dtype):
    """FusedAdamW.step(from_flat=True, max_norm > 0) against the checker's references, within the same bounds on p, m, v; the bf16
    reference uses the rounded gradients"""
    L, lib = env
    ps, opt, g = _host_setup(flat_dtype, seed=1)
    hp = dict(b1=F(B1), b2=F(B2), eps=F(UC.EPS))
    steps = 3
    for step in range(1, steps + 1):
        _set_grads(ps, g)
        opt.gather_grads()
        slots, _ = _slots(opt)
        flat = _f(opt._flat_g)
        x = [dict(p=_f(p), g=flat[a:a + n], m=_f(opt._m[a:a + n]), v=_f(opt._v[a:a + n])) for p, (a, n) in zip(opt._ps, slots)]
        opt.step(max_norm=0.1, from_flat=True)
        torch.cuda.synchronize()
        gs = [xx['g'][c0:c0 + 65536] for xx in x for c0 in range(0, len(xx['g']), 65536)]           # the optimizer's own chunks
        s = float(opt._sumsq.item())
        _note(K.sumsq_check(gs, _f(opt._partial), s, f'step {step}'), 'FusedAdamW ')
        coef = K.clip_coef(s, 0.1)
        assert coef[0] < 1.0
        for i, (p, (a, n)) in enumerate(zip(opt._ps, slots)):
            grp = opt.param_groups[0] if any(p is q for q in opt.param_groups[0]['params']) else opt.param_groups[1]
            got = dict(p=_f(p), m=_f(opt._m[a:a + n]), v=_f(opt._v[a:a + n]))
            _note(K.adamw_check(x[i], got, grp['lr'], grp['weight_decay'], hp, coef, step, f'step {step} n={n}'), 'FusedAdamW ')
        assert int(opt._step_t.item()) == step
    _, pad = _slots(opt)
    assert not _f(opt._m)[pad].any() and not _f(opt._v)[pad].any()


class _Pair(object):
    """all EMA needs of a model: named_parameters()"""

    def __init__(self, params):
        self.params = params

    def named_parameters(self):
        return list(self.params.items())


def test_host_ema_update_on_misaligned_slices(env):
    from sound_event_detection_transformer_amd.utilities.utils import EMA
    g = torch.Generator().manual_seed(2)
    params, shadow = {}, {}
    for i, (n, po, so) in enumerate(((7, 1, 0), (4097, 0, 3), (65537, 3, 1))):
        params[f'w{i}'] = torch.nn.Parameter(torch.randn(n + 8, generator=g).cuda()[po:po + n])
        shadow[f'w{i}'] = torch.randn(n + 8, generator=g).cuda()[so:so + n]
        assert (params[f'w{i}'].data_ptr() | shadow[f'w{i}'].data_ptr()) % 16 != 0
    ema = EMA(_Pair(params), UC.EMA_DEFAULT)
    ema.shadow = shadow
    before = {k: _f(v) for k, v in shadow.items()}
    ema.update()
    torch.cuda.synchronize()
    for k, p in params.items():
        RATIOS['EMA.update shadow'] = max(RATIOS['EMA.update shadow'],
                                          K.ema_check(_f(p), before[k], _f(ema.shadow[k]), UC.EMA_DEFAULT, f'EMA.update {k}'))
