"""GPU: weight preparation and the split-K finishing pass at their tile, vector, unroll and job-table edges, element by element
(tests/prep_check.py: references, bounds, restatements; tests/prep_cases.py: the rows): sedt_multi_pack (multi_pack_kernel, pack_tile,
pack_tile_vec) and sedt_pack_conv, the PackPlan / PlanSet host tables, sedt_pack_frag, sedt_multi_bn_fold / sedt_bn_fold, sedt_stem_prep,
sedt_stem_conv0_grad, sedt_multi_wgrad_reduce / sedt_wgrad_reduce / sedt_wgrad_reduce_bias.

The C entry points are called through lib.load() with pointers into guard frames (glue_check.Frame) and, where the entry takes one, the
module's own device job table.  Per row: gemm_check.poison() before the launch; no byte outside the owned elements changes; every owned
element is written; a second launch (the other entry point of the same kernel, or the same job at another place of a table) gives
identical bits; the exact kernels - pack, frag, reduce - equal their np.float32 restatement bit for bit and float64 under the bound, the
bounded ones - bn_fold, stem_prep, stem_conv0_grad - stay under their bound.  The synthetic split-K slabs give every slice a magnitude and
every row a row scale of its own; no GEMM runs here.  Then the refused calls and the empty tensors: sedt_bn_fold and sedt_pack_conv
launched nblk(0) = 0 blocks for an empty tensor and checked no argument; they now return 0 for empty and name the entry point for a null
pointer or a negative dimension (test_bn_fold_and_pack_conv_arguments).  No row is sampled or skipped.

The largest error / bound ratio per kernel, the k_rsqrt measurement and the module's run time are printed at the end with -s.  On MI355X
(0.9 s inside the whole suite, 1.9 s alone; [dtype] = the row's compute dtype, a bf16 output's ratio is mostly its own rounding):
  bn_fold scale [f32]        0.118     bn_fold bias [f32]         0.43      k:rsqrt(bn_fold)           1.88 (K_FN: 8)
  pack wf [f32]              0         pack wf [bf16]             0.498     pack wb [f32]              0.499
  pack wb [bf16]             0.498     frag wf                    0.497     frag wb                    0.495
  stem_prep [f32]            0.756     stem_prep [bf16]           0.497     stem_conv0_grad dw0        0.013
  stem_conv0_grad db0        0.0166    reduce out [f32]           0.68      reduce colsum [f32]        0.443
The exact kernels' ratios are those of their restatements by construction (tests/test_prep_check_cpu.py prints the same figures).  No
kernel failed a row; the entry-point changes and PackPlan's alignment filter came from reading the code, before the rows were run.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import prep_cases as PC
import prep_check as K
from gemm_check import poison
from glue_check import bits, ratio_key
from test_glue_envelope_gpu import _frame, _refused, up, vp

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)
T0 = [None]
DT = dict(f32=0, bf16=1)
PATTERN = 0xA5


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, packing
    assert torch.cuda.is_available()
    lib = L.load()
    T0[0] = time.time()
    yield L, lib, packing
    if RATIOS:
        print('\nlargest error / bound ratio per kernel and output (k: the k_fn measurement, in units of 2^-24 |ref|):')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - T0[0]:.1f} s')


class Row(object):
    """a row's inputs and frames on the device; the inputs a row's `mis` names sit 4 bytes past a 16-byte boundary"""
    LEAD = {('pack', 'w', 'w'): 4, ('reduce', 'slab', 'slab'): 4}

    def __init__(self, key, c):
        self.key, self.c, self.k = key, c, K.KERNELS[key]
        self.inp = self.k.make(c)
        self.fr = self.k.frames(c, self.inp)
        self.P_in, self.T_in = {}, {}
        for n, a in self.inp.items():
            self.T_in[n], self.P_in[n] = up(a, self.LEAD.get((key, n, c.get('mis')), 0))
        self.P, self.T = dict(self.P_in), dict(self.T_in)

    def fresh_frames(self):
        self.P, self.T = dict(self.P_in), dict(self.T_in)
        for n, f in self.fr.items():
            t, p = up(f.buf)
            self.T[n], self.P[n] = t, p + f.off * f.buf.itemsize
            assert self.P[n] % 16 == ((f.off - 32) * f.buf.itemsize) % 16

    def images(self):
        torch.cuda.synchronize()
        return {n: self.T[n].cpu().numpy()[:f.buf.nbytes].view(f.buf.dtype).copy() for n, f in self.fr.items()}

    def verify(self, img):
        for k, v in K.verify_row(self.key, self.c, self.inp, self.fr, img).items():
            RATIOS[ratio_key(k, self.c)] = max(RATIOS[ratio_key(k, self.c)], v)

    def same(self, a, b, what):
        for n in self.fr:
            assert np.array_equal(bits(a[n]), bits(b[n])), f'{self.c["name"]}.{n}: {what}'


def launches(r, *fns):
    """the row through each launcher on fresh frames, poisoned before; the first result is verified, the others must equal its bits"""
    imgs = []
    for fn in fns:
        r.fresh_frames()
        poison(16)
        fn(r)
        imgs.append(r.images())
    r.verify(imgs[0])
    for i in imgs[1:]:
        r.same(imgs[0], i, 'a second launch differs')
    return imgs[0]


def table_launches(rows, launch):
    """all rows as the jobs of one launch, in table order and then in reverse (first blocks recomputed): every job verified, and every
    job's bits the same at either place of the table"""
    first = None
    for order in (list(range(len(rows))), list(range(len(rows)))[::-1]):
        for r in rows:
            r.fresh_frames()
        poison(16)
        launch([rows[i] for i in order])
        imgs = [r.images() for r in rows]
        if first is None:
            first = imgs
            for r, i in zip(rows, imgs):
                r.verify(i)
        else:
            for r, a, b in zip(rows, first, imgs):
                r.same(a, b, 'the job gives other bits at another place of the table')
    return first


# ================================================================================================ pack
def pack_launch(env, dt):
    L, lib, packing = env

    def go(rows):
        t = np.zeros(len(rows), packing._PK)
        e0 = 0
        for i, r in enumerate(rows):
            c = r.c
            t[i]['w'], t[i]['bnscale'], t[i]['wf'], t[i]['wb'] = r.P['w'], (r.P['scale'] if c['scale'] else 0), r.P.get('wf', 0), r.P.get('wb', 0)
            t[i]['e0'], t[i]['Cout'], t[i]['Cin'], t[i]['taps'] = e0, c['Co'], c['Ci'], c['taps']
            e0 += PC.pack_blocks(c)
            assert r.P['w'] % 16 == (4 if c['mis'] == 'w' else 0)
        dev, p = up(t)
        L.check(lib.sedt_multi_pack(vp(p), len(rows), e0, DT[dt], L.stream_ptr()), 'multi_pack')
        torch.cuda.synchronize()
        del dev
    return go


def pack_conv_launch(env, r):
    L, lib, _ = env
    c, P = r.c, r.P
    L.check(lib.sedt_pack_conv(vp(P['w']), c['Co'], c['Ci'], c['taps'], vp(P['scale']) if c['scale'] else None, vp(P.get('wf')), vp(P.get('wb')),
                               DT[c['dt']], L.stream_ptr()), 'pack_conv')


@pytest.mark.parametrize('dt', PC.DTS)
def test_pack_rows(env, dt):
    """every row as a table of one job and through sedt_pack_conv: the same bits; a row with a pointer off its 16-byte boundary (scalar
    path) gives the bits of the same tensor aligned (vector path)"""
    go = pack_launch(env, dt)
    pairs = 0
    for c in [c for c in PC.PACK if c['dt'] == dt]:
        r = Row('pack', c)
        img = launches(r, lambda r: go([r]), lambda r: pack_conv_launch(env, r))
        if c['mis'] != 'none':
            c0 = dict(c, mis='none')                         # same name -> same inputs, every pointer aligned
            assert PC.pack_path(c0) == 'vec' and PC.pack_path(c) == 'scalar'
            r0 = Row('pack', c0)
            img0 = launches(r0, lambda r: go([r]))
            for n in r.fr:
                assert np.array_equal(bits(r.fr[n].owned(img[n])), bits(r0.fr[n].owned(img0[n]))), f'{c["name"]}.{n}: the scalar and the vector path differ'
            pairs += 1
    assert pairs == 3


@pytest.mark.parametrize('dt', PC.DTS)
def test_pack_table(env, dt):
    rows = [Row('pack', c) for c in PC.pack_table(dt)]
    table_launches(rows, pack_launch(env, dt))


# ================================================================================================ PackPlan / PlanSet
def _plan_parts(dt, salt):
    """the section-1 shapes as convs (FrozenBN on every other one), linears, bn_only, frags and conv_frags; host copies by id"""
    bnk, host, alive = K.KERNELS['bn_fold'], {}, []

    def tens(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        host[id(t)] = a
        alive.append(t)                                      # (host is keyed by id: no tensor of the set may be freed)
        return t

    def weight(Co, Ci, taps, i, linear=False):
        c = dict(Co=Co, Ci=Ci, taps=taps, dt=dt, scale=1, wf=1, wb=1, mis='none', name=f'plan{salt}_{i}_{Co}x{Ci}x{taps}')
        w = K.KERNELS['pack'].make(c)['w']
        return tens(w.reshape(Co, Ci) if linear else w)

    def bn(n, i):
        b = bnk.make(dict(n=n, name=f'plan{salt}_bn{i}_{n}'))
        return tuple(tens(b[k]) for k in ('w', 'b', 'rm', 'rv'))

    shapes = sorted({(c['Co'], c['Ci'], c['taps']) for c in PC.PACK})
    convs = [(weight(co, ci, t, i), bn(co, i) if i % 2 == 0 else None) for i, (co, ci, t) in enumerate(shapes)]
    linears = [weight(n, k, 1, 100 + i, linear=True) for i, (n, k) in enumerate([(64, 64), (72, 136), (65, 64), (96, 160), (32, 64), (1, 1)])]
    # a 32 x 32 linear that is a view 4 bytes past a 16-byte boundary: packed (scalar path), but below pack_frag's float4 alignment
    a = K.KERNELS['pack'].make(dict(Co=32, Ci=32, taps=1, dt=dt, scale=1, wf=1, wb=1, mis='none', name=f'plan{salt}_view'))['w'].reshape(32, 32)
    view = tens(np.concatenate([np.zeros(1, np.float32), a.reshape(-1)]))[1:].view(32, 32)
    assert view.data_ptr() % 16 == 4
    host[id(view)] = a
    alive.append(view)
    linears.append(view)
    bn_only = [(weight(8, 8, 1, 200), bn(8, 200)), (weight(4, 4, 10, 201), bn(4, 201))]
    host['alive'] = alive
    conv_frags = [w for w, _ in convs if tuple(w.shape) in ((64, 64, 1), (32, 32, 9), (32, 32, 2), (32, 32, 8))]
    return convs, linears, bn_only, list(linears), conv_frags, host


def _check_plan(plan, dt, parts, what):
    """every element of every table entry equals the restatement; gaps and tails keep the pattern"""
    convs, linears, bn_only, frags, conv_frags, host = parts
    torch.cuda.synchronize()
    es = 4 if dt == 'f32' else 2
    npdt = np.float32 if dt == 'f32' else np.uint16
    wimg = plan.wbuf.cpu().view(torch.uint8).numpy().view(npdt)
    sc_img, bi_img = plan.scale_buf.cpu().numpy(), plan.bias_buf.cpu().numpy()
    cover = np.zeros(wimg.shape, bool)
    bn_cover = np.zeros(sc_img.shape, bool)
    bn_of = {id(w): b for w, b in convs + bn_only}
    packed = {}
    for w, wf, wb, sc, bi in plan._entries:
        Co, Ci = w.shape[0], w.shape[1]
        taps = w.numel() // (Co * Ci)
        hw = np.asarray(host[id(w)] if id(w) in host else w.cpu().numpy(), np.float32).reshape(Co, Ci, taps)
        scale = np.ones(Co, np.float32)
        if sc is not None:
            o = (sc.data_ptr() - plan.scale_buf.data_ptr()) // 4
            scale = sc_img[o:o + Co]
            b = bn_of[id(w)]
            got = dict(scale=scale[None], bias=bi_img[o:o + Co][None])
            for k, v in K.KERNELS['bn_fold'].verify(dict(n=Co, name=f'{what} bn {Co}'), {n: host[id(t)] for n, t in zip(('w', 'b', 'rm', 'rv'), b)}, got).items():
                RATIOS[ratio_key(k, {})] = max(RATIOS[ratio_key(k, {})], v)
            assert not bn_cover[o:o + Co].any()
            bn_cover[o:o + Co] = True
        c = dict(Co=Co, Ci=Ci, taps=taps, dt=dt, scale=int(sc is not None), name=what)
        ref = K.KERNELS['pack'].images(c, dict(w=hw, scale=scale))
        for n, t in (('wf', wf), ('wb', wb)):
            if t is None or t.data_ptr() == w.data_ptr():
                continue
            o = (t.data_ptr() - plan.wbuf.data_ptr()) // es
            assert o % 8 == 0 and not cover[o:o + t.numel()].any()
            K.exact(wimg[o:o + t.numel()][None], ref[n].reshape(1, -1), f'{what}: {n} of {tuple(w.shape)}')
            cover[o:o + t.numel()] = True
            packed[(id(w), n)] = ref[n]
    fill = np.full(1, PATTERN, np.uint8).repeat(es).view(npdt)[0]
    assert (bits(wimg[~cover]) == bits(np.asarray([fill]))[0]).all(), f'{what}: an alignment gap or the tail of wbuf changed'
    assert (~cover[:-64]).any(), 'the table has no alignment gap'
    n_bn = sum(b[0].numel() for _, b in convs + bn_only if b is not None)
    assert bn_cover.sum() == n_bn == sc_img.size
    rows = [dict(Co=w.shape[0], Ci=w.shape[1], taps=w.numel() // (w.shape[0] * w.shape[1])) for w, wf, wb, _, _ in plan._entries if wb is not None]
    assert plan._nblocks == sum(PC.pack_blocks(c) for c in rows) and len(plan._pk) == len(rows)
    if dt != 'bf16':
        assert not len(plan._fj)
        return
    fimg = plan.fbuf.cpu().view(torch.int16).numpy().view(np.uint16)
    fcover = np.zeros(fimg.shape, bool)

    def frag_is(t, b2d, name):
        o = (t.data_ptr() - plan.fbuf.data_ptr()) // 2
        K.exact(fimg[o:o + t.numel()][None], K.frag_layout(b2d), f'{what}: {name}')
        assert not fcover[o:o + t.numel()].any()
        fcover[o:o + t.numel()] = True

    # (64,64), (96,160), (32,64) of the linears - not the misaligned 32 x 32 view, which _init_frags leaves out; the four conv shapes
    assert len(plan._fr_entries) == 3 and len(plan._cf_entries) == 4 and linears[-1].data_ptr() % 16 == 4
    assert all(w.data_ptr() % 16 == 0 for w, _, _ in plan._fr_entries) and linears[-1].data_ptr() not in plan.frag_table
    for w, wf, wb in plan._fr_entries:
        b = K.to_bf16(host[id(w)].reshape(tuple(w.shape)))
        frag_is(wf, b, f'frag W {tuple(w.shape)}')
        frag_is(wb, np.ascontiguousarray(b.T), f'frag W^T {tuple(w.shape)}')
    for w, ff, bf in plan._cf_entries:
        frag_is(ff, packed[(id(w), 'wf')], f'conv frag fwd {tuple(w.shape)}')
        frag_is(bf, packed[(id(w), 'wb')], f'conv frag dgrad {tuple(w.shape)}')
    assert fcover.all()
    assert plan._fr_blocks == sum((int(j['N']) // 32) * (int(j['K']) // 32) for j in plan._fj)


def _fill(plan):
    for t in (plan.wbuf, plan.scale_buf, plan.bias_buf) + ((plan.fbuf,) if len(plan._fj) else ()):
        t.view(torch.uint8).fill_(PATTERN)


@pytest.mark.parametrize('dt', PC.DTS)
def test_pack_plan_and_plan_set_tables(env, dt):
    L, lib, packing = env
    parts = _plan_parts(dt, 0)
    convs, linears, bn_only, frags, conv_frags, host = parts
    dev = torch.device('cuda')
    made = []

    def factory():
        made.append(packing.PackPlan(DT[dt], dev, convs, linears, bn_only, frags, conv_frags))
        _fill(made[-1])
        return made[-1]

    ps = packing.PlanSet(factory)
    with ps as p0:
        pass
    assert p0 is made[0] and len(ps.plans) == 1
    _check_plan(p0, dt, parts, f'plan[{dt}]')
    keep = [t.clone() for t in (p0.wbuf, p0.scale_buf, p0.bias_buf)]
    last = p0._last
    # every parameter's and buffer's .data swapped to another tensor (the EMA shadow): a second plan, whose images follow the new pointers
    other = _plan_parts(dt, 1)
    olds = []
    flat = lambda ps_: [t for w, b in ps_[0] + ps_[2] for t in (w,) + (b or ())] + list(ps_[1])
    for t, o in zip(flat(parts), flat(other)):
        olds.append(t.data)
        t.data = o.data
        host[('old', id(t))] = host[id(t)]
        host[id(t)] = other[5][id(o)]
    with ps as p1:
        pass
    assert p1 is made[1] and p1 is not p0 and len(ps.plans) == 2
    _check_plan(p1, dt, parts, f'plan2[{dt}]')
    torch.cuda.synchronize()
    for a, b in zip(keep, (p0.wbuf, p0.scale_buf, p0.bias_buf)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), 'the first plan\'s buffers changed under the second plan'
    for t, o in zip(flat(parts), olds):
        t.data = o
        host[id(t)] = host[('old', id(t))]
    assert ps.current() is p0 and p0._last is last and len(ps.plans) == 2
    _fill(p0)
    with ps as p:
        assert p is p0 and p0._last is last
    _check_plan(p0, dt, parts, f'plan again[{dt}]')


# ================================================================================================ pack_frag
def frag_launch(env):
    L, lib, packing = env

    def go(rows):
        t = np.zeros(len(rows), packing._FJ)
        blk = 0
        for i, r in enumerate(rows):
            c = r.c
            t[i]['w'], t[i]['wf'], t[i]['wb'] = r.P['w'], r.P.get('wf', 0), r.P.get('wb', 0)
            t[i]['N'], t[i]['K'], t[i]['blk0'], t[i]['src_bf16'] = c['N'], c['K'], blk, int(c['src'] == 'bf16')
            blk += (c['N'] // 32) * (c['K'] // 32)
            assert r.P['w'] % 16 == 0 and all(r.P[n] % 16 == 0 for n in r.fr)
        dev, p = up(t)
        L.check(lib.sedt_pack_frag(vp(p), len(rows), blk, L.stream_ptr()), 'pack_frag')
        torch.cuda.synchronize()
        del dev
    return go


@pytest.mark.parametrize('src', PC.DTS)
def test_pack_frag_table(env, src):
    """twelve jobs in one table: four shapes, both images / W only / W^T only; the bf16 source is a packed operand of multi_pack"""
    rows = [Row('frag', c) for c in PC.FRAG if c['src'] == src]
    assert len(rows) == 12
    table_launches(rows, frag_launch(env))


# ================================================================================================ FrozenBN fold, stem
def test_bn_fold_rows_and_table(env):
    L, lib, packing = env

    def single(r):
        P = r.P
        L.check(lib.sedt_bn_fold(vp(P['w']), vp(P['b']), vp(P['rm']), vp(P['rv']), vp(P['scale']), vp(P['bias']), r.c['n'], L.stream_ptr()), 'bn_fold')

    def multi(rows):
        t = np.zeros(len(rows), packing._BN)
        for i, r in enumerate(rows):
            for n in ('w', 'b', 'rm', 'rv', 'scale', 'bias'):
                t[i][n] = r.P[n]
            t[i]['n'] = r.c['n']
        dev, p = up(t)
        L.check(lib.sedt_multi_bn_fold(vp(p), len(rows), L.stream_ptr()), 'multi_bn_fold')
        torch.cuda.synchronize()
        del dev

    rows = [Row('bn_fold', c) for c in PC.BN_FOLD]
    for r in rows:
        launches(r, single, lambda r: multi([r]))
    assert [r.c['n'] for r in rows] == [0, 1, 255, 256, 257, 2048]
    table_launches(rows, multi)
    print(f'\nk_rsqrt measured: {RATIOS["k:rsqrt(bn_fold)"]:.3g} (K_FN: {K.K_FN["rsqrt"]})')
    assert 4 * RATIOS['k:rsqrt(bn_fold)'] <= K.K_FN['rsqrt'], 'K_FN[rsqrt] is less than four times the measured value'


def test_stem_prep_and_conv0_grad(env):
    L, lib, _ = env
    for c in PC.STEM_PREP:
        go = lambda r: L.check(lib.sedt_stem_prep(vp(r.P['w0']), vp(r.P['b0']), vp(r.P['w1']), vp(r.P['wcat']), DT[r.c['dt']], L.stream_ptr()), 'stem_prep')
        launches(Row('stem_prep', c), go, go)
    for c in PC.STEM_CONV0_GRAD:
        go = lambda r: L.check(lib.sedt_stem_conv0_grad(vp(r.P['G']), vp(r.P['w1']), vp(r.P['dw0']), vp(r.P['db0']), L.stream_ptr()), 'stem_conv0_grad')
        launches(Row('stem_conv0_grad', c), go, go)


# ================================================================================================ split-K reduce
def red_job(L, r):
    c, P = r.c, r.P
    j = L.SedtReduceJob()
    if c['Ci']:
        j.slab, j.out = P['slab'], P['out']
        assert P['slab'] % 16 == (4 if c['mis'] == 'slab' else 0) and P['out'] % 16 == (4 if c['mis'] == 'out' else 0)
    if c['scale']:
        j.rowscale = P['rowscale']
    if c['cs'] is not None:
        j.colsum_slab, j.bias_out, j.cs_splitk = P['cs'], P['bias'], c['cs']
    j.splitk, j.R, j.taps, j.Ci = c['splitk'], c['R'], c['taps'], c['Ci']
    return j


def reduce_launch(env, pf=None):
    L, lib, _ = env

    def go(rows):
        arr = (L.SedtReduceJob * len(rows))(*[red_job(L, r) for r in rows])
        L.check(lib.sedt_multi_wgrad_reduce(arr, len(rows), pf, L.stream_ptr()), 'multi_wgrad_reduce')
    return go


def reduce_single(env, r):
    """the single-job entry points where they can express the row (a slab, and column sums with the slab's slice count)"""
    L, lib, _ = env
    c, P = r.c, r.P
    if not c['Ci'] or (c['cs'] or 0) > 0:
        return reduce_launch(env)([r])
    a = (vp(P['slab']), c['splitk'], c['R'], c['taps'], c['Ci'], vp(P['rowscale']) if c['scale'] else None, vp(P['out']))
    if c['cs'] is None:
        L.check(lib.sedt_wgrad_reduce(*a, L.stream_ptr()), 'wgrad_reduce')
    else:
        L.check(lib.sedt_wgrad_reduce_bias(*a, vp(P['cs']), vp(P['bias']), L.stream_ptr()), 'wgrad_reduce')


@pytest.mark.parametrize('mode', ['mode0', 'mode1', 'mode2', 'mode3', 'sums_only'])
def test_reduce_rows(env, mode):
    rows = [c for c in PC.REDUCE if (f'mode{PC.reduce_mode(c)}' if c['Ci'] else 'sums_only') == mode]
    assert rows
    go = reduce_launch(env)
    for c in rows:
        launches(Row('reduce', c), lambda r: go([r]), lambda r: reduce_single(env, r))


def test_reduce_table_prefetch_and_refusals(env):
    L, lib, _ = env
    rows = [Row('reduce', c) for c in PC.reduce_table()]
    assert len(rows) == L.MAX_REDUCE_JOBS == PC.MAX_REDUCE_JOBS
    first = table_launches(rows, reduce_launch(env))
    # the same launch with a prefetch hint: regions of 0, 127, 128 and 4096 bytes; same outputs, the regions unchanged
    src = np.random.default_rng(7).integers(0, 256, 8192, dtype=np.uint8)
    for sizes in ((0, 127, 128), (4096, 128, 0)):
        t, p = up(src)
        pf = L.SedtPrefetch()
        for i, n in enumerate(sizes):
            pf.ptr[i], pf.bytes[i] = p + 4096 * (i % 2) + 256 * (i // 2), n
        for r in rows:
            r.fresh_frames()
        poison(16)
        reduce_launch(env, C.byref(pf))(rows)
        for r, a in zip(rows, first):
            r.same(a, r.images(), f'the prefetch hint {sizes} changed a result')
        assert np.array_equal(t.cpu().numpy()[:src.size], src), 'the prefetched bytes changed'
    # refused: 41 jobs; a null slab / output on a job that is not sums-only; column sums without bias_out and the reverse
    ok = next(r for r in rows if r.c['Ci'] and r.c['cs'] is not None)
    ok.fresh_frames()
    before = [(ok.T[n], ok.T[n].cpu().clone()) for n in ok.fr]

    def refused(jobs):
        arr = (L.SedtReduceJob * len(jobs))(*jobs)
        _refused(L, lib, lib.sedt_multi_wgrad_reduce(arr, len(jobs), None, L.stream_ptr()), 'multi_wgrad_reduce', before)

    refused([red_job(L, ok)] * 41)
    for field in ('slab', 'out', 'colsum_slab', 'bias_out'):
        j = red_job(L, ok)
        setattr(j, field, None)
        refused([red_job(L, ok), j])
        assert 'job 1' in lib.sedt_last_error().decode(), lib.sedt_last_error().decode()
    j = red_job(L, ok)
    j.splitk = 0
    refused([j])
    P = ok.P
    a = (vp(P['slab']), ok.c['splitk'], ok.c['R'], ok.c['taps'], ok.c['Ci'], None, vp(P['out']))
    _refused(L, lib, lib.sedt_wgrad_reduce_bias(*a, vp(P['cs']), None, L.stream_ptr()), 'wgrad_reduce', before)
    _refused(L, lib, lib.sedt_wgrad_reduce_bias(*a, None, vp(P['bias']), L.stream_ptr()), 'wgrad_reduce', before)
    _refused(L, lib, lib.sedt_wgrad_reduce(None, *a[1:], L.stream_ptr()), 'wgrad_reduce', before)


# ================================================================================================ entry points
def test_bn_fold_and_pack_conv_arguments(env):
    """an empty tensor is status 0 and no launch (a grid of 0 blocks is a launch error); a null required pointer or a negative dimension
    is refused with the entry point's name; the frame is untouched either way"""
    L, lib, _ = env
    S = L.stream_ptr()
    t, p, b = _frame('f32', 1, 64)
    src_t, src = up(np.ones(64, np.float32))
    assert lib.sedt_bn_fold(vp(src), vp(src), vp(src), vp(src), vp(p), vp(p), 0, S) == 0, lib.sedt_last_error().decode()
    assert lib.sedt_bn_fold(None, None, None, None, None, None, 0, S) == 0
    for dims in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
        for dt in (0, 1):
            assert lib.sedt_pack_conv(vp(src), *dims, vp(src), vp(p), vp(p), dt, S) == 0, (dims, lib.sedt_last_error().decode())
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), b)
    _refused(L, lib, lib.sedt_bn_fold(vp(src), vp(src), vp(src), vp(src), vp(p), vp(p), -1, S), 'bn_fold', [(t, b)])
    for null in range(6):
        a = [vp(src)] * 4 + [vp(p)] * 2
        a[null] = None
        _refused(L, lib, lib.sedt_bn_fold(*a, 4, S), 'bn_fold', [(t, b)])
    _refused(L, lib, lib.sedt_pack_conv(None, 2, 2, 1, None, vp(p), vp(p), 0, S), 'pack_conv', [(t, b)])
    for dims in ((-1, 2, 1), (2, -1, 1), (2, 2, -1)):
        _refused(L, lib, lib.sedt_pack_conv(vp(src), *dims, None, vp(p), vp(p), 0, S), 'pack_conv', [(t, b)])
    assert lib.sedt_pack_conv(vp(src), 2, 2, 1, None, vp(p), vp(p), 7, S) != 0          # an unknown dtype
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), b)
    del src_t
