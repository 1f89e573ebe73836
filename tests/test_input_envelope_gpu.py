"""GPU: the seven kernels of csrc/input.hip (box_transform, box_transform_views, scaler_clip_stats + scaler_accumulate, mixup,
mixup_targets, query_patch) at their band, frame, wave and LDS edges, element by element (tests/input_check.py: references, bounds,
guard frames, restatements; tests/input_cases.py: the rows).

One parametrised test per kernel over its rows.  A row is driven through the Python class or op where it can express the case ('ops':
DeviceBoxTransform, DeviceViewTransform, ops.mixup, DeviceQuery) and through the C entry point otherwise ('c': the constant fill, row
counts the Python layer refuses, non-zero accumulators, the label merge's raw tables).  Every output is a guard frame
(input_check.Frame); after the synchronisation the images go through the same verify() as the np.float32 restatements of
tests/test_input_check_cpu.py.  The refusal rows assert that the entry point raises and that nothing was launched (lib.launch_log) or
written.  box_transform_views: view 0 and every clean view 1 must also equal the single-view kernel on the same records bit for bit.

The largest error / bound ratio per bounded kernel is printed at the end of the module with -s.  On MI355X (136 rows, 2.8 s with the
references; every row passed the first time it ran, no kernel or threshold needed a change):
  box_transform       0.451     views.clean         0.383     views.noisy         0.479
  scaler.clip_stats   0.495     scaler.acc          0.349     mixup.mode0         0.734
The np.float32 restatements of tests/test_input_check_cpu.py give 0.451, 0.326, 0.479, 0.495, 0.349 and 0.957: the worst elements are
those of the mean fill and the f32 square, which the restatement rounds like the kernel; mixup's mode 0 is contracted on the device (one
rounding fewer).  The label merge and the query patches are exact.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import input_cases as IC
import input_check as K

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L
    assert torch.cuda.is_available()
    lib = L.load()
    t0 = time.time()
    yield L, lib
    if RATIOS:
        print('\nlargest error / bound ratio per kernel:')
        for k in sorted(RATIOS):
            print(f'  {k:24s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - t0:.1f} s')


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def up(fr):
    """the frames' images on the device"""
    return {n: torch.from_numpy(f.buf.copy()).cuda() for n, f in fr.items()}


def own(t, f, *shape):
    """the owned elements of an uploaded frame as a tensor view"""
    v = t[K.GUARD:K.GUARD + f.n]
    return v.view(*shape) if shape else v


def ptr(t, f=None):
    """address of a tensor's first element, or of the first owned element of an uploaded frame"""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + (K.GUARD * f.dtype.itemsize if f is not None else 0))


def down(d):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in d.items()}


def finish(key, c, inp, fr, d):
    for n, r in K.KERNELS[key].verify(c, inp, fr, down(d)).items():
        RATIOS[n] = max(RATIOS[n], r)


def refused(L, c, fr, d, call):
    with L.launch_log() as log:
        with pytest.raises(RuntimeError):
            call()
    assert sum(log.values()) == 0, dict(log)
    img = down(d)
    for n, f in fr.items():
        K.exact(img[n], f.buf, f'{c["name"]}.{n} after the refused call')


def _box_transform_c(L, lib, c, amp, recs, mean, std, out_ptr):
    L.check(lib.sedt_box_transform(ptr(amp), IC.raw_stride(c), ptr(recs), ptr(mean), ptr(std), recs.shape[0], c['frames'], c['F'], c['log'],
                                   c.get('fill_mean', 1), float(c.get('fill_const', 0.0)), out_ptr, L.stream_ptr()), 'box_transform')


@pytest.mark.parametrize('c', IC.BOX_TRANSFORM, ids=lambda c: c['name'])
def test_box_transform(env, c):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform, _AUG
    L, lib = env
    k = K.KERNELS['box_transform']
    inp = k.make(c)
    fr = k.frames(c, inp)
    d = up(fr)
    B, frames, F = len(c['recs']), c['frames'], c['F']
    amp = dev(inp['amp'])

    def call():
        if c['via'] == 'ops':
            tf = DeviceBoxTransform(frames, inp['mean'], inp['std'], apply_log=bool(c['log']), n_mels=F)
            tf(amp, params=inp['recs'].view(_AUG).reshape(-1), out=own(d['out'], fr['out'], B, 1, frames, F), nframes=[r[0] for r in c['recs']])
        else:
            _box_transform_c(L, lib, c, amp, dev(inp['recs']), dev(inp['mean']), dev(inp['std']), ptr(d['out'], fr['out']))
    if c.get('refuse'):
        return refused(L, c, fr, d, call)
    call()
    finish('box_transform', c, inp, fr, d)


@pytest.mark.parametrize('c', IC.BOX_TRANSFORM_VIEWS, ids=lambda c: c['name'])
def test_box_transform_views(env, c):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceViewTransform, _VAUG
    L, lib = env
    k = K.KERNELS['box_transform_views']
    inp = k.make(c)
    fr = k.frames(c, inp)
    d = up(fr)
    B, frames, F = len(c['recs']), c['frames'], c['F']
    amp, mean, std = dev(inp['amp']), dev(inp['mean']), dev(inp['std'])
    z = None if c.get('drawn') else dev(inp['z'])

    def call():
        if c['via'] == 'ops':
            tf = DeviceViewTransform(frames, inp['mean'], inp['std'], noise_snr=K.SNR, apply_log=bool(c['log']), n_mels=F,
                                     noise='device' if c.get('drawn') else 'host', seed=c.get('seed', 0))
            tf.offset = c.get('offset', 0)
            tf(amp, params=inp['recs'].view(_VAUG).reshape(-1), normals=z, nframes=[q[0][0] for q in c['recs']],
               out=(own(d['out0'], fr['out0'], B, 1, frames, F), own(d['out1'], fr['out1'], B, 1, frames, F)))
            assert tf.offset == c.get('offset', 0) + (B * IC.raw_stride(c) * F if c.get('drawn') else 0)
        else:
            L.check(lib.sedt_box_transform_views(ptr(amp), IC.raw_stride(c), ptr(dev(inp['recs'])), ptr(mean), ptr(std), B, frames, F, c['log'],
                                                 c.get('fill_mean', 1), float(c.get('fill_const', 0.0)), K.SNR, ptr(z), 0, None, 0,
                                                 ptr(d['out0'], fr['out0']), ptr(d['out1'], fr['out1']), L.stream_ptr()), 'box_transform_views')
    if c.get('refuse'):
        return refused(L, c, fr, d, call)
    call()
    img = down(d)
    for n, r in k.verify(c, inp, fr, img).items():
        RATIOS[n] = max(RATIOS[n], r)
    # view 0 and every clean view 1 are the single-view kernel's bits
    for v, clips, recs in k.single_view_rows(c, inp):
        if not clips:
            continue
        one = torch.full((len(clips), frames, F), float('nan'), device='cuda')
        _box_transform_c(L, lib, c, amp[clips].contiguous(), dev(recs), mean, std, ptr(one))
        torch.cuda.synchronize()
        got = fr[f'out{v}'].own(img[f'out{v}']).reshape(B, frames, F)[clips]
        K.exact(got, one.cpu().numpy(), f'{c["name"]} view {v} against the single-view kernel')


@pytest.mark.parametrize('c', IC.SCALER, ids=lambda c: c['name'])
def test_scaler_update(env, c):
    L, lib = env
    k = K.KERNELS['scaler_update']
    inp = k.make(c)
    fr = k.frames(c, inp)
    d = up(fr)
    F, stride = c['F'], IC.raw_stride(c)

    def update(amp, nf, stats, acc, count):
        amp, nf = dev(amp), dev(nf)
        L.check(lib.sedt_scaler_update(ptr(amp), stride, ptr(nf), len(nf), c['frames'], F, c['log'], ptr(d[stats], fr[stats]), ptr(d[acc], fr[acc]),
                                       ptr(d[count], fr[count]), L.stream_ptr()), 'scaler_update')
        torch.cuda.synchronize()

    def call():
        for i, q in enumerate(inp['calls']):
            update(q['amp'], q['nf'], f'stats{i}', 'acc', 'count')
        update(np.concatenate([q['amp'] for q in inp['calls']]), np.concatenate([q['nf'] for q in inp['calls']]), 'stats_cat', 'acc_cat', 'count_cat')
    if c.get('refuse'):
        return refused(L, c, fr, d, call)
    call()
    finish('scaler_update', c, inp, fr, d)


@pytest.mark.parametrize('c', IC.MIXUP, ids=lambda c: c['name'])
def test_mixup(env, c):
    from sound_event_detection_transformer_amd import ops
    L, lib = env
    k = K.KERNELS['mixup']
    inp = k.make(c)
    fr = k.frames(c, inp)
    d = up(fr)
    x1, x2 = dev(inp['x1']), dev(inp['x2'])
    n, elems = len(c['jobs']), 4 * c['clip4'] + c['rem']
    jobs = torch.from_numpy(np.concatenate([inp['jobs'].view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).cuda()

    def call():
        if c['via'] == 'ops':
            ops.mixup(x1, x2, jobs[:16 * n], out=own(d['out'], fr['out'], n, elems))
        else:
            L.check(lib.sedt_mixup(ptr(x1), ptr(x2), ptr(jobs), n, elems, ptr(d['out'], fr['out']), L.stream_ptr()), 'mixup')
    if c.get('refuse'):
        return refused(L, c, fr, d, call)
    with L.launch_log() as log:
        call()
    assert log['mixup'] == 1
    finish('mixup', c, inp, fr, d)


@pytest.mark.parametrize('c', IC.MIXUP_TARGETS, ids=lambda c: c['name'])
def test_mixup_targets(env, c):
    L, lib = env
    k = K.KERNELS['mixup_targets']
    inp = k.make(c)
    fr = k.frames(c, inp)
    d = up(fr)
    t = {n: dev(inp[n]) for n in ('lab1', 'lab_off1', 'box1', 'box_off1', 'ratio1', 'split1', 'lab2', 'lab_off2', 'box2', 'box_off2', 'lam')}
    ro = ptr(d['ratio_out'], fr['ratio_out']) if 'ratio_out' in fr else None
    L.check(lib.sedt_mixup_targets(ptr(t['lab1']), ptr(t['lab_off1']), ptr(t['box1']), ptr(t['box_off1']), ptr(t['ratio1']), ptr(t['split1']),
                                   c['B1'], c['ns1'], ptr(t['lab2']), ptr(t['lab_off2']), ptr(t['box2']), ptr(t['box_off2']), c['B2'], ptr(t['lam']),
                                   c['mix_num'], c['max_events'], ptr(d['lab_out'], fr['lab_out']), ptr(d['lab_off_out'], fr['lab_off_out']),
                                   ptr(d['box_out'], fr['box_out']), ptr(d['box_off_out'], fr['box_off_out']), ro, inp['cap'],
                                   ptr(d['jobs'], fr['jobs']), L.stream_ptr()), 'mixup_targets')
    finish('mixup_targets', c, inp, fr, d)


@pytest.mark.parametrize('c', IC.QUERY, ids=lambda c: c['name'])
def test_query_patches(env, c):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceQuery
    L, lib = env
    k = K.KERNELS['query_patches']
    inp = k.make(c)
    fr = k.frames(c, inp)
    d = up(fr)
    data = dev(inp['data'])
    n = len(c['jobs'])
    jobs = dev(np.concatenate([inp['jobs'], np.zeros((1, 4), np.int32)]))

    def call():
        L.check(lib.sedt_query_patches(ptr(data), c['B'], c['T'], c['F'], ptr(jobs), n, c['fixed'], ptr(d['out'], fr['out']), L.stream_ptr()),
                'query_patches')
    if c.get('refuse'):
        return refused(L, c, fr, d, call)
    if c['via'] == 'ops':                                    # the class allocates its own output: (B, P, 1, 128, F), clip-major like the jobs
        boxes = [[K.box_of_rows(s, e, c['T']) for b, s, e in c['jobs'] if b == i] for i in range(c['B'])]
        out = DeviceQuery(bool(c['fixed']))(data[:, None], [np.stack(b) for b in boxes])
        own(d['out'], fr['out']).copy_(out.reshape(-1))
    else:
        call()
    finish('query_patches', c, inp, fr, d)
