"""GPU: sedt_reverb / sedt_reverb_spectra (csrc/reverb.hip) stage by stage against tests/reverb_ref.py, and the public stage
utilities.reverb.DeviceReverb.

Every row of tests/reverb_cases.py runs once on the device, with guards around the bank, the destination, the workspace and the
spectra, and is read back whole: H against the float64 partition spectra of h, X against the float64 block spectra of the faded x, the
wet row against the float64 products and inverse applied to the DEVICE's X and H - each within its bound (tests/reverb_ref.py derives
the forms; DESIGN.md quotes the measured ratios behind the constants).  End to end, against the direct form np.convolve in float64,
the device may miss by 8 times what the float32 restatement misses by on the same input - the factor of the stretch tests."""
import functools

import numpy as np
import pytest
import torch

import reverb_cases as K
import reverb_ref as R

pytestmark = pytest.mark.gpu

G = 64                                                      # guard floats on every side
ROWS = list(range(len(K.ROWS)))


def _reverb(N, responses):
    """a DeviceReverb over ``responses`` (staged as they are) whose spectra lie between guards: (stage, guarded re, guarded im)"""
    from sound_event_detection_transformer_amd.utilities.reverb import DeviceReverb

    class Guarded(DeviceReverb):
        def _alloc_spectra(self, n_parts, Kb):
            self.raw = [torch.full((n_parts * Kb + 2 * G,), -7.0, dtype=torch.float32, device='cuda') for _ in range(2)]
            return tuple(r[G:G + n_parts * Kb].view(n_parts, Kb) for r in self.raw)

    rv = Guarded(16000, N).add_rirs(list(responses), normalize=None)
    for raw in rv.raw:
        host = raw.cpu().numpy()
        assert (host[:G] == -7.0).all() and (host[-G:] == -7.0).all()
    return rv


def _launch(rows, mutate=None, group=None):
    """the rows (all of one n_fft), each with its own response, as ONE call through DeviceReverb.launch, everything guarded: dict of
    host arrays.  ``mutate`` changes the DEVICE copy of the records only: the entry point sees the sound ones."""
    from sound_event_detection_transformer_amd.utilities import reverb as M
    N = K.ROWS[rows[0]][0]
    rv = _reverb(N, [K.response(r) for r in rows])
    xs = [K.signal(r) for r in rows]
    jobs, floats = M.reverb_jobs([len(x) for x in xs], list(range(len(rows))), rv.rir_lens, N, fades=[K.ROWS[r][3] for r in rows])
    jobs['src_off'] += G
    jobs['dst_off'] += G
    totals = [len(x) + len(K.response(r)) - 1 for x, r in zip(xs, rows)]
    room = int(jobs['dst_off'][-1]) + totals[-1] + G
    dev_jobs = jobs.copy()
    if mutate is not None:
        mutate(dev_jobs)
    bank = np.concatenate([np.full(G, 3.0, np.float32)] + xs + [np.full(G, 3.0, np.float32)])
    flat = torch.from_numpy(bank).cuda()
    dst = torch.full((room,), -7.0, dtype=torch.float32, device='cuda')
    ws = torch.full((floats + G,), -7.0, dtype=torch.float32, device='cuda')
    status = torch.full((len(rows),), -9, dtype=torch.int32, device='cuda')
    rv.launch(flat, jobs, dst, ws[:max(floats, 4)], status=status, jobs_dev=torch.from_numpy(dev_jobs.view(np.uint8).copy()).cuda(),
              group=group)
    out = dict(jobs=jobs, floats=floats, totals=totals, dst=dst.cpu().numpy(), ws=ws.cpu().numpy(), status=status.cpu().numpy(),
               H=[rv.spectra(i) for i in range(len(rows))], h_raw=[r.cpu().numpy() for r in rv.raw])
    assert flat.cpu().numpy().tobytes() == bank.tobytes()
    assert (out['ws'][floats:] == -7.0).all()               # nothing behind the workspace is written
    for raw in out['h_raw']:                                # ... or around the spectra
        assert (raw[:G] == -7.0).all() and (raw[-G:] == -7.0).all()
    return out


def _parts(out, e, N):
    """(X, wet) of job e as the device left them"""
    from sound_event_detection_transformer_amd.utilities import reverb as M
    job = out['jobs'][e]
    reg = M.regions(job, N)
    get = lambda name: out['ws'][reg[name][0]:reg[name][0] + int(np.prod(reg[name][1]))].reshape(reg[name][1])
    X = get('X_re').astype(np.float64) + 1j * get('X_im').astype(np.float64)
    return X, out['dst'][int(job['dst_off']):int(job['dst_off']) + out['totals'][e]]


@functools.lru_cache(maxsize=None)
def _run(row):
    out = _launch([row])
    assert out['status'].tolist() == [0]
    assert (out['dst'][:G] == -7.0).all() and (out['dst'][G + out['totals'][0]:] == -7.0).all()      # the guards of the destination
    X, wet = _parts(out, 0, K.ROWS[row][0])
    return out['H'][0], X, wet


def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def _stage_ratios(row):
    """{stage: largest error / bound} of the device on one row, each stage against float64 from the device's own input to it"""
    N, n, L, fade, _, _ = K.ROWS[row]
    nb, P, nout, total = R.counts(n, L, N)
    x, h, ref = K.signal(row), K.response(row), K.reference(row)
    H, X, wet = _run(row)
    assert H.shape == (P, N // 2 + 1) and X.shape == (nb, N // 2 + 1) and wet.shape == (total,)
    return {'spectra': _ratio(np.abs(H - ref['H']).max(axis=1), R.spectra_bound(h, N)),
            'blocks': _ratio(np.abs(X - ref['X']).max(axis=1), R.blocks_bound(x, fade, N)),
            'wet': _ratio(np.abs(wet - R.mac_inverse(X, H, n, L, N)), R.wet_bound(X, H, n, L, N))}


@pytest.mark.parametrize('row', ROWS)
def test_every_stage_against_float64(row):
    e = _stage_ratios(row)
    print('stage ratios', K.ROWS[row], {k: round(v * c, 4) for (k, v), c in zip(e.items(), (R.C_H, R.C_X, R.C_Y))}, '(constants at 1)')
    assert all(v <= 1.0 for v in e.values()), e


@pytest.mark.parametrize('row', ROWS)
def test_end_to_end_against_the_direct_form(row):
    want = K.reference(row)['direct']
    wet = _run(row)[2]
    yard, err = float(np.abs(K.restatement(row) - want).max(initial=0.0)), float(np.abs(wet - want).max(initial=0.0))
    print('end to end', K.ROWS[row], f'float32 restatement {yard:.3e} device {err:.3e} ratio {err / yard if yard else 0.0:.3f}')
    assert err <= 8.0 * yard, (err, yard)


MULTI = [4, 9, 13, 16, 20]                                   # five jobs at n_fft 512, five different responses


def test_bad_device_records_raise_only_their_own_status():
    """job 1's DEVICE record is moved out of the destination, job 3's names a response outside the table: both get status 2, nothing of
    theirs is touched, and the other jobs are what they are on their own"""
    def mutate(jobs):
        jobs['dst_off'][1] += 10 ** 7
        jobs['rir'][3] = 99
    out = _launch(MULTI, mutate=mutate)
    assert out['status'].tolist() == [0, 2, 0, 2, 0]
    for e in (0, 2, 4):
        H, X, wet = _run(MULTI[e])
        Xe, wete = _parts(out, e, 512)
        assert np.array_equal(Xe, X) and np.array_equal(wete, wet) and np.array_equal(out['H'][e], H)
    for e in (1, 3):
        job, nxt = out['jobs'][e], out['jobs'][e + 1]
        assert (out['ws'][int(job['ws_off']):int(nxt['ws_off'])] == -7.0).all()
        assert (out['dst'][int(job['dst_off']):int(nxt['dst_off'])] == -7.0).all()
    for field, value in (('src_off', 10 ** 7), ('ws_off', 10 ** 9), ('n', 2 ** 26 + 1), ('rir', -1), ('fade', -1), ('ws_off', 2)):
        def one(jobs, field=field, value=value):
            jobs[field][2] = value
        assert _launch(MULTI[:3], mutate=one)['status'].tolist() == [0, 0, 2], field


def test_two_calls_give_the_same_bits_whatever_the_group():
    a, b = _launch(MULTI), _launch(MULTI)
    assert a['status'].tolist() == [0] * 5
    assert a['ws'].tobytes() == b['ws'].tobytes() and a['dst'].tobytes() == b['dst'].tobytes()
    for group in (1, 2, 4, 8):
        c = _launch(MULTI, group=group)
        assert c['status'].tolist() == [0] * 5 and c['dst'].tobytes() == a['dst'].tobytes(), group
    for row in (23, 24):                                     # ... at the two longer frames as well
        wet = _run(row)[2]
        for group in (1, 2, 8):
            out = _launch([row], group=group)
            assert np.array_equal(_parts(out, 0, K.ROWS[row][0])[1], wet), (row, group)


def _abi(rv, flat, jobs, jobs_dev, dst, ws, ws_bytes, status, n_fft=None, E=None, null=None, group=0, table=None):
    from sound_event_detection_transformer_amd import lib as L
    table = rv.table if table is None else table
    args = [L.p(flat), flat.numel(), jobs.ctypes.data, L.p(jobs_dev), len(jobs) if E is None else E, L.p(dst), dst.numel(), L.p(ws), ws_bytes,
            L.p(rv.h_re), L.p(rv.h_im), rv.n_parts, table.ctypes.data, L.p(rv._table_dev), len(rv.rirs), L.p(rv._twiddle),
            rv.n_fft if n_fft is None else n_fft, group, L.p(status), L.stream_ptr()]
    if null is not None:
        args[null] = None
    return L.load().sedt_reverb(*args), L.load().sedt_last_error().decode()


def test_refusals_launch_nothing():
    from sound_event_detection_transformer_amd.utilities import reverb as M
    x, h = K.signal(13), K.response(13)
    rv = _reverb(512, [h])
    jobs, floats = M.reverb_jobs([len(x)], [0], rv.rir_lens, 512, fades=[16])
    flat = torch.from_numpy(np.array(x)).cuda()
    dst = torch.full((len(x) + len(h) - 1,), -7.0, dtype=torch.float32, device='cuda')
    ws = torch.full((floats,), -7.0, dtype=torch.float32, device='cuda')
    status = torch.full((1,), -9, dtype=torch.int32, device='cuda')
    dev = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()

    def refused(match, jobs_=jobs, **kw):
        rc, msg = _abi(rv, flat, jobs_, dev, dst, ws, kw.pop('ws_bytes', 4 * floats), status, **kw)
        assert rc != 0 and match in msg, (rc, msg)

    refused('is too small', ws_bytes=4 * floats - 1)
    refused('n_fft=256', n_fft=256)
    refused('negative', E=-1)
    refused('group=3', group=3)
    for i in (0, 2, 3, 5, 7, 9, 10, 12, 13, 15, 18):
        refused('null pointer', null=i)
    for field, value, match in (('n', 0, 'n >= 1'), ('n', 2 ** 26 + 1, 'outside the envelope'), ('fade', -1, 'outside the envelope'),
                                ('rir', 1, 'names response'), ('rir', -1, 'names response'), ('ws_off', 2, 'ws_off')):
        bad = jobs.copy()
        bad[field][0] = value
        refused(match, jobs_=bad)
    for r, c, value, match in ((0, 0, 0, 'taps'), (0, 0, 176 * 256 + 1, 'taps'), (1, 0, 1, 'partitions lie behind')):
        table = rv.table.copy()
        table[r][c] = value
        refused(match, table=table)
    torch.cuda.synchronize()
    assert (dst.cpu() == -7.0).all() and (ws.cpu() == -7.0).all() and status.cpu().tolist() == [-9]
    rc, msg = _abi(rv, flat, jobs, dev, dst, ws, 4 * floats, status, E=0)                   # no job: nothing to do, nothing launched
    assert rc == 0 and (dst.cpu() == -7.0).all() and status.cpu().tolist() == [-9]
    rc, msg = _abi(rv, flat, jobs, dev, dst, ws, 4 * floats, status)
    assert rc == 0 and status.cpu().tolist() == [0] and not (dst.cpu() == -7.0).any()


def test_device_reverb_on_a_resampled_response():
    """the public stage: a response staged from 32 kHz is resampled to the stage's rate on the device and normalised to unit energy on
    the host; sounds of different lengths in one call, zeros behind each"""
    from sound_event_detection_transformer_amd.utilities.reverb import DeviceReverb
    gen = np.random.default_rng(12)
    raw = (gen.standard_normal(1200) * np.exp(-5.0 * np.arange(1200) / 1200)).astype(np.float32)
    rv = DeviceReverb(16000, 512, resample_quality='kaiser_fast')
    rv.add_rirs([raw], sample_rates=32000).add_rirs([np.asarray([0, 16384, 0], np.int16)], normalize=None)
    assert len(rv) == 2 and rv.rir_lens == [rv.resampler(32000).n_out(1200), 3] and rv.rirs[1].tolist() == [0.0, 0.5, 0.0]
    h = rv.rirs[0]
    assert h.dtype == np.float32 and abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    want_h = rv.resampler(32000)([torch.from_numpy(raw)])[0].cpu().numpy().reshape(-1)[:len(h)].astype(np.float64)
    assert np.allclose(h, want_h / np.sqrt(np.sum(want_h * want_h)), rtol=0, atol=1e-6)
    xs = [K.signal(20), K.signal(13), torch.from_numpy(np.array(K.signal(16))).cuda()]
    out, ms = rv.rv(xs, [0, 1, 0], fades=[16, 0, 5])
    rv.check(rv.last_status)
    host = out.cpu().numpy()
    assert ms == [3000 + len(h) - 1, 602, 600 + len(h) - 1] and out.shape == (3, max(ms))
    for e, (x, r, fade) in enumerate(zip((K.signal(20), K.signal(13), K.signal(16)), (0, 1, 0), (16, 0, 5))):
        want = R.direct(x, rv.rirs[r], fade)
        yard = float(np.abs(R.chain(x, rv.rirs[r], fade, 512, np.float32)['wet'] - want).max())
        err = float(np.abs(host[e, :ms[e]] - want).max())
        print('DeviceReverb sound', e, f'float32 restatement {yard:.3e} device {err:.3e}')
        assert err <= 8.0 * yard and not host[e, ms[e]:].any()
    assert rv.read(1, 'X_re').shape == (4, 257)
    with pytest.raises(ValueError, match='names response 2 of 2'):
        rv.rv(xs[:1], 2)
