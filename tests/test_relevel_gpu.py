"""GPU: sedt_relevel (csrc/relevel.hip) through the ctypes ABI against tests/relevel_ref.py and against the entry points it shares its
arithmetic with, the public stage utilities.relevel.DeviceRelevel, and the ``relevel`` mode of SoundscapeClips.

Cases (tests/relevel_cases.py; tests/test_relevel_cpu.py checks on the reference alone that no block lies within 1e-6 of a gate
threshold): 16 kHz (H = 1600); regions of 1, 255, 256, 257, H - 1, H, 4H - 1, 4H, 4H + 1, 6H + 3 and 257H + 3 samples (a second round of
hops) at offsets 0 .. 3 mod 4; 1, 3 and 270 jobs; stepped noise, noise, zeros, noise under the absolute gate, noise on a DC offset.
Every run sits between guards of 64 floats around flat, the workspace, the records and the outputs.

Bounds.  level and counts: bit-identical to sedt_bank_stats (sumsq / n) and to sedt_loudness on the same regions as a source table, and
within the 1e-10 relative of the float64 reference that tests/test_loudness_gpu.py holds zbar to (its docstring derives it).  Gains:
within ONE float32 ulp of float32(target / sqrt(level_ref)) - the float64 chain errs by <= 1e-10 relative, far below half a float32
ulp (3e-8), so the two roundings can only land on neighbours.  End to end: the mixed event measures within 1e-4 dB / LU of its
target_db (the figure tests/test_loudness_gpu.py uses after a normalisation: the float32 gain and products bound the error near 1e-6)."""
import numpy as np
import pytest
import torch

import relevel_cases as K
import relevel_ref as R
import reverb_ref as RV
import soundscape_ref as S

pytestmark = pytest.mark.gpu

SR, H = K.SR, K.H
GUARD = np.full(64, -7.0, np.float32).view(np.uint8)
LABELS = [f'c{i}' for i in range(10)]


class Guarded(object):
    """host bytes on the device between two guards of 64 floats; the data starts 256 bytes into a fresh allocation"""

    def __init__(self, host):
        raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        self.n, self.pad = raw.size, -raw.size % 8
        self.buf = torch.from_numpy(np.concatenate([GUARD, raw, np.zeros(self.pad, np.uint8), GUARD])).cuda()

    @property
    def data(self):
        return self.buf[GUARD.size:GUARD.size + self.n]

    def view(self, dtype):
        return self.data.view(dtype)

    def read(self, dtype):
        return self.data.cpu().numpy().view(dtype).copy()

    def intact(self):
        b = self.buf.cpu().numpy()
        return b[:GUARD.size].tobytes() == GUARD.tobytes() == b[GUARD.size + self.n + self.pad:].tobytes()


def _records(E, gen):
    """(EVENT [E + 2], TAIL [(E + 1) // 2 + 1]) of arbitrary bytes with recognisable gains, and each job's record indices: the events
    in reverse order, every second job with a tail"""
    from sound_event_detection_transformer_amd.utilities.reverb import TAIL
    from sound_event_detection_transformer_amd.utilities.soundscape import EVENT
    ev = gen.integers(0, 255, (E + 2) * EVENT.itemsize, dtype=np.uint8).view(EVENT).copy()
    tails = gen.integers(0, 255, ((E + 1) // 2 + 1) * TAIL.itemsize, dtype=np.uint8).view(TAIL).copy()
    ev['gain'] = 0.25 + np.arange(E + 2, dtype=np.float32)
    tails['gain'] = -0.5 - np.arange(len(tails), dtype=np.float32)
    return ev, tails, (E - np.arange(E)).astype(np.int64), np.where(np.arange(E) % 2 == 0, np.arange(E) // 2, -1).astype(np.int64)


def _run(flat, jobs, mode, ev, tails, jobs_dev=None, work_len=None):
    """one sedt_relevel call through the ABI between guards: dict of host arrays level, counts, status, ev, tails, work"""
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities import loudness as LD
    from sound_event_detection_transformer_amd.utilities import relevel as M
    E = len(jobs)
    sized = jobs if jobs_dev is None else jobs_dev                  # (a faulty host copy comes with the sound records as jobs_dev)
    doubles = int(sized['ws_off'][-1]) + M.job_doubles(sized['n'][-1], H if mode else None)
    assert doubles == L.load().sedt_relevel_workspace(sized.ctypes.data, E, mode, H)
    g = dict(flat=Guarded(flat), jobs=Guarded(jobs if jobs_dev is None else jobs_dev), ev=Guarded(ev), tails=Guarded(tails),
             work=Guarded(np.full(max(doubles, 1), -7.0, np.float64)), level=Guarded(np.full(E, -7.0, np.float64)),
             counts=Guarded(np.full((E, 4), -9, np.int32)), status=Guarded(np.full(E, -9, np.int32)),
             consts=Guarded(np.concatenate([LD.k_weighting(SR), LD.hop_map(SR).reshape(-1)])))
    consts = g['consts'].view(torch.float64)
    L.check(L.load().sedt_relevel(L.p(g['flat'].data), len(flat), jobs.ctypes.data, L.p(g['jobs'].data), E, mode, L.p(consts), L.p(consts[10:]),
                                  H, LD.Z_ABS, L.p(g['work'].data), doubles if work_len is None else work_len, L.p(g['ev'].data), len(ev),
                                  L.p(g['tails'].data), len(tails), L.p(g['level'].data), L.p(g['counts'].data), L.p(g['status'].data),
                                  L.stream_ptr()), 'relevel')
    torch.cuda.synchronize()
    assert all(v.intact() for v in g.values()), [k for k, v in g.items() if not v.intact()]
    assert g['flat'].read(np.float32).tobytes() == flat.tobytes() and g['jobs'].read(np.uint8).tobytes() == (jobs if jobs_dev is None else jobs_dev).tobytes()
    return dict(level=g['level'].read(np.float64), counts=g['counts'].read(np.int32).reshape(E, 4), status=g['status'].read(np.int32),
                ev=g['ev'].read(ev.dtype), tails=g['tails'].read(tails.dtype), work=g['work'].read(np.float64)[:doubles])


def _tables(flat, offs, ns):
    return torch.from_numpy(np.array(flat)).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(ns).cuda()      # (flat is read-only)


def _bank_stats(flat, offs, ns):
    from sound_event_detection_transformer_amd import lib as L
    d_flat, d_off, d_len = _tables(flat, offs, ns)
    sumsq, peak = torch.zeros(len(ns), dtype=torch.float64, device='cuda'), torch.zeros(len(ns), dtype=torch.float32, device='cuda')
    L.check(L.load().sedt_bank_stats(L.p(d_flat), len(flat), L.p(d_off), L.p(d_len), len(ns), L.p(sumsq), L.p(peak), L.stream_ptr()), 'bank_stats')
    return sumsq.cpu().numpy()


def _loudness(flat, offs, ns):
    from sound_event_detection_transformer_amd.utilities.loudness import DeviceLoudness
    d_flat, d_off, d_len = _tables(flat, offs, ns)
    zbar, counts = DeviceLoudness(SR).launch(d_flat, len(flat), d_off, d_len, ns.tolist())
    return zbar.cpu().numpy(), counts.cpu().numpy()


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _unchanged(got, host, skip):
    """the records of ``got`` are ``host``'s bit for bit, the gains of the records in ``skip`` aside"""
    a, b = got.copy(), host.copy()
    a['gain'][list(skip)] = b['gain'][list(skip)] = 0
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('n_jobs', K.N_JOBS)
def test_levels_and_gains_against_the_entry_points_and_the_reference(n_jobs, mode):
    from sound_event_detection_transformer_amd.utilities import relevel as M
    flat, offs, ns = K.layout(n_jobs)
    ref = K.reference(n_jobs, mode)
    ev, tails, ev_idx, tail_idx = _records(n_jobs, np.random.default_rng(n_jobs))
    targets = M.target_amplitude([K.target_db(i) for i in range(n_jobs)], mode)
    jobs, _ = M.relevel_jobs(offs, ns, targets, ev=ev_idx, tails=tail_idx, hop=H if mode == 'lufs' else None)
    got = _run(flat, jobs, M.MODES[mode], ev, tails)
    # ---- level and counts: the bits of the existing entry points on the same regions
    if mode == 'rms':
        assert got['level'].tobytes() == (_bank_stats(flat, offs, ns) / ns.astype(np.float64)).tobytes()
        assert got['counts'].tolist() == [[int(n), 0, 0, 0] for n in ns]
    else:
        zbar, counts = _loudness(flat, offs, ns)
        assert got['level'].tobytes() == zbar.tobytes() and got['counts'].tobytes() == counts.tobytes()
    # ---- ... and the float64 reference
    worst, worst_ulp, written_ev, written_tail = 0.0, 0, set(), set()
    for i, m in enumerate(ref):
        assert got['counts'][i].tolist() == m['counts'] and got['status'][i] == m['status'], (i, got['counts'][i], got['status'][i], m['counts'])
        if m['level'] == 0.0:
            assert got['level'][i] == 0.0
            continue
        worst = max(worst, abs(got['level'][i] - m['level']) / m['level'])
        written_ev.add(int(ev_idx[i]))
        d = _ulps(got['ev']['gain'][ev_idx[i]], m['gain'])
        if tail_idx[i] >= 0:
            written_tail.add(int(tail_idx[i]))
            assert got['tails']['gain'][tail_idx[i]].tobytes() == got['ev']['gain'][ev_idx[i]].tobytes()
        worst_ulp = max(worst_ulp, d)
    print(f'{n_jobs} jobs, {mode}: worst relative error of the level {worst:.3e}, worst gain distance {worst_ulp} ulp')
    assert worst < 1e-10 and worst_ulp <= 1
    # ---- every other byte of the records is the host's: status 1 and unnamed records included
    assert _unchanged(got['ev'], ev, written_ev) and _unchanged(got['tails'], tails, written_tail)
    assert len(written_ev) == sum(m['status'] == 0 for m in ref) and (n_jobs < 270 or 0 < len(written_ev) < n_jobs)
    # ---- two calls into the same kind of buffers: the same bytes
    again = _run(flat, jobs, M.MODES[mode], ev, tails)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_silent_quiet_and_non_finite_regions_raise_status_1():
    from sound_event_detection_transformer_amd.utilities import relevel as M
    gen = np.random.default_rng(12)
    parts = [np.zeros(5 * H + 1, np.float32), K.LC.content('quiet', 6 * H + 3, gen), K.LC.content('noise', 5 * H, gen),
             K.LC.content('noise', 5 * H + 2, gen), K.LC.content('noise', 300, gen)]
    parts[2][2 * H + 5] = np.nan
    parts[3][7] = np.inf
    ns = np.asarray([len(x) for x in parts], np.int64)
    offs = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64) + 1
    flat = np.concatenate([[GUARD.view(np.float32)[0]]] + parts).astype(np.float32)
    for mode in R.MODES:
        ev, tails, ev_idx, tail_idx = _records(5, gen)
        jobs, _ = M.relevel_jobs(offs, ns, [0.05] * 5, ev=ev_idx, tails=[0, 1, 2, -1, 3], hop=H if mode == 'lufs' else None)
        got = _run(flat, jobs, M.MODES[mode], ev, tails)
        quiet_ok = mode == 'rms'                                                            # noise at 1e-5 has an RMS, but no loudness
        assert got['status'].tolist() == [1, 0 if quiet_ok else 1, 1, 1, 0], (mode, got['status'])
        assert got['level'][0] == 0.0 and not np.isfinite(got['level'][2]) and not np.isfinite(got['level'][3]) and got['level'][4] > 0
        named_ev = {int(ev_idx[i]) for i in ((1, 4) if quiet_ok else (4,))}
        named_tails = {1, 3} if quiet_ok else {3}
        assert _unchanged(got['ev'], ev, named_ev) and _unchanged(got['tails'], tails, named_tails)
        want = R.gain(0.05, R.level(parts[4], SR, mode)['level'])[1]
        assert _ulps(got['ev']['gain'][ev_idx[4]], want) <= 1 and got['tails']['gain'][3] == got['ev']['gain'][ev_idx[4]]


def test_device_records_are_checked_again_and_the_entry_point_refuses():
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities import relevel as M
    gen = np.random.default_rng(13)
    ns = np.asarray([H, 4 * H + 1, 257, 6 * H + 3, 255], np.int64)
    offs = np.concatenate([[0], np.cumsum(ns + 3)[:-1]]).astype(np.int64) + 2
    flat = (0.05 * gen.standard_normal(int(offs[-1] + ns[-1]) + 9)).astype(np.float32)
    for mode in R.MODES:
        ev, tails, ev_idx, tail_idx = _records(5, gen)
        jobs, doubles = M.relevel_jobs(offs, ns, [0.1] * 5, ev=ev_idx, tails=tail_idx, hop=H if mode == 'lufs' else None)
        clean = _run(flat, jobs, M.MODES[mode], ev, tails)
        assert clean['status'].tolist() == [0] * 5
        bad = jobs.copy()
        bad['off'][1] = len(flat) - ns[1] + 1                                               # one sample past the end of flat
        bad['ev'][3] = len(ev)                                                              # one record past the end of the table
        got = _run(flat, jobs, M.MODES[mode], ev, tails, jobs_dev=bad)
        assert got['status'].tolist() == [0, 2, 0, 2, 0]
        for i in (1, 3):                                                                    # nothing is written for them
            assert got['level'][i] == -7.0 and got['counts'][i].tolist() == [-9] * 4
            assert got['ev'][ev_idx[i]].tobytes() == ev[ev_idx[i]].tobytes()
        assert got['tails'][tail_idx[2]].tobytes() == clean['tails'][tail_idx[2]].tobytes()
        for i in (0, 2, 4):                                                                 # the others as in the clean call
            assert got['level'][i] == clean['level'][i] and got['ev'][ev_idx[i]].tobytes() == clean['ev'][ev_idx[i]].tobytes()
        if mode == 'lufs':                                                                  # the refused jobs' doubles of the workspace too
            lo1, lo3 = int(jobs['ws_off'][1]), int(jobs['ws_off'][3])
            assert (got['work'][lo1:int(jobs['ws_off'][2])] == -7.0).all() and (got['work'][lo3:int(jobs['ws_off'][4])] == -7.0).all()
            assert got['work'][0] != -7.0
        # ---- the same faults in jobs_host: refused before any launch, nothing written
        for fault, match in ((dict(off=bad['off'][1]), 'job 1 .* does not lie inside'), (dict(ev=len(ev)), f'job 1 names event record {len(ev)}'),
                             (dict(tail=len(tails)), 'job 1 names event record'), (dict(n=0), 'job 1 is the region')):
            host = jobs.copy()
            for k, v in fault.items():
                host[k][1] = v
            with pytest.raises(RuntimeError, match=match):
                _run(flat, host, M.MODES[mode], ev, tails, jobs_dev=jobs)
        if mode == 'lufs':
            with pytest.raises(RuntimeError, match=f'work_len={doubles - 1} is too small'):
                _run(flat, jobs, 1, ev, tails, work_len=doubles - 1)
            host = jobs.copy()
            host['ws_off'][2] -= 1
            with pytest.raises(RuntimeError, match='job 2 has ws_off'):
                _run(flat, host, 1, ev, tails, jobs_dev=jobs)
    with pytest.raises(RuntimeError, match='null pointer'):
        L.check(L.load().sedt_relevel(None, 0, None, None, 0, 0, None, None, H, 0.0, None, 0, None, 0, None, 0, None, None, None, None), 'relevel')


def test_device_relevel_stage():
    """the public stage on its own: jobs through its pinned ring, its own workspace, gains into the caller's device records"""
    from sound_event_detection_transformer_amd.utilities import relevel as M
    from sound_event_detection_transformer_amd.utilities.soundscape import EVENT
    flat, offs, ns = K.layout(3)
    d_flat = torch.from_numpy(np.array(flat)).cuda()
    for mode in R.MODES:
        ref = K.reference(3, mode)
        rl = M.DeviceRelevel(SR, mode)
        jobs, doubles = rl.jobs(offs, ns, [K.target_db(i) for i in range(3)], ev=[2, 0, 1])
        assert doubles == (sum(int(n) // H + 1 for n in ns) if mode == 'lufs' else 0)
        ev = torch.zeros(3 * EVENT.itemsize, dtype=torch.uint8, device='cuda')
        level, counts, status = rl.launch(d_flat, jobs, ev=ev, n_ev=3)
        assert status.cpu().tolist() == [0, 0, 0] and counts.cpu().tolist() == [m['counts'] for m in ref]
        M.DeviceRelevel.check(status)
        gains = ev.cpu().numpy().view(EVENT)['gain']
        assert all(_ulps(gains[k], ref[i]['gain']) <= 1 for i, k in enumerate((2, 0, 1)))
        level2, _, _ = rl.launch(d_flat, rl.jobs(offs, ns, [K.target_db(i) for i in range(3)])[0])    # no records: the levels alone
        assert level2.cpu().numpy().tobytes() == level.cpu().numpy().tobytes()
    silent = M.relevel_jobs([0], [5], [0.1])[0]
    with pytest.raises(RuntimeError, match='region 0: status 1'):
        M.DeviceRelevel.check(M.DeviceRelevel(SR).launch(torch.zeros(8, device='cuda'), silent)[2])


# ---------------------------------------------------------------------------------------------------- soundscapes
W, NFFT, HALF = 16000, 512, 8000


@pytest.fixture(scope='module')
def bank():
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    gen = np.random.default_rng(31)
    two = np.concatenate([0.2 * gen.standard_normal(HALF), 0.02 * gen.standard_normal(HALF)]).astype(np.float32)    # halves 20 dB apart
    rir = (gen.standard_normal(700) * np.exp(-6.0 * np.arange(700) / 700)).astype(np.float32)
    return dict(sounds=[two], classes=[3], rirs=[rir], mel=DeviceMelSpectrogram.dcase())


def _scapes(bank, level, **kw):
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    s = SoundscapeClips(bank['mel'], LABELS, W / SR, level=level, stretch_n_fft=NFFT, reverb_n_fft=NFFT, resample_quality='kaiser_fast', **kw)
    return s.add_events(bank['sounds'], bank['classes']).add_rirs(bank['rirs'])


N_EV, ONSET, TARGET = 7000, 100, -31.5
CLIPS = {'excerpt': ((0, 3, HALF + 500, N_EV, ONSET, 0.0, 0), -1, N_EV),
         'stretched': ((0, 3, HALF + 500, N_EV, ONSET, 0.0, 0, 3.0, 1.25), -1, 8750),
         'wet': ((0, 3, HALF + 500, N_EV, ONSET, 0.0, 0), 0, N_EV + 700 - 1)}


@pytest.mark.parametrize('level', R.MODES)
def test_a_releveled_event_measures_its_target(bank, level):
    """one event cut from the QUIET half, fade 0, no background, the peak limit off: mixed with relevel its extent in the clip measures
    target_db - as an excerpt, stretched, and wet (head + the bed's tail) - while the host's gain, taken from the whole source's level,
    misses by more than 1 dB"""
    from sound_event_detection_transformer_amd.utilities.soundscape import gains
    s = _scapes(bank, level, relevel=True)
    host_gain = gains(TARGET, 0.0, s.level_amp[0] if level == 'lufs' else s.rms[0])         # what draw_plan would write
    got = {}
    for name, (event, rir, extent) in CLIPS.items():
        event = event[:5] + (host_gain,) + event[6:]
        plan = s.plan([None], [[event]], [[rir]], levels=[[TARGET]])
        for relevel in (True, False):
            wave, _, dt = s.mix(plan, relevel=relevel)
            assert float(s.last_scale.cpu()[0]) == 1.0 and not dt.status.any().item()      # the peak limit does not bite
            x = wave.cpu().numpy()[0]
            assert not x[:ONSET].any() and not x[ONSET + extent:].any() and ONSET + extent < W
            got[name, relevel] = R.measured_db(x[ONSET:ONSET + extent], SR, level)
            if relevel:
                assert s.last_relevel[2].cpu().tolist() == [0] and len(s.last_fx['relevel_jobs']) == 1
                assert int(s.last_fx['relevel_jobs']['n'][0]) == extent
            else:
                assert s.last_relevel is None
    print(level, {k: round(v, 6) for k, v in got.items()})
    for name in CLIPS:
        assert abs(got[name, True] - TARGET) < 1e-4, (name, got[name, True])
    assert abs(got['excerpt', False] - TARGET) > 1.0, got['excerpt', False]


EVENTS = [[(0, 3, 200, 2000, 1500, 0.7, 0)],
          [(0, 3, 0, 1000, 100, 0.5, 16), (0, 3, HALF, 2000, 900, 0.3, 160), (0, 3, 9000, 700, 2000, 0.6, 16, 3.0, 1.25)],
          [(0, 3, 12000, 700, 3000, 0.9, 8)]]
RIRS = [[-1], [0, -1, 0], [0]]
LEVELS = [[-30.0], [-28.0, -35.5, -24.0], [-33.0]]


def test_wiring_of_the_stage_inside_mix(bank):
    """three clips - dry, wet + dry + stretched wet, wet - mixed with relevel: the device records carry the gains of the stage run on its
    own over the same rows, the wave is soundscape_ref's fed those gains, the targets are those of the plan mixed without relevel"""
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities import relevel as M
    from sound_event_detection_transformer_amd.utilities.reverb import TAIL
    from sound_event_detection_transformer_amd.utilities.soundscape import EVENT
    s = _scapes(bank, 'lufs', relevel=True)
    plan = s.plan([None] * 3, EVENTS, RIRS, levels=LEVELS)
    with L.launch_log() as log:
        wave, _, dt = s.mix(plan)
    assert log['relevel'] == 1 and log['soundscape'] == 1 and log['stretch'] == 1 and log['reverb'] == 1 and log['reverb_bed'] == 1
    wave, blob = wave.cpu().numpy().copy(), dt.blob.cpu().numpy().copy()
    fx = s.last_fx
    jobs, ev, tails, rj, sj = fx['relevel_jobs'], fx['events'], fx['tails'], fx['reverb_jobs'], fx['jobs']
    assert s.last_relevel[2].cpu().tolist() == [0] * 5 and not dt.status.any().item()
    flat = fx['flat'].cpu().numpy()
    # ---- the regions: bank excerpts for the dry events, the wet rows (head and tail) for the wet ones
    assert jobs['ev'].tolist() == [0, 1, 2, 3, 4] and jobs['tail'].tolist() == [-1, 0, -1, 1, 2]
    assert jobs['n'].tolist() == [2000, 1000 + 699, 2000, 875 + 699, 700 + 699] and jobs['off'][[0, 2]].tolist() == [200, HALF]
    assert jobs['off'][[1, 3, 4]].tolist() == rj['dst_off'].tolist() and int(rj['src_off'][1]) == int(sj['dst_off'][0])
    assert np.array_equal(jobs['target'], M.target_amplitude(np.concatenate(LEVELS), 'lufs'))
    # ---- the gains in the device records: those of the stage on its own over the same buffer, bit for bit
    ev_dev, tails_dev = fx['ev_dev'].cpu().numpy().view(EVENT), fx['tails_dev'].cpu().numpy().view(TAIL)
    own_ev, own_tails = torch.from_numpy(ev.view(np.uint8).copy()).cuda(), torch.from_numpy(tails.view(np.uint8).copy()).cuda()
    level, counts, status = s.releveler().launch(fx['flat'], jobs, ev=own_ev, n_ev=5, tails=own_tails, n_tails=3)
    assert level.cpu().numpy().tobytes() == s.last_relevel[0].cpu().numpy().tobytes()
    assert ev_dev.tobytes() == own_ev.cpu().numpy().tobytes() and tails_dev.tobytes() == own_tails.cpu().numpy().tobytes()
    assert tails_dev['gain'].tobytes() == ev_dev['gain'][[1, 3, 4]].tobytes()
    zbar = level.cpu().numpy()
    for i in range(5):                                                                      # ... and they bring every region to its level
        region = flat[int(jobs['off'][i]):int(jobs['off'][i] + jobs['n'][i])].astype(np.float64) * np.float64(ev_dev['gain'][i])
        assert abs(R.measured_db(region, SR, 'lufs') - np.concatenate(LEVELS)[i]) < 1e-5
        assert _ulps(ev_dev['gain'][i], R.gain(jobs['target'][i], zbar[i])[1]) <= 1
    assert not np.array_equal(ev_dev['gain'], ev['gain']) and _unchanged(ev_dev, ev, range(5)) and _unchanged(tails_dev, tails, range(3))
    # ---- the wave: soundscape_ref fed the device's rows and those gains
    stretched = flat[int(sj['dst_off'][0]):int(sj['dst_off'][0] + sj['m'][0])].copy()
    wets = [flat[int(j['dst_off']):int(j['dst_off']) + int(t)].copy() for j, t in zip(rj, tails['total'])]
    g = ev_dev['gain']
    beds = [RV.bed(W, None, 0, 1.0, [(g[1], wets[0], 100, 1000), (g[3], wets[1], 2000, 875)]), RV.bed(W, None, 0, 1.0, [(g[4], wets[2], 3000, 700)])]
    sources = bank['sounds'] + [stretched] + wets + beds
    want = S.soundscape(sources, fx['bg'], ev_dev, plan.ev_off, W, SR, s.max_targets, s.min_event_seconds, s.collapse, s.peak_limit)
    assert np.array_equal(wave.view(np.int32), want[0].view(np.int32)) and (want[4] == 0).all()
    # ---- the targets are those of the plan mixed without relevel; so is everything else of that mix
    s0 = _scapes(bank, 'lufs')
    with L.launch_log() as log0:
        wave0, _, dt0 = s0.mix(plan)
    wave0 = wave0.cpu().numpy().copy()
    assert dt0.blob.cpu().numpy().tobytes() == blob.tobytes() and not np.array_equal(wave0, wave)
    # ---- unchanged default: relevel=False on an object built with relevel=True issues the calls and writes the bytes of one built without
    with L.launch_log() as log1:
        wave1, _, dt1 = s.mix(plan, relevel=False)
    assert dict(log1) == dict(log0) and 'relevel' not in dict(log0) and wave1.cpu().numpy().tobytes() == wave0.tobytes()
    assert dt1.blob.cpu().numpy().tobytes() == blob.tobytes() and s.last_relevel is None and 'relevel_jobs' not in s.last_fx
    plain = s.plan([None], [EVENTS[0]], levels=[LEVELS[0]])
    with L.launch_log() as log2:
        wave2, _, _ = s.mix(plain, relevel=False)
    with L.launch_log() as log3:
        wave3, _, _ = s0.mix(s0.plan([None], [EVENTS[0]]))
    assert dict(log2) == dict(log3) == {'soundscape': 1} and wave2.cpu().numpy().tobytes() == wave3.cpu().numpy().tobytes() and s.last_fx is None
    # ---- a plan without effects: the stage reads the bank itself
    with L.launch_log() as log4:
        s.mix(plain)
    assert dict(log4) == {'relevel': 1, 'soundscape': 1} and s.last_fx['flat'] is s.flat and s.last_relevel[2].cpu().tolist() == [0]
    # ---- relevel needs the plan's levels
    with pytest.raises(ValueError, match='the plan has no target_db'):
        s.mix(s.plan([None], [EVENTS[0]]))
    with pytest.raises(ValueError, match='not finite'):
        s.mix(s.plan([None], [EVENTS[0]], levels=[[float('nan')]]))


def test_drawn_plans_with_relevel(bank):
    """a drawn plan with every effect, RMS mode: every event lies in the bank, every job is measured, and an event whose record lies
    outside the bank gets no job - its clip's status is raised as without relevel"""
    s = _scapes(bank, 'rms', relevel=True)
    np.random.seed(5)
    plan = s.draw(4, n_events=(1, 3), background=False, reverb=0.5, pitch_shift=(-2.0, 2.0), time_stretch=(0.8, 1.25), max_event_seconds=0.2)
    assert plan.target_db is not None and (plan.rir >= 0).any() and (plan.rir < 0).any()
    wave, _, dt = s.mix(plan)
    assert not dt.status.any().item() and torch.isfinite(wave).all().item()
    assert len(s.last_fx['relevel_jobs']) == len(plan.ev) and not s.last_relevel[2].cpu().numpy()[:len(plan.ev)].any()
    _, _, dt = s.mix(s.plan([None, None], [[(0, 3, 15000, 2000, 0, 0.5, 0)], [EVENTS[0][0]]], levels=[[-30.0], [-30.0]]))
    assert dt.status.cpu().tolist() == [2, 0] and s.last_fx['relevel_jobs']['ev'].tolist() == [1]
