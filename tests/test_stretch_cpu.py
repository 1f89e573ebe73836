"""CPU: the float64 restatement of the stretch stage is what it claims, the case table reaches its edges, the per-stage bounds hold a
float32 restatement and reject planted faults, and the host half (utilities.stretch, the plans of utilities.soundscape) - no GPU.

Two planted faults need a word.  phi_u+1 = phi_u + omega_k + wrap(arg D_i+1 - arg D_i - omega_k) equals phi_u + arg D_i+1 - arg D_i
up to whole turns WHATEVER omega_k is and whether or not the difference is wrapped, and exp(i phi) has period 2 pi: dropping ``wrap``
or taking omega_k one bin off leaves S the same up to float64 rounding, so no bound on S can see either (measured here: 4e-10 of the
bound).  What both break is the definition's property that a step's phase advance deviates from omega_k by at most pi; the stage
check asks for that property ('advance') wherever an implementation shows its phase, and that is where these two are caught."""
import math

import numpy as np
import pytest

import stretch_cases as K
import stretch_ref as R
from sound_event_detection_transformer_amd.utilities import soundscape as SC
from sound_event_detection_transformer_amd.utilities import stretch as M

ROWS = list(range(len(K.ROWS)))


def test_the_case_table_reaches_every_named_edge():
    hit = K.edges()
    assert all(hit[k] for k in hit), {k: v for k, v in hit.items() if not v}
    assert {r[1] for r in K.ROWS} >= set(K.LENGTHS) and {r[2] for r in K.ROWS} >= set(K.FACTORS)
    assert {r[3] for r in K.ROWS} >= set(K.SHIFTS)
    assert all(r[0] == 512 or 1 + r[1] // (r[0] // 4) <= 6 for r in K.ROWS)
    assert any(K.ROWS[i][4] == 'noise' for i in K.BEST_ROWS)


@pytest.mark.parametrize('row', ROWS)
def test_host_half_agrees_with_the_restatement(row):
    N, n, f, p, _ = K.ROWS[row]
    assert M.stretch_lengths(n, f, p, N) == R.lengths(n, f, p, N)
    m, m1, r, alpha, T, U = R.lengths(n, f, p, N)
    assert K.reference(row)['y'].shape == (m,) and m == math.floor(n * f + 0.5)
    if T:
        assert (U - 1) * r < T <= U * r and abs(U - T / r) < 1.0 + 1e-9
        from sound_event_detection_transformer_amd import lib as L
        assert L.load().sedt_stretch_ok(N, n, m, m1, r, alpha, T, U) == 1
        assert L.load().sedt_stretch_ok(N, n, m, m1, r, alpha, T, U + 1) == 0


def test_tables():
    for N in M.N_FFTS:
        assert np.array_equal(M.hann_window(N), R.hann(N)) and M.hann_window(N)[0] == 0.0 and M.hann_window(N)[N // 2] == 1.0
        tw = M.twiddle_table(N)
        assert tw.shape == (2, N // 2 + 1) and tw.dtype == np.float32 and tw[0, 0] == 1.0 and tw[1, N // 4] == -1.0
        # the window sums of the overlap-add never sit at the threshold: the float32 sum on the device decides as float64 does
        ws = R.window_sum(7, N, 0)
        assert not ((ws > 0.99 * R.WS_MIN) & (ws < 1.01 * R.WS_MIN)).any()
    for q in ('kaiser_best', 'kaiser_fast'):
        tab, Z = M.filter_table(q)
        assert tab.dtype == np.float32 and tab.shape == (512 * Z + 1,) and np.array_equal(tab, R.filter_table(q)[0])
        assert tab[0] == np.float32(R.QUALITIES[q][1])
    with pytest.raises(ValueError, match='quality'):
        M.filter_table('sinc_best')


def test_rate_one_reconstructs_the_input():
    for N, n in ((512, 3000), (1024, 1300), (512, 100)):
        x = np.random.default_rng(n).standard_normal(n)
        D = R.stft(x, N)
        S, phi, _ = R.vocoder(D, 1.0, D.shape[0], N)
        assert np.abs(R.istft(S, N, n) - x).max() <= 1e-10 * np.abs(x).max()


def _peak_bin(y, N):
    mid = R.stft(y, N)[2:-2] if len(y) >= 6 * (N // 4) else R.stft(y, N)
    return int(np.abs(mid).sum(axis=0).argmax())


def test_a_tone_keeps_its_bin_under_a_stretch_and_doubles_it_an_octave_up():
    N, b = 512, 20
    x = np.sin(2.0 * np.pi * b * np.arange(6000) / N)
    assert _peak_bin(x, N) == b
    for f in (0.8123, 1.25, 2.0):
        out = R.chain(x, f, 0.0, N)
        assert len(out['y']) == math.floor(6000 * f + 0.5) and _peak_bin(out['y'], N) == b
    out = R.chain(x, 1.0, 12.0, N)
    assert len(out['y']) == 6000 and _peak_bin(out['y'], N) == 2 * b
    assert _peak_bin(R.chain(x, 1.25, -12.0, N)['y'], N) == b // 2


def _stage_errors(row, dtype, fault=None, quality=K.QUALITY):
    """{stage: largest error / bound} of an implementation (dtype, fault) against float64, every stage fed what the implementation's
    own previous stage produced (as the device is checked); 'advance': the largest |phase advance - omega| / pi"""
    N, n, f, p, _ = K.ROWS[row]
    m, m1, r, alpha, T, U = R.lengths(n, f, p, N)
    x = K.signal(row)
    out = {}
    ratio = lambda err, bound: float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)),
                                            initial=0.0))
    if T:
        D = R.stft(x, N, dtype)
        out['stft'] = ratio(np.abs(D - K.reference(row)['D']).max(axis=1), R.stft_bound(x, N))
        S, phi, _ = R.vocoder(D, r, U, N, dtype, fault)
        S_ref, _, mag = R.vocoder(D.astype(np.complex128), r, U, N)
        out['vocoder'] = ratio(np.abs(S - S_ref), R.vocoder_bound(mag, N))
        k = np.arange(N // 2 + 1)
        adv = np.diff(phi, axis=0) - (2.0 * np.pi * (N // 4) * k) / N
        out['advance'] = float(np.abs(adv).max() / np.pi) if U > 1 else 0.0
        z = R.istft(S, N, m1, dtype, fault)
        out['inverse'] = ratio(np.abs(z - R.istft(S.astype(np.complex128), N, m1)), R.istft_bound(S.astype(np.complex128), N, m1))
    else:
        z = x.astype(dtype)
    y = R.resample(z, alpha, m, quality, dtype, fault)
    assert y.shape == (m,)
    z64 = z.astype(np.float64)
    out['resample'] = ratio(np.abs(y - R.resample(z64, alpha, m, quality)), R.resample(z64, alpha, m, quality, bound=True))
    return out


# the constants are fixed from the device's measurement; the float32 restatement has to pass the same bounds
def _passes(e):
    return all(v <= 1.0 for k, v in e.items() if k != 'advance') and e.get('advance', 0.0) <= 1.0 + 1e-6


@pytest.mark.parametrize('row', ROWS)
def test_the_float32_restatement_passes_every_stage_bound(row):
    e = _stage_errors(row, np.float32)
    print(K.ROWS[row], {k: round(v, 4) for k, v in e.items()})
    assert _passes(e), e
    assert _passes(_stage_errors(row, np.float64))


def test_the_float32_restatement_with_the_long_filter():
    for row in K.BEST_ROWS:
        assert _passes(_stage_errors(row, np.float32, quality='kaiser_best'))


@pytest.mark.parametrize('fault', R.FAULTS)
def test_a_planted_fault_fails_a_row(fault):
    stage = {'swap_a': 'vocoder', 'no_wrap': 'advance', 'omega_off': 'advance', 'ws_plain': 'inverse', 'no_scale': 'resample',
             'nearest': 'resample', 'round_step': 'vocoder'}[fault]
    failed = []
    for row in ROWS:
        if K.ROWS[row][1] > 3000:
            continue
        e = _stage_errors(row, np.float32, fault)
        if e.get(stage, 0.0) > (1.0 + 1e-6 if stage == 'advance' else 1.0):      # the stage it was planted in
            failed.append(row)
            assert not _passes(e)
    print(fault, 'fails rows', failed)
    assert failed, fault


def test_envelope_violations_are_refused():
    ok = dict(n=1000, factor=1.1, semitones=2.0, n_fft=512)
    M.stretch_lengths(**ok)
    for bad in (dict(n=0), dict(n=-5), dict(n=2 ** 26 + 1), dict(n=10.5), dict(factor=0.49), dict(factor=2.01), dict(factor=float('nan')),
                dict(semitones=12.5), dict(semitones=-13), dict(semitones=float('nan')), dict(n_fft=256), dict(n_fft=4096)):
        with pytest.raises(ValueError, match='outside the envelope'):
            M.stretch_lengths(**{**ok, **bad})
    with pytest.raises(ValueError, match='one duration factor'):
        M.stretch_jobs([10, 20], [1.0], [0.0, 0.0])
    with pytest.raises(ValueError, match='outside the envelope'):
        M.stretch_jobs([10, 20], [1.0, 3.0], [0.0, 0.0])
    with pytest.raises(ValueError, match='outside the envelope'):
        M.DeviceStretch(16000, n_fft=256, device='cpu')


def test_jobs_and_the_workspace_they_ask_for():
    from sound_event_detection_transformer_amd import lib as L
    ns, fs, ps = [1, 129, 3000, 257], [0.5, 0.5, 1.25, 1.0], [-12.0, 12.0, 3.0, 0.0]
    jobs, floats = M.stretch_jobs(ns, fs, ps, 512)
    assert jobs.dtype.itemsize == 72 == L.load().sedt_sizeof(15)
    assert jobs['src_off'].tolist() == [0, 1, 130, 3130] and all(o % 4 == 0 for o in jobs['dst_off'].tolist() + jobs['ws_off'].tolist())
    for e in range(4):
        assert tuple(jobs[e][k] for k in ('m', 'm1', 'r', 'alpha', 'T', 'U')) == R.lengths(ns[e], fs[e], ps[e], 512)
    assert L.load().sedt_stretch_workspace(jobs.ctypes.data, 4, 512) == 4 * floats
    reg = M.regions(jobs[2], 512)
    assert reg['D_re'][0] == jobs[2]['ws_off'] and reg['z'][0] + jobs[2]['m1'] <= jobs[3]['ws_off']
    assert reg['S_re'][1] == (int(jobs[2]['U']), 257) and reg['frames'][1] == (int(jobs[2]['U']), 512)
    bad = jobs.copy()
    bad['U'][2] += 1
    assert L.load().sedt_stretch_workspace(bad.ctypes.data, 4, 512) == -1
    assert b'outside the envelope' in L.load().sedt_last_error()
    assert L.load().sedt_stretch_workspace(jobs.ctypes.data, -1, 512) == -1 and L.load().sedt_stretch_workspace(jobs.ctypes.data, 4, 256) == -1
    assert L.load().sedt_stretch_workspace(None, 4, 512) == -1


# ---------------------------------------------------------------------- plans
LENS = [700, 5000, 20000, 3, 40000]
LEVEL = [0.1, 0.2, 0.05, 0.3, 0.01]
BY_CLASS = [[0], [1, 2], [], [3]]


def _draw(seed, **kw):
    np.random.seed(seed)
    return SC.draw_plan(6, LENS, LEVEL, BY_CLASS, [4], 16000, 16000, n_events=(1, 5), max_event_seconds=0.8, **kw)


@pytest.mark.parametrize('seed', [3, 4, 5])
def test_a_plan_without_effects_is_the_plan_it_was(seed):
    a, b = _draw(seed), _draw(seed, pitch_shift=None, time_stretch=None)
    assert a.fx is None and b.fx is None
    assert a.bg.tobytes() == b.bg.tobytes() and a.ev.tobytes() == b.ev.tobytes() and a.ev_off.tobytes() == b.ev_off.tobytes()
    # ... and what the restated draw of the soundscape tests gives, which consumes np.random in the documented order
    import soundscape_ref as S
    np.random.seed(seed)
    bg, ev, off = S.draw(6, LENS, LEVEL, BY_CLASS, [4], 16000, 16000, (1, 5), (6.0, 30.0), -30.0, 0.8, 0.01)
    assert a.bg.tobytes() == bg.tobytes() and a.ev.tobytes() == ev.tobytes()


@pytest.mark.parametrize('seed', [3, 4, 5])
def test_a_plan_with_effects_fits_the_window(seed):
    plan = _draw(seed, pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2))
    assert plan.fx is not None and plan.fx.shape == plan.ev.shape and len(plan.ev)
    cap = int(round(0.8 * 16000))
    for e, x in zip(plan.ev, plan.fx):
        assert -3.0 <= x['semitones'] <= 3.0 and np.float32(0.8) <= x['factor'] <= np.float32(1.2)
        m = math.floor(int(e['n']) * float(x['factor']) + 0.5)
        assert m == M.stretch_lengths(int(e['n']), x['factor'], x['semitones'])[0]
        assert 1 <= e['n'] and e['src_start'] + e['n'] <= LENS[e['src']] and 0 <= e['onset'] and e['onset'] + m <= 16000 and m <= cap
        longer = math.floor((int(e['n']) + 1) * float(x['factor']) + 0.5)
        assert e['n'] == LENS[e['src']] or longer > cap                      # the LARGEST excerpt that fits
    only_p = _draw(seed, pitch_shift=(-2.0, 2.0))
    assert (only_p.fx['factor'] == 1.0).all() and (only_p.fx['semitones'] != 0.0).any()
    for bad in (dict(pitch_shift=(-13.0, 0.0)), dict(time_stretch=(0.4, 1.0)), dict(time_stretch=(1.2, 0.8))):
        with pytest.raises(ValueError):
            _draw(seed, **bad)


def test_make_plan_round_trips_fx():
    events = [[(0, 1, 5, 100, 7, 0.5, 3, -2.5, 1.125), (1, 0, 0, 50, 0, 1.0, 0)], [], [(2, 2, 1, 10, 2, 0.25, 0, 0.0, 1.0)]]
    plan = SC.make_plan([None, (4, 10, 0.5), None], events)
    assert plan.fx.tolist() == [(-2.5, 1.125), (0.0, 1.0), (0.0, 1.0)] and SC.is_identity(plan.fx).tolist() == [False, True, True]
    assert plan.ev['n'].tolist() == [100, 50, 10] and plan.ev_off.tolist() == [0, 2, 2, 3]
    plain = SC.make_plan([None], [[(1, 0, 0, 50, 0, 1.0, 0)]])
    assert plain.fx is None
    again = SC.SoundscapePlan(plan.bg, plan.ev, plan.ev_off, plan.fx)
    assert again.fx.tobytes() == plan.fx.tobytes()
    with pytest.raises(ValueError, match='fx'):
        SC.SoundscapePlan(plan.bg, plan.ev, plan.ev_off, plan.fx[:2])
    with pytest.raises(ValueError, match='optional'):
        SC.make_plan([None], [[(1, 0, 0, 50, 0, 1.0, 0, 2.0)]])
    assert SC.excerpt_for(1000, 1.0) == 1000 and SC.excerpt_for(1000, 2.0) == 500 and SC.excerpt_for(1000, 0.5) == 2000
