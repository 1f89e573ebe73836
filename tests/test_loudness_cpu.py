"""CPU: the host half of the loudness stage (utilities/loudness.py) and its float64 reference (tests/loudness_ref.py): the K-weighting
coefficients against the standard's table, the hop map against direct simulation, the 997 Hz anchors, the restated gates on a designed
signal, the entry points' argument checks, the level='lufs' mode of the soundscape plan - and, on the reference alone, that no block of
a GPU case lies at a gate threshold (the condition under which tests/test_loudness_gpu.py compares the counts exactly)."""
import math
import types

import numpy as np
import pytest

import loudness_cases as K
import loudness_ref as R


def _mel(sr=16000):
    return types.SimpleNamespace(sr=sr, min_samples=513, hop=256, F=64)


def test_coefficients_at_48_khz_are_the_standards_table():
    from sound_event_detection_transformer_amd.utilities import loudness as M
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
            1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    got = M.k_weighting(48000)
    assert got.dtype == np.float64 and got.shape == (10,) and np.abs(got - np.asarray(want)).max() < 1e-12
    for sr in K.RATES + (44100,):
        (b1, a1), (b2, a2) = R.k_weighting(sr)
        assert np.array_equal(M.k_weighting(sr), np.concatenate([b1, a1[1:], b2, a2[1:]]))      # the restatement, to the bit
        assert a1[0] == 1.0 and a2[0] == 1.0 and b2.tolist() == [1.0, -2.0, 1.0]
    assert M.hop_samples(16000) == 1600 and M.hop_samples(22050) == 2205 and M.hop_samples(48000) == 4800 and M.hop_samples(44100) == 4410
    assert M.Z_ABS == R.Z_ABS == 10.0 ** ((-70.0 + 0.691) / 10.0)
    with pytest.raises(ValueError):
        M.k_weighting(0)


@pytest.mark.parametrize('sr', K.RATES)
def test_hop_map_against_direct_simulation(sr):
    """hop_map @ (state at a hop's start) + (the state the hop leaves from zero state) is the state the serial filter has there"""
    from sound_event_detection_transformer_amd.utilities import loudness as M
    Hm = M.hop_map(sr)
    assert Hm.shape == (4, 4) and Hm.dtype == np.float64 and np.array_equal(Hm, R.hop_map(sr))
    H = R.hop_samples(sr)
    (b1, a1), (b2, a2) = R.k_weighting(sr)
    x = np.random.default_rng(3).standard_normal(3 * H).astype(np.float32).astype(np.float64)

    def run(seg, state):
        y, s_a = R.biquad(b1, a1, seg, state[:2])
        y, s_b = R.biquad(b2, a2, y, state[2:])
        return y, np.asarray(s_a + s_b)

    y_serial, _ = run(x, np.zeros(4))
    start, worst = np.zeros(4), 0.0
    for h in range(3):
        seg = x[h * H:(h + 1) * H]
        y, _ = run(seg, start)                                     # pass B: from the true start state
        e_serial = np.sum(y_serial[h * H:(h + 1) * H] ** 2)
        worst = max(worst, abs(np.sum(y * y) - e_serial) / e_serial)
        start = Hm @ start + run(seg, np.zeros(4))[1]              # pass A and the walk
    assert worst < 1e-13, worst
    assert np.abs(np.linalg.eigvals(Hm)).max() < 1e-2             # a hop later little of a state is left


def test_997_hz_anchors():
    for sr, want, tol in ((48000, -3.01, 0.005), (16000, -2.970, 0.05), (22050, -2.981, 0.05)):
        x = np.sin(2.0 * np.pi * 997.0 * np.arange(5 * sr) / sr).astype(np.float32)
        m = R.measure(x, sr)
        assert abs(m['lufs'] - want) < tol, (sr, m['lufs'])
        assert m['J'] == 5 * sr // R.hop_samples(sr) - 3 and m['n_abs'] == m['J'] == m['n_rel'] and not m['short']


def test_restated_gates_on_a_designed_signal():
    """2 s of noise at 0.1, 6 s at 30 dB less, 2 s at 1e-5, at 16 kHz: blocks fall under each gate"""
    sr = 16000
    gen = np.random.default_rng(5)
    x = np.concatenate([0.1 * gen.standard_normal(2 * sr), 0.1 * 10.0 ** (-30.0 / 20.0) * gen.standard_normal(6 * sr),
                        1e-5 * gen.standard_normal(2 * sr)]).astype(np.float32)
    m = R.measure(x, sr)
    assert m['J'] == 97 and 0 < m['n_rel'] < m['n_abs'] < m['J'], (m['J'], m['n_abs'], m['n_rel'])
    assert (m['n_abs'], m['n_rel']) == (80, 20)
    z = m['z']
    assert m['n_abs'] == int((z > R.Z_ABS).sum()) and m['thr'] == 0.1 * z[z > R.Z_ABS].mean()
    assert abs(m['zbar'] - z[(z > R.Z_ABS) & (z > m['thr'])].mean()) <= 1e-15 * m['zbar']
    # the loud fifth alone decides the result: about 20 log10(0.1) plus the K-weighting's gain for white noise
    assert abs(m['lufs'] - R.measure(x[:2 * sr], sr)['lufs']) < 0.5
    # the short-source rule and the empty gates
    short = R.measure(x[:4 * 1600 - 1], sr)
    assert short['short'] and short['J'] == 1 and short['n_abs'] == 1 == short['n_rel']
    y = R.k_filter(x[:4 * 1600 - 1], sr)
    assert short['zbar'] == np.sum(y * y) / (4 * 1600 - 1)
    silent = R.measure(np.zeros(5 * 1600, np.float32), sr)
    assert silent['zbar'] == 0.0 and silent['lufs'] == -math.inf and silent['J'] == 2 and silent['n_abs'] == 0 == silent['n_rel']
    assert not R.measure(x[:4 * 1600], sr)['short']


@pytest.mark.parametrize('sr,n_src', K.CASES)
def test_no_block_of_a_gpu_case_lies_at_a_gate_threshold(sr, n_src):
    """... within 1e-6 relative: then the device's counts can be compared exactly.  Also: the cases contain what they are there for."""
    ref, plan = K.reference(sr, n_src), K.plan(sr, n_src)
    H = R.hop_samples(sr)
    assert len(ref) == n_src == len(plan) and [len(x) for x in K.sources(sr, n_src)] == [n for n, _ in plan]
    for i, m in enumerate(ref):
        assert R.gate_clearance(m['z'], m['thr']) > 1e-6, (i, plan[i])
        assert m['short'] == (plan[i][0] < 4 * H) and m['J'] == (1 if m['short'] else plan[i][0] // H - 3)
    if n_src == 70:
        assert {n for n, _ in plan} >= {1, H - 1, 4 * H - 1, 4 * H, 4 * H + 1, 5 * H - 1, 5 * H} and {k for _, k in plan} == set(K.CONTENTS)
        by = lambda kind: [m for m, (n, k) in zip(ref, plan) if k == kind]
        assert all(m['zbar'] == 0.0 and m['n_abs'] == 0 for m in by('zero') + by('quiet')) and any(m['z'].max() > 0 for m in by('quiet'))
        assert any(m['n_rel'] < m['n_abs'] < m['J'] for m in by('steps'))                  # both gates act
        assert all(m['zbar'] > 0 for m in by('noise') + by('dc'))
        assert sum(1 for x in np.cumsum([n for n, _ in plan])[:-1] if x % 4) > 20           # most sources start off a 16-byte boundary
    if sr == 16000 and n_src in (1, 3):
        assert any(n // H > 256 for n, _ in plan)                                          # a second round of hops
        assert any(m['n_rel'] < m['n_abs'] < m['J'] for m in ref)


def test_entry_points_refuse_bad_arguments():
    """refused with a message before a pointer is touched (every pointer here is null)"""
    from sound_event_detection_transformer_amd import _build, lib
    _build.build()
    l = lib.load()
    loud = lambda n_src=2, flat_len=0, hop=1600, z_abs=R.Z_ABS, work_len=8: l.sedt_loudness(
        None, flat_len, None, None, n_src, None, None, hop, z_abs, None, work_len, None, None, None)
    for n_src in (0, -1):
        assert loud(n_src=n_src) != 0 and f'n_src={n_src}' in l.sedt_last_error().decode()
    assert loud(flat_len=-1) != 0 and 'flat_len=-1' in l.sedt_last_error().decode()
    for hop in (0, -5):
        assert loud(hop=hop) != 0 and f'hop={hop}' in l.sedt_last_error().decode()
    for z in (float('nan'), -1.0):
        assert loud(z_abs=z) != 0 and 'z_abs' in l.sedt_last_error().decode()
    assert loud(n_src=3, work_len=2) != 0 and 'work_len=2 is too small' in l.sedt_last_error().decode()
    assert loud(work_len=-1) != 0 and 'too small' in l.sedt_last_error().decode()
    assert loud() != 0 and 'null pointer' in l.sedt_last_error().decode()                  # inside the envelope: the pointers are looked at
    scale = lambda n_src=2, flat_len=0: l.sedt_scale_sources(None, flat_len, None, None, n_src, None, None)
    assert scale(n_src=0) != 0 and 'n_src=0' in l.sedt_last_error().decode()
    assert scale(flat_len=-1) != 0 and 'flat_len=-1' in l.sedt_last_error().decode()
    assert scale() != 0 and 'null pointer' in l.sedt_last_error().decode()


def test_host_half_of_the_stage():
    from sound_event_detection_transformer_amd.utilities import loudness as M
    assert M.work_doubles([1, 1599, 1600, 6400, 0], 1600) == 1 + 1 + 2 + 5 + 1
    got = M.lufs_of(np.asarray([0.0, 1.0, 10.0 ** -2.3]))
    assert got[0] == -np.inf and got[1] == -0.691 and abs(got[2] - (-23.691)) < 1e-12 and got.dtype == np.float64
    assert all(M.lufs_of([m['zbar']])[0] == m['lufs'] for m in K.reference(16000, 3))
    # gains of a normalisation: float32(min(10^((target - L) / 20), peak_limit / peak)) from float64
    g, limited, silent = M.normalize_gains([-30.0, -10.0, -np.inf, -40.0], np.asarray([0.1, 0.5, 0.0, 0.3], np.float32), -23.0, 1.0)
    assert g.dtype == np.float32 and g[0] == np.float32(10.0 ** (7.0 / 20.0)) and g[1] == np.float32(10.0 ** (-13.0 / 20.0)) and g[2] == 1.0
    assert limited.tolist() == [False, False, False, True] and silent.tolist() == [False, False, True, False]
    assert abs(float(g[3]) - 1.0 / float(np.float32(0.3))) < 1e-6 and np.float32(0.3) * g[3] <= np.float32(1.0)
    for peak in np.random.default_rng(2).uniform(0.01, 0.99, 200).astype(np.float32):      # the limited peak never passes the limit
        g, limited, _ = M.normalize_gains([-60.0], [peak], 0.0, 0.7)
        assert limited[0] and float(np.float32(peak) * g[0]) <= 0.7 and float(np.float32(peak) * np.nextafter(g[0], np.float32(2))) > 0.7 - 1e-6
    dev = M.DeviceLoudness(22050, device='cpu')                                            # built without a device; nothing is uploaded yet
    assert dev.hop == 2205 and np.array_equal(dev.coef, M.k_weighting(22050)) and np.array_equal(dev.map, M.hop_map(22050))
    with pytest.raises(ValueError, match='target'):
        dev.normalize(None, [0], [1], float('nan'))
    with pytest.raises(ValueError, match='peak_limit'):
        dev.normalize(None, [0], [1], -23.0, peak_limit=0.0)


def test_soundscape_level_modes():
    from sound_event_detection_transformer_amd.utilities import soundscape as M
    labels = [f'c{i}' for i in range(10)]
    with pytest.raises(ValueError, match="level 'x' is neither 'rms' nor 'lufs'"):
        M.SoundscapeClips(_mel(), labels, 1.0, device='cpu', level='x')
    assert M.SoundscapeClips(_mel(), labels, 1.0, device='cpu').level == 'rms'                # the default
    s = M.SoundscapeClips(_mel(), labels, 1.0, device='cpu', level='lufs')
    assert s.level == 'lufs' and s.lufs.shape == (0,) and s.level_amp.shape == (0,)
    # gains under 'lufs': gains(ref, snr, 10^(L / 20)), which is 10^((ref + snr - L) / 20) up to float32 rounding; -inf: gain 1
    for ref_db, snr, lufs in ((-30.0, 6.0, -23.5), (-50.0, 0.0, -61.25), (-30.0, 29.0, -3.01)):
        amp = np.float64(10.0) ** (np.float64(lufs) / 20.0)
        g = M.gains(ref_db, snr, amp)
        assert g == np.float32(10.0 ** ((ref_db + snr) / 20.0) / amp) and g.dtype == np.float32
        assert abs(float(g) / 10.0 ** ((ref_db + snr - lufs) / 20.0) - 1.0) < 1e-7
    assert np.float64(10.0) ** (np.float64(-np.inf) / 20.0) == 0.0 and M.gains(-30.0, 0.0, 0.0) == 1.0
    # a drawn plan hands level_amp to draw_plan where it hands rms under 'rms': the same draws, other gains
    s.ns, s.by_class, s.backgrounds = [5, 4000, 90000, 700], [[0, 1]] + [[] for _ in range(9)], [2, 3]
    s.lufs = np.asarray([-20.0, -35.5, -48.0, -np.inf])
    s.level_amp = np.float64(10.0) ** (s.lufs / 20.0)
    s.rms = np.asarray([0.5, 0.01, 0.2, 0.0])
    np.random.seed(9)
    plan = s.draw(6, ref_db=-40.0)
    after = np.random.random_sample(2)
    np.random.seed(9)
    want = M.draw_plan(6, s.ns, s.level_amp, s.by_class, s.backgrounds, s.window, 16000, ref_db=-40.0)
    assert plan.ev.tobytes() == want.ev.tobytes() and plan.bg.tobytes() == want.bg.tobytes()
    s.level = 'rms'
    np.random.seed(9)
    rms_plan = s.draw(6, ref_db=-40.0)
    assert np.array_equal(after, np.random.random_sample(2))                               # np.random consumed identically
    same = lambda f: np.array_equal(plan.ev[f], rms_plan.ev[f])
    assert all(same(f) for f in ('src', 'cls', 'src_start', 'n', 'onset', 'fade')) and not same('gain') and len(plan.ev) > 0
    assert np.array_equal(plan.bg['src'], rms_plan.bg['src']) and np.array_equal(plan.bg['start'], rms_plan.bg['start'])
    assert all(g['gain'] == (1.0 if g['src'] == 3 else M.gains(-40.0, 0.0, s.level_amp[2])) for g in plan.bg)
    # what staging does with the loudness the device returns
    M.check_bank_loudness('add_backgrounds', [-np.inf, -20.0], [-1, -1])                   # a background under the gate is allowed
    with pytest.raises(ValueError, match='source 1 lies under the absolute gate'):
        M.check_bank_loudness('add_events', [-20.0, -np.inf], [3, 4])
