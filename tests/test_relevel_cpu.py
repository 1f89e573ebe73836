"""CPU: the host half of "Levels measured after the effects" (utilities/relevel.py, the plan's ``target_db``) and its float64 reference
(tests/relevel_ref.py): on the reference alone, that no block of a GPU case lies at a gate threshold (the condition under which
tests/test_relevel_gpu.py compares the counts exactly) and that the three planted faults - the tail measured twice, the whole source
measured instead of the excerpt, the 0.691 of the loudness formula dropped - move a gain past the bound the GPU test holds it to; the
record dtype against the library, the entry points' refusals, and the plans."""
import ctypes
import math
import types

import numpy as np
import pytest

import loudness_ref as LR
import relevel_cases as K
import relevel_ref as R
import soundscape_ref as S


def _mel(sr=16000):
    return types.SimpleNamespace(sr=sr, min_samples=513, hop=256, F=64)


def ulps(a, b):
    """the distance of two float32 values of one sign in units in the last place"""
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize('n_jobs', K.N_JOBS)
def test_no_block_of_a_gpu_case_lies_at_a_gate_threshold(n_jobs):
    """... within 1e-6 relative (loudness_ref.gate_clearance, the condition of tests/test_loudness_cpu.py).  Also: the cases contain
    what they are there for."""
    flat, offs, ns = K.layout(n_jobs)
    plan, ref = K.plan(n_jobs), K.reference(n_jobs, 'lufs')
    assert len(ref) == n_jobs == len(plan) and ns.tolist() == [p[0] for p in plan] and (offs % 4).tolist() == [p[2] for p in plan]
    assert (np.diff(offs) >= ns[:-1] + 5).all() and offs[0] >= 5 and len(flat) >= offs[-1] + ns[-1] + 5         # gaps all round
    for i, m in enumerate(ref):
        assert LR.gate_clearance(m['z'], m['thr']) > 1e-6, (i, plan[i])
        short = plan[i][0] < 4 * K.H
        assert m['counts'][3] == int(short) and m['counts'][0] == (1 if short else plan[i][0] // K.H - 3)
    rms = K.reference(n_jobs, 'rms')
    assert all(m['counts'] == [p[0], 0, 0, 0] for m, p in zip(rms, plan))
    if n_jobs == 270:
        assert {p[0] for p in plan} == set(K.LENGTHS[:-1]) and {p[1] for p in plan} == set(K.CONTENTS)
        assert {(p[0], p[2]) for p in plan} >= {(n, r) for n in (1, 257, K.H) for r in range(4)}        # every alignment at the edges
        by = lambda rs, kind: [m for m, p in zip(rs, plan) if p[1] == kind]
        assert all(m['status'] == 1 and m['gain'] is None for m in by(ref, 'zero') + by(ref, 'quiet') + by(rms, 'zero'))
        assert all(m['status'] == 0 and m['level'] > 0 for m in by(rms, 'quiet'))           # quiet has an RMS, but no loudness
        assert all(m['status'] == 0 for kind in ('steps', 'noise', 'dc') for m in by(ref, kind) + by(rms, kind))
    else:
        assert plan[0][0] // K.H > 256 and all(m['status'] == 0 for m in ref)               # a second round of hops
        assert any(m['counts'][2] < m['counts'][1] < m['counts'][0] for m in ref)           # both gates act


def test_reference_gains_bring_a_region_to_its_target():
    gen = np.random.default_rng(4)
    x = (0.03 * gen.standard_normal(7 * K.H + 5)).astype(np.float32)
    for mode in R.MODES:
        st, g = R.event_gain(-27.5, K.SR, mode, x, 0, len(x))
        assert st == 0 and g.dtype == np.float32
        assert abs(R.measured_db(x.astype(np.float64) * np.float64(g), K.SR, mode) + 27.5) < 1e-5        # (the wave stays float64 here)
    assert R.gain(1.0, 0.0) == (1, None) and R.gain(1.0, math.nan) == (1, None) and R.gain(1.0, math.inf) == (1, None)
    assert R.target_amplitude(-20.0, 'rms') == 0.1 and abs(R.target_amplitude(-20.691, 'lufs') - 0.1) < 1e-15


def test_three_planted_faults_are_caught():
    """an event cut from the quiet half of a source whose halves differ by 20 dB, and its wet row: each fault moves the gain by far more
    than the one float32 ulp tests/test_relevel_gpu.py allows"""
    gen = np.random.default_rng(6)
    half = 5 * K.H
    source = np.concatenate([0.2 * gen.standard_normal(half), 0.02 * gen.standard_normal(half)]).astype(np.float32)
    h = (gen.standard_normal(900) * np.exp(-6.0 * np.arange(900) / 900)).astype(np.float64)
    n = 4 * K.H + 77
    wet = np.convolve(source[half:half + n].astype(np.float64), h / np.sqrt(np.sum(h * h))).astype(np.float32)
    for mode in R.MODES:
        right = R.event_gain(-30.0, K.SR, mode, source, half, n)
        assert right[0] == 0 and ulps(right[1], R.event_gain(-30.0, K.SR, mode, source, half, n)[1]) == 0
        whole = R.event_gain(-30.0, K.SR, mode, source, half, n, fault='whole_source')
        assert whole[0] == 0 and ulps(right[1], whole[1]) > 1000 and float(right[1]) / float(whole[1]) > 5.0      # ~17 dB too quiet
        wet_right = R.event_gain(-30.0, K.SR, mode, source, half, n, row=wet, head=n)
        twice = R.event_gain(-30.0, K.SR, mode, source, half, n, row=wet, head=n, fault='tail_twice')
        assert wet_right[0] == 0 == twice[0] and ulps(wet_right[1], twice[1]) > 1000
    lufs = R.event_gain(-30.0, K.SR, 'lufs', source, half, n)
    plain = R.event_gain(-30.0, K.SR, 'lufs', source, half, n, fault='no_offset')
    assert ulps(lufs[1], plain[1]) > 1000 and abs(20.0 * math.log10(float(lufs[1]) / float(plain[1])) - 0.691) < 1e-5
    assert R.event_gain(-30.0, K.SR, 'rms', source, half, n, fault='no_offset')[1] == R.event_gain(-30.0, K.SR, 'rms', source, half, n)[1]


def test_job_records_and_targets():
    from sound_event_detection_transformer_amd import _build, lib
    from sound_event_detection_transformer_amd.utilities import relevel as M
    _build.build()
    assert M.JOB.itemsize == 40 == lib.load().sedt_sizeof(19) and lib.load().sedt_sizeof(20) == -1
    M.check_sizes()
    assert M.target_amplitude(-20.0) == 0.1 and M.target_amplitude([-20.0 - 0.691], 'lufs')[0] == R.target_amplitude(-20.691, 'lufs')
    assert all(M.target_amplitude(db, m) == R.target_amplitude(db, m) for db in (-36.0, -23.5, 0.0) for m in R.MODES)
    with pytest.raises(ValueError, match="neither 'rms' nor 'lufs'"):
        M.target_amplitude(-20.0, 'peak')
    jobs, doubles = M.relevel_jobs([3, 10000, 7], [1599, 1600, 6403], [0.1, 0.2, 0.3], ev=[2, 0, 1], tails=[-1, 0, -1], hop=1600)
    assert doubles == 1 + 2 + 5 and jobs['ws_off'].tolist() == [0, 1, 3] and jobs['ev'].tolist() == [2, 0, 1] and jobs['tail'].tolist() == [-1, 0, -1]
    assert jobs['off'].tolist() == [3, 10000, 7] and jobs['n'].tolist() == [1599, 1600, 6403] and jobs['target'].tolist() == [0.1, 0.2, 0.3]
    jobs0, doubles0 = M.relevel_jobs([3, 10000], [1599, 1600], [0.1, 0.2])
    assert doubles0 == 0 and jobs0['ws_off'].tolist() == [0, 0] and jobs0['ev'].tolist() == [-1, -1] == jobs0['tail'].tolist()
    l = lib.load()
    assert l.sedt_relevel_workspace(jobs.ctypes.data, 3, 1, 1600) == doubles and l.sedt_relevel_workspace(jobs.ctypes.data, 3, 0, 1600) == 3
    assert l.sedt_relevel_workspace(jobs0.ctypes.data, 2, 0, 1600) == 0 and l.sedt_relevel_workspace(jobs.ctypes.data, 0, 1, 1600) == 0
    for bad in ([(0, 0, 0.1)], [(-1, 5, 0.1)], [(0, 5, 0.0)], [(0, 5, math.nan)], [(0, 5, math.inf)]):
        with pytest.raises(ValueError, match='relevel_jobs: region 0'):
            M.relevel_jobs([b[0] for b in bad], [b[1] for b in bad], [b[2] for b in bad])
    with pytest.raises(ValueError, match='one offset, one length, one target'):
        M.relevel_jobs([0, 1], [5], [0.1])
    for n_jobs, mode, hop in ((3, 2, 1600), (3, 1, 0), (-1, 1, 1600)):
        assert l.sedt_relevel_workspace(jobs.ctypes.data, n_jobs, mode, hop) == -1 and 'relevel_workspace' in l.sedt_last_error().decode()
    assert l.sedt_relevel_workspace(None, 1, 1, 1600) == -1
    out_of_order = jobs.copy()
    out_of_order['ws_off'] = [0, 0, 3]
    assert l.sedt_relevel_workspace(out_of_order.ctypes.data, 3, 1, 1600) == -1 and 'job 1 has ws_off=0' in l.sedt_last_error().decode()
    with pytest.raises(ValueError, match="neither 'rms' nor 'lufs'"):
        M.DeviceRelevel(16000, 'peak', device='cpu')


def test_entry_point_refuses_before_any_launch():
    """the host copy of the records is checked at the entry point: nothing is launched, so the other pointers - host memory here, never
    dereferenced - only have to be non-null and aligned"""
    from sound_event_detection_transformer_amd import _build, lib
    from sound_event_detection_transformer_amd.utilities import relevel as M
    _build.build()
    l = lib.load()
    jobs, doubles = M.relevel_jobs([0, 2000, 4001], [1600, 2000, 6400], [0.1, 0.1, 0.1], ev=[0, 1, 2], tails=[-1, 0, -1], hop=1600)
    dummy = np.zeros(64, np.float64)
    d = dummy.ctypes.data

    def call(j=jobs, n_jobs=3, flat_len=20000, mode=1, hop=1600, z_abs=LR.Z_ABS, work_len=doubles, n_ev=3, n_tails=1, flat=d, jobs_dev=d):
        return l.sedt_relevel(flat, flat_len, j.ctypes.data, jobs_dev, n_jobs, mode, d, d, hop, z_abs, d, work_len, d, n_ev, d, n_tails, d, d, d,
                              None)

    def refused(match, **kw):
        assert call(**kw) != 0 and match in l.sedt_last_error().decode(), l.sedt_last_error().decode()

    def edit(i, **fields):
        j = jobs.copy()
        for k, v in fields.items():
            j[k][i] = v
        return j

    refused('null pointer', flat=None)
    refused('null pointer', jobs_dev=None)
    refused('n_jobs=-1', n_jobs=-1)
    refused('flat_len=-1', flat_len=-1)
    refused('mode=2', mode=2)
    refused('hop=0', hop=0)
    refused('z_abs', z_abs=math.nan)
    refused('job 2 (samples 4001 .. +6400) does not lie inside the 10400 samples given', flat_len=10400)
    refused('job 1 (samples 18001', j=edit(1, off=18001))
    refused('job 0 is the region off=-1', j=edit(0, off=-1))
    refused('job 1 is the region off=2000 n=0', j=edit(1, n=0))
    refused('job 1 names event record 3 of 3', j=edit(1, ev=3))
    refused('job 2 names event record 2 of 3 and tail record 1 of 1', j=edit(2, tail=1))
    refused('job 0 names event record -2', j=edit(0, ev=-2))
    refused('job 2 has target=', j=edit(2, target=math.nan))
    refused('job 1 has ws_off=1: the regions lie in job order', j=edit(1, ws_off=1))
    refused(f'work_len={doubles - 1} is too small: the jobs need {doubles} doubles', work_len=doubles - 1)
    assert call(n_jobs=0) == 0                                                              # nothing to do: nothing launched


def test_plans_carry_target_db():
    from sound_event_detection_transformer_amd.utilities import soundscape as M
    labels = [f'c{i}' for i in range(10)]
    ns, rms = [5, 4000, 90000, 700], np.asarray([0.5, 0.01, 0.2, 0.0])
    by_class, backgrounds = [[0, 1]] + [[] for _ in range(9)], [2, 3]
    np.random.seed(9)
    plan = M.draw_plan(6, ns, rms, by_class, backgrounds, 16000, 16000, ref_db=-40.0)
    after = np.random.random_sample(2)
    np.random.seed(9)
    bg, ev, off = S.draw(6, ns, rms, by_class, backgrounds, 16000, 16000, ref_db=-40.0)
    assert np.array_equal(after, np.random.random_sample(2))                                # no randomness is consumed for it
    assert plan.ev.tobytes() == ev.tobytes() and plan.bg.tobytes() == bg.tobytes() and len(ev) > 6
    assert plan.target_db.dtype == np.float64 and plan.target_db.shape == ev.shape
    assert ((plan.target_db >= -34.0) & (plan.target_db <= -10.0)).all() and len(set(plan.target_db.tolist())) == len(ev)
    for e, t in zip(plan.ev, plan.target_db):                                               # ref_db + snr: the level the host's gain aimed at
        assert e['gain'] == np.float32(np.float64(10.0) ** (t / np.float64(20.0)) / rms[e['src']])
    np.random.seed(9)
    fx = M.draw_plan(6, ns, rms, by_class, backgrounds, 16000, 16000, ref_db=-40.0, pitch_shift=(-2.0, 2.0), time_stretch=(0.8, 1.25))
    assert fx.target_db.shape == fx.ev.shape and fx.fx is not None
    events = [[(1, 0, 0, 100, 5, 0.5, 0)], [], [(0, 0, 0, 5, 0, 1.0, 0), (1, 0, 10, 20, 30, 1.0, 2)]]
    hand = M.make_plan([None] * 3, events, levels=[[-30.0], [], [-20.5, -41.0]])
    assert hand.target_db.tolist() == [-30.0, -20.5, -41.0] and M.make_plan([None] * 3, events).target_db is None
    for levels in ([[-30.0], [], [-20.5]], [[-30.0], [-1.0]]):
        with pytest.raises(ValueError, match='levels holds one list per clip, one level per event'):
            M.make_plan([None] * 3, events, levels=levels)
    with pytest.raises(ValueError, match='target_db'):
        M.SoundscapePlan(hand.bg, hand.ev, hand.ev_off, target_db=[-30.0])
    s = M.SoundscapeClips(_mel(), labels, 1.0, device='cpu')
    assert s.relevel is False and M.SoundscapeClips(_mel(), labels, 1.0, device='cpu', relevel=True).relevel is True
    assert s.plan([None] * 3, events, levels=[[-30.0], [], [-20.5, -41.0]]).target_db.tolist() == [-30.0, -20.5, -41.0]
