"""CPU: the float64 restatement of the reverb stage (tests/reverb_ref.py) against the direct form on every row of tests/reverb_cases.py, the
named edges of the table, planted faults, the host half of utilities/reverb.py (jobs, regions, tables, refusals) and the order in which
SoundscapeClips' draw consumes np.random with and without ``reverb``."""
import math

import numpy as np
import pytest

import reverb_cases as K
import reverb_ref as R
from sound_event_detection_transformer_amd.utilities import reverb as M
from sound_event_detection_transformer_amd.utilities import soundscape as SC

ROWS = list(range(len(K.ROWS)))


def test_every_named_edge_is_reached():
    hit = K.edges()
    print({k: v for k, v in hit.items()})
    assert all(len(v) for v in hit.values()), [k for k, v in hit.items() if not v]
    assert {r[1] for r in K.ROWS if r[0] == 512} == set(K.LENGTHS)
    assert set(K.TAPS) <= {r[2] for r in K.ROWS if r[0] == 512}
    for n in K.LENGTHS:                                      # every length meets a single partition and more than one
        ps = {R.counts(r[1], r[2], 512)[1] > 1 for r in K.ROWS if r[0] == 512 and r[1] == n}
        assert ps == {False, True}, n


def _rel(a, b):
    scale = float(np.abs(b).max(initial=0.0))
    return float(np.abs(a - b).max(initial=0.0)) / (scale if scale else 1.0)


@pytest.mark.parametrize('row', ROWS)
def test_the_partitioned_chain_equals_the_direct_form(row):
    N, n, L, fade, _, kind = K.ROWS[row]
    ref = K.reference(row)
    nb, P, nout, total = R.counts(n, L, N)
    assert ref['H'].shape == (P, N // 2 + 1) and ref['X'].shape == (nb, N // 2 + 1) and ref['wet'].shape == ref['direct'].shape == (total,)
    assert _rel(ref['wet'], ref['direct']) <= 1e-12
    xf = R.faded(K.signal(row), fade)
    if kind == 'unit':                                       # wet = the faded dry sound, then zeros
        assert np.array_equal(ref['direct'][:n], xf) and not ref['direct'][n:].any()
    if kind == 'lag':                                        # ... or the faded dry sound L - 1 samples later
        assert np.array_equal(ref['direct'][L - 1:], xf) and not ref['direct'][:L - 1].any()


@pytest.mark.parametrize('row', ROWS)
def test_the_float32_restatement_passes_every_stage_bound(row):
    N, n, L, fade, _, _ = K.ROWS[row]
    x, h, ref = K.signal(row), K.response(row), K.reference(row)
    H32, X32 = R.partition_spectra(h, N, np.float32), R.block_spectra(x, fade, N, np.float32)
    assert H32.dtype == X32.dtype == np.complex64
    assert (np.abs(H32 - ref['H']).max(axis=1) <= R.spectra_bound(h, N)).all()
    assert (np.abs(X32 - ref['X']).max(axis=1) <= R.blocks_bound(x, fade, N)).all()
    wet32 = R.mac_inverse(X32, H32, n, L, N, np.float32)
    assert wet32.dtype == np.float32
    assert (np.abs(wet32 - R.mac_inverse(X32, H32, n, L, N)) <= R.wet_bound(X32, H32, n, L, N)).all()


def test_fft32_is_a_fourier_transform():
    gen = np.random.default_rng(1)
    for N in (2, 8, 512):
        v = gen.standard_normal((3, N)).astype(np.float32)
        assert np.abs(R.rfft(v, np.float32) - np.fft.rfft(v.astype(np.float64))).max() <= 8 * R.EPS * math.log2(N) * np.abs(v).sum(axis=1).max()
        back = R.irfft(R.rfft(v, np.float32), N, np.float32)
        assert back.dtype == np.float32 and np.abs(back - v).max() <= 1e-5


@pytest.mark.parametrize('fault', R.FAULTS)
def test_a_planted_fault_is_caught_by_the_direct_form(fault):
    caught = []
    for row in ROWS:
        N, n, L, fade, _, _ = K.ROWS[row]
        if L > 4096:
            continue
        ref = K.reference(row)
        wet = R.mac_inverse(ref['X'], ref['H'], n, L, N, fault=fault)
        if _rel(wet, ref['direct']) > 1e-12:
            caught.append(row)
    print(fault, 'is caught on rows', caught)
    assert len(caught) >= len(ROWS) // 2, (fault, caught)


def test_fades_are_those_of_the_mixing_call():
    import soundscape_ref as S
    for n, fade in ((1, 0), (1, 5), (600, 16), (600, 400), (255, 8), (10, 0)):
        i = np.arange(n, dtype=np.int64)
        assert R.fade_weight(n, fade).tobytes() == S.fade_weight(i, n, fade).tobytes()


# ---------------------------------------------------------------------- the host half of the stage
def test_jobs_regions_and_the_workspace_they_ask_for():
    from sound_event_detection_transformer_amd import lib as L
    M.check_sizes()
    assert M.JOB.itemsize == 40 == L.load().sedt_sizeof(16) and M.TAIL.itemsize == 40 == L.load().sedt_sizeof(17)
    assert M.BED.itemsize == 32 == L.load().sedt_sizeof(18)
    ns, rirs, lens = [1, 257, 3000, 600], [1, 0, 1, 2], [700, 1, 256]
    jobs, floats = M.reverb_jobs(ns, rirs, lens, 512, fades=[0, 3, 16, 400])
    assert jobs['src_off'].tolist() == [0, 1, 258, 3258] and jobs['rir'].tolist() == rirs and jobs['fade'].tolist() == [0, 3, 16, 400]
    assert jobs['dst_off'].tolist() == [0, 4, 960, 3960] and all(o % 4 == 0 for o in jobs['ws_off'].tolist())
    for e in range(4):
        nb = R.counts(ns[e], lens[rirs[e]], 512)[0]
        assert M.blocks_in(ns[e], 512) == nb and M.job_floats(512, ns[e]) == (2 * nb * 257 + 3) & ~3
        assert M.blocks_out(ns[e], lens[rirs[e]], 512) == R.counts(ns[e], lens[rirs[e]], 512)[2]
        reg = M.regions(jobs[e], 512)
        assert reg['X_re'] == (int(jobs['ws_off'][e]), (nb, 257)) and reg['X_im'] == (int(jobs['ws_off'][e]) + nb * 257, (nb, 257))
        assert reg['X_im'][0] + nb * 257 <= (int(jobs['ws_off'][e + 1]) if e < 3 else floats)
    assert L.load().sedt_reverb_workspace(jobs.ctypes.data, 4, 512) == 4 * floats
    placed, _ = M.reverb_jobs(ns, rirs, lens, 512, src_offs=[10, 20, 30, 40], dst_offs=[0, 1000, 2000, 8000])
    assert placed['src_off'].tolist() == [10, 20, 30, 40] and placed['dst_off'].tolist() == [0, 1000, 2000, 8000]
    bad = jobs.copy()
    bad['ws_off'][2] -= 4
    assert L.load().sedt_reverb_workspace(bad.ctypes.data, 4, 512) == -1 and b'ws_off' in L.load().sedt_last_error()
    assert L.load().sedt_reverb_workspace(jobs.ctypes.data, -1, 512) == -1 and L.load().sedt_reverb_workspace(jobs.ctypes.data, 4, 256) == -1
    assert L.load().sedt_reverb_workspace(None, 4, 512) == -1
    ok = L.load().sedt_reverb_ok
    assert ok(512, 1, 1, 0) == 1 and ok(2048, 2 ** 26, 176 * 1024, 5) == 1 and ok(2048, 441000, 4 * 44100, 441) == 1
    assert ok(512, 0, 1, 0) == 0 and ok(512, 1, 0, 0) == 0 and ok(512, 1, 176 * 256 + 1, 0) == 0 and ok(512, 1, 1, -1) == 0
    assert ok(256, 1, 1, 0) == 0 and ok(512, 2 ** 26 + 1, 1, 0) == 0


def test_the_rir_table():
    table, parts = M.rir_table([700, 1, 256, 257], 512)
    assert table.dtype == np.int64 and table.tolist() == [[700, 1, 256, 257], [0, 3, 4, 5], [0, 700, 701, 957]] and parts == 7
    assert M.max_taps(2048) >= 4 * 44100 and M.MAX_PART == K.MAX_PART


def test_refusals():
    ok = dict(n=1000, taps=300, fade=16, n_fft=512)
    M.check_shape(**ok)
    for bad in (dict(n=0), dict(n=-5), dict(n=2 ** 26 + 1), dict(n=10.5), dict(taps=0), dict(taps=176 * 256 + 1), dict(fade=-1),
                dict(n_fft=256), dict(n_fft=4096)):
        with pytest.raises(ValueError, match='outside the envelope'):
            M.check_shape(**{**ok, **bad})
    with pytest.raises(ValueError, match='one response index'):
        M.reverb_jobs([10, 20], [0], [5])
    with pytest.raises(ValueError, match='names response 1 of 1'):
        M.reverb_jobs([10, 20], [0, 1], [5])
    with pytest.raises(ValueError, match='outside the envelope'):
        M.DeviceReverb(16000, n_fft=256, device='cpu')
    f = lambda *v: np.asarray(v, np.float32)
    for rirs, match in (([f()], 'is empty'), ([f(1.0, np.nan)], 'non-finite'), ([f(0.5), f(np.inf)], 'response 1 holds non-finite'),
                        ([f(0.0, 0.0)], 'all zero'), ([np.zeros(176 * 256 + 1, np.float32)], 'more than 176 partitions'),
                        ([np.ones((2, 2), np.float32)], 'not a 1-D'), ([np.ones(3, np.float64)], 'not a 1-D float32')):
        with pytest.raises(ValueError, match=match):
            M.prepare_rirs(rirs, 512)
    with pytest.raises(ValueError, match='neither'):
        M.prepare_rirs([f(1.0)], 512, normalize='peak')
    h, q = M.prepare_rirs([f(3.0, 4.0), np.asarray([16384, -16384], np.int16)], 512)
    assert h.dtype == np.float32 and np.allclose(h, [0.6, 0.8]) and np.allclose(q, [math.sqrt(0.5), -math.sqrt(0.5)])
    assert M.prepare_rirs([f(3.0, 4.0)], 512, normalize=None)[0].tolist() == [3.0, 4.0]


# ---------------------------------------------------------------------- plans
LENS = [700, 5000, 20000, 3, 40000]
LEVEL = [0.1, 0.2, 0.05, 0.3, 0.01]
BY_CLASS = [[0], [1, 2], [], [3]]
ROOMS = [[0, 3], [1], [2, 4, 5]]


def _draw(seed, **kw):
    np.random.seed(seed)
    return SC.draw_plan(6, LENS, LEVEL, BY_CLASS, [4], 16000, 16000, n_events=(1, 5), max_event_seconds=0.8, **kw)


def _restated(seed, reverb, effects=False):
    """the documented order, written out again: room after the background, wet / rir after the effects and before src_start"""
    np.random.seed(seed)
    classes = [c for c, own in enumerate(BY_CLASS) if own]
    cap, fade, window = 12800, 160, 16000
    ev, rir, off, bgs = [], [], [0], []
    for b in range(6):
        bgs.append((4, np.random.randint(LENS[4])) if np.random.randint(1) == 0 else None)
        room = ROOMS[np.random.randint(len(ROOMS))]
        for _ in range(np.random.randint(1, 6)):
            c = classes[np.random.randint(len(classes))]
            s = BY_CLASS[c][np.random.randint(len(BY_CLASS[c]))]
            snr = np.random.uniform(6.0, 30.0)
            n = m = min(LENS[s], cap, window)
            if effects:
                p = np.float32(np.random.uniform(-3.0, 3.0))
                f = np.float32(np.random.uniform(0.8, 1.2))
                n = min(LENS[s], SC.excerpt_for(min(cap, window), float(f)))
                m = int(math.floor(n * float(f) + 0.5))
            wet = True if reverb is True else bool(np.random.uniform() < reverb)
            rir.append(room[np.random.randint(len(room))] if wet else -1)
            src_start = np.random.randint(LENS[s] - n + 1)
            onset = np.random.randint(window - m + 1)
            ev.append((s, c, src_start, n, onset, SC.gains(-30.0, snr, LEVEL[s]), fade))
        off.append(len(ev))
    return bgs, np.array(ev, SC.EVENT), np.asarray(rir, np.int32), off


@pytest.mark.parametrize('seed', [3, 4, 5])
def test_a_plan_without_reverb_is_the_plan_it_was(seed):
    import soundscape_ref as S
    a, b = _draw(seed), _draw(seed, reverb=None, rooms=ROOMS)
    assert a.rir is None and b.rir is None
    assert a.bg.tobytes() == b.bg.tobytes() and a.ev.tobytes() == b.ev.tobytes() and a.ev_off.tobytes() == b.ev_off.tobytes()
    np.random.seed(seed)
    bg, ev, off = S.draw(6, LENS, LEVEL, BY_CLASS, [4], 16000, 16000, (1, 5), (6.0, 30.0), -30.0, 0.8, 0.01)
    assert a.bg.tobytes() == bg.tobytes() and a.ev.tobytes() == ev.tobytes() and a.ev_off.tobytes() == off.tobytes()
    fx0, fx1 = _draw(seed, pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2)), _draw(seed, pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2), reverb=None)
    assert fx0.ev.tobytes() == fx1.ev.tobytes() and fx0.fx.tobytes() == fx1.fx.tobytes() and fx1.rir is None


@pytest.mark.parametrize('seed', [3, 4, 5])
@pytest.mark.parametrize('reverb', [True, 0.5, 1.0])
def test_a_plan_with_reverb_is_drawn_in_the_documented_order(seed, reverb):
    plan = _draw(seed, reverb=reverb, rooms=ROOMS)
    bgs, ev, rir, off = _restated(seed, reverb)
    assert plan.rir.dtype == np.int32 and plan.rir.tobytes() == rir.tobytes() and plan.ev.tobytes() == ev.tobytes()
    assert plan.ev_off.tolist() == off and plan.bg['start'].tolist() == [g[1] for g in bgs]
    for b in range(6):                                       # one room per clip
        own = {int(r) for r in plan.rir[off[b]:off[b + 1]] if r >= 0}
        assert any(own <= set(room) for room in ROOMS)
    if reverb is True or reverb == 1.0:
        assert (plan.rir >= 0).all()
    else:
        assert (plan.rir >= 0).any() and (plan.rir < 0).any()
    # n, m and the onset are drawn as before: the head fits the window, the tail is not made to
    assert ((plan.ev['onset'] + plan.ev['n']) <= 16000).all()
    both = _draw(seed, reverb=reverb, rooms=ROOMS, pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2))
    _, ev2, rir2, _ = _restated(seed, reverb, effects=True)
    assert both.ev.tobytes() == ev2.tobytes() and both.rir.tobytes() == rir2.tobytes() and both.fx.shape == both.ev.shape


def test_reverb_arguments_are_checked():
    for bad in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match='probability'):
            _draw(3, reverb=bad, rooms=ROOMS)
    with pytest.raises(ValueError, match='add_rirs'):
        _draw(3, reverb=True, rooms=[])
    with pytest.raises(ValueError, match='add_rirs'):
        _draw(3, reverb=0.5)


def test_make_plan_round_trips_rir():
    events = [[(0, 1, 5, 100, 7, 0.5, 3), (1, 0, 0, 50, 0, 1.0, 0)], [], [(2, 2, 1, 10, 2, 0.25, 0, 0.0, 1.0)]]
    plan = SC.make_plan([None, (4, 10, 0.5), None], events, rirs=[[2, -1], [], [0]])
    assert plan.rir.dtype == np.int32 and plan.rir.tolist() == [2, -1, 0] and plan.fx is not None
    assert SC.make_plan([None, (4, 10, 0.5), None], events).rir is None
    again = SC.SoundscapePlan(plan.bg, plan.ev, plan.ev_off, plan.fx, plan.rir)
    assert again.rir.tobytes() == plan.rir.tobytes()
    with pytest.raises(ValueError, match='rir'):
        SC.SoundscapePlan(plan.bg, plan.ev, plan.ev_off, rir=plan.rir[:2])
    with pytest.raises(ValueError, match='one list per clip'):
        SC.make_plan([None, None, None], events, rirs=[[2], [], [0]])


# ---------------------------------------------------------------------- the bed and the split
def test_the_bed_and_the_split():
    gen = np.random.default_rng(9)
    bg = gen.standard_normal(50).astype(np.float32)
    wet_a, wet_b = gen.standard_normal(40).astype(np.float32), gen.standard_normal(30).astype(np.float32)
    head, tail = R.split(wet_a, 25)
    assert len(head) == 25 and len(tail) == 15 and np.array_equal(np.concatenate([head, tail]), wet_a)
    out = R.bed(64, bg, 45, 0.5, [(2.0, wet_a, 10, 25), (0.25, wet_b, 50, 10)])
    want = (np.float32(0.5) * bg[(45 + np.arange(64)) % 50]).astype(np.float32)
    assert out.dtype == np.float32 and np.array_equal(out[:35], want[:35]) and np.array_equal(out[50:60], want[50:60])
    assert np.array_equal(out[35:50], (want[35:50] + (np.float32(2.0) * wet_a[25:40]).astype(np.float32)).astype(np.float32))
    assert np.array_equal(out[60:64], (want[60:64] + (np.float32(0.25) * wet_b[10:14]).astype(np.float32)).astype(np.float32))   # cut at the window
    assert not R.bed(16, None, 0, 1.0, []).any()
