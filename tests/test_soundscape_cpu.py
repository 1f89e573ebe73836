"""CPU: the host half of the soundscape synthesis (utilities/soundscape.py) and its NumPy reference (tests/soundscape_ref.py): the restated
collapse against the reference's own (tests/golden/g25_collapse.npz), the seeded plan, the gains, the refusals, the shared blob layout,
the entry points' argument checks - and, on the reference alone, that the designed inputs of the GPU test contain what they are there for."""
import os
import types

import numpy as np
import pytest

import soundscape_cases as K
import soundscape_ref as S
from conftest import GOLDEN


def _mel():
    return types.SimpleNamespace(sr=K.SR, min_samples=513, hop=256, F=64)


def test_restated_collapse_equals_the_reference_fixture():
    g = np.load(os.path.join(GOLDEN, 'g25_collapse.npz'))
    assert int(g['sr']) == 16000 and int(g['n_files']) == 7
    removed = 0
    for f in range(int(g['n_files'])):
        i, o = g['in_file'] == f, g['out_file'] == f
        events = list(zip(g['in_cls'][i].tolist(), g['in_on'][i].tolist(), g['in_end'][i].tolist()))
        want = set(zip(g['out_cls'][o].tolist(), g['out_on'][o].tolist(), g['out_end'][o].tolist()))
        got = S.collapse(events)
        assert len(got) == len(set(got)) and set(got) == want, (str(g['names'][f]), got, want)
        assert S.collapse(events[::-1]) == got                       # the input order does not matter
        removed += len(events) - len(got)
    names = g['names'].tolist()
    count = lambda n, which: int((g[which] == names.index(n)).sum())
    assert removed == 10 and count('empty', 'in_file') == 0 == count('empty', 'out_file')
    assert count('touching', 'out_file') == 1 and count('disjoint', 'out_file') == 3 and count('chained', 'out_file') == 1
    assert count('nested', 'out_file') == 1 and count('single', 'out_file') == 1 and count('interleaved', 'out_file') == 6


def _toy_bank():
    lens = [5, 4000, 90000, 16000, 700, 48000]
    rms = [0.5, 0.01, 0.2, 0.07, 0.0, 0.03]
    by_class = [[], [0, 1], [], [2], [3]] + [[] for _ in range(5)]
    return lens, rms, by_class, [4, 5]


@pytest.mark.parametrize('kw', [{}, {'n_events': (0, 5), 'snr_db': (-3.0, 12.0), 'ref_db': -40.0, 'max_event_seconds': 0.5, 'fade_seconds': 0.0},
                                {'background': False, 'n_events': (63, 63)}])
def test_seeded_draw_equals_the_restated_draw(kw):
    from sound_event_detection_transformer_amd.utilities import soundscape as M
    assert M.EVENT == S.EVENT and M.BACKGROUND == S.BACKGROUND and M.EVENT.itemsize == 40 and M.BACKGROUND.itemsize == 24
    lens, rms, by_class, bgs = _toy_bank()
    window = 32000
    np.random.seed(31)
    plan = M.draw_plan(6, lens, rms, by_class, bgs, window, K.SR, **kw)
    after = np.random.random_sample(3)
    np.random.seed(31)
    bg, ev, off = S.draw(6, lens, rms, by_class, bgs, window, K.SR, **kw)
    assert np.array_equal(after, np.random.random_sample(3))         # np.random was consumed identically
    assert plan.bg.tobytes() == bg.tobytes() and plan.ev.tobytes() == ev.tobytes() and plan.ev_off.tolist() == off.tolist()
    assert len(plan) == 6 and len(plan.events(0)) == off[1]
    # what a plan promises: events inside their sources and inside the window
    for e in plan.ev:
        assert 0 <= e['src_start'] and e['src_start'] + e['n'] <= lens[e['src']] and 0 <= e['onset'] and e['onset'] + e['n'] <= window
        assert e['cls'] in (1, 3, 4) and e['src'] in by_class[e['cls']] and e['n'] >= 1
    if kw.get('background', True):
        assert set(plan.bg['src'].tolist()) <= {4, 5} and all(0 <= g['start'] < lens[g['src']] for g in plan.bg)
        assert all(g['gain'] == 1.0 for g in plan.bg if g['src'] == 4)                     # the silent background
    else:
        assert (plan.bg['src'] == -1).all() and (np.diff(plan.ev_off) == 63).all()
    if 'max_event_seconds' in kw:
        assert plan.ev['n'].max() <= 8000 and (plan.ev['fade'] == 0).all()
    else:
        assert (plan.ev['fade'] == 160).all()


def test_gains_match_the_float64_formula():
    from sound_event_detection_transformer_amd.utilities import soundscape as M
    for ref_db, snr, rms in ((-30.0, 6.0, 0.1), (-30.0, 29.99, 0.0123), (-40.0, -3.5, 2.5), (0.0, 0.0, 1.0)):
        want = np.float32(10.0 ** ((ref_db + snr) / 20.0) / rms)
        assert M.gains(ref_db, snr, rms) == want == S.gain(ref_db, snr, rms) and M.gains(ref_db, snr, rms).dtype == np.float32
    assert M.gains(-30.0, 0.0, 0.0) == 1.0 == S.gain(-30.0, 0.0, 0.0)
    assert M.gains(-30.0, 0.0, 0.5) == np.float32(10.0 ** (-30.0 / 20.0) / 0.5)           # a background: snr 0
    # an event at `snr` dB over a background: the ratio of the two scaled RMS values is 10^(snr / 20)
    g_ev, g_bg = float(M.gains(-30.0, 12.0, 0.2)), float(M.gains(-30.0, 0.0, 0.05))
    assert abs(20.0 * np.log10((g_ev * 0.2) / (g_bg * 0.05)) - 12.0) < 1e-5


def test_refusals():
    from sound_event_detection_transformer_amd.utilities import soundscape as M
    scapes = M.SoundscapeClips(_mel(), K.LABELS, 1.0, device='cpu')
    assert scapes.window == 16000 and scapes.max_targets == 32 and scapes.collapse and scapes.peak_limit == 1.0
    with pytest.raises(ValueError, match="class 'Bird' is not one of the 10 labels"):
        scapes.add_events([np.ones(8, np.float32)], ['Bird'])
    with pytest.raises(ValueError, match='class 10 is not one of the 10 labels'):
        scapes.add_events([np.ones(8, np.float32)], [10])
    with pytest.raises(ValueError, match='source 0 is empty'):
        scapes.add_events([np.ones(0, np.float32)], ['c1'])
    with pytest.raises(ValueError, match='the bank is empty'):
        scapes.draw(4)
    assert len(scapes) == 0
    # what the staging does with the statistics the device returns
    M.check_bank_stats('add_backgrounds', np.asarray([0.0, 2.5]), [-1, -1])                # a silent background is allowed
    with pytest.raises(ValueError, match='source 1 is silent'):
        M.check_bank_stats('add_events', np.asarray([1.0, 0.0]), [3, 4])
    for q in (np.nan, np.inf):
        with pytest.raises(ValueError, match='source 0 holds non-finite samples'):
            M.check_bank_stats('add_backgrounds', np.asarray([q]), [-1])
    lens, rms, by_class, bgs = _toy_bank()
    with pytest.raises(ValueError, match='up to 64 events per clip asked for, sedt_soundscape takes 63'):
        M.draw_plan(2, lens, rms, by_class, bgs, 32000, K.SR, n_events=(1, 64))
    with pytest.raises(ValueError, match='the bank is empty'):
        M.draw_plan(2, lens, rms, [[] for _ in range(10)], bgs, 32000, K.SR)
    with pytest.raises(ValueError, match='no background recording is staged'):
        M.draw_plan(2, lens, rms, by_class, [], 32000, K.SR)
    with pytest.raises(ValueError, match='a clip holds 64 events'):
        M.make_plan([None, None], [[], [(0, 1, 0, 1, 0, 1.0, 0)] * 64])
    assert len(M.make_plan([None], [[(0, 1, 0, 1, 0, 1.0, 0)] * 63]).ev) == 63
    for bad in ({'max_targets': 0}, {'max_targets': 64}, {'peak_limit': 0.0}, {'peak_limit': float('nan')},
                {'min_event_seconds': float('nan')}):
        with pytest.raises(ValueError):
            M.SoundscapeClips(_mel(), K.LABELS, 1.0, device='cpu', **bad)
    with pytest.raises(ValueError, match='what the front end needs'):
        M.SoundscapeClips(_mel(), K.LABELS, 0.01, device='cpu')


def test_hand_made_plan_and_shared_blob_layout():
    from sound_event_detection_transformer_amd import lib
    from sound_event_detection_transformer_amd.utilities import recording_clips, soundscape as M
    import recording_clips_ref as R
    assert M.blob_layout is recording_clips.blob_layout and M.DeviceTargets is recording_clips.DeviceTargets
    assert lib.SCAPE_MAXEV == S.MAXEV == 63 and lib.SCAPE_MAXB == 1024 and lib.SCAPE_CHUNK == 2048
    assert set(M.STATUS_REASONS) == {1, 2} == set(M.SoundscapeClips.STATUS_REASONS)
    chosen = K.pick(4096, 5)
    bg, ev, off = K.records(chosen)
    plan = M.make_plan([g for g, _ in chosen], [e for _, e in chosen])
    assert plan.bg.tobytes() == bg.tobytes() and plan.ev.tobytes() == ev.tobytes() and plan.ev_off.tolist() == off.tolist()
    by_name = M.SoundscapeClips(_mel(), K.LABELS, 1.0, device='cpu').plan([None], [[(2, 'c7', 0, 5, 9, 0.5, 0)]])
    assert by_name.ev[0]['cls'] == 7 and by_name.ev[0]['onset'] == 9 and by_name.bg[0]['src'] == -1
    sounds, _, backgrounds = K.bank()
    _, _, _, targets, _ = S.soundscape(sounds + backgrounds, bg, ev, off, 4096, K.SR, 63)
    assert R.blob(targets, 63)[3] == M.blob_layout(5, 63)[1:]


def test_entry_points_refuse_outside_the_envelope():
    """refused with a message before a pointer is touched (every pointer here is null)"""
    from sound_event_detection_transformer_amd import _build, lib
    _build.build()
    l = lib.load()
    assert l.sedt_sizeof(13) == S.EVENT.itemsize == 40 and l.sedt_sizeof(14) == S.BACKGROUND.itemsize == 24
    call = lambda B=4, M=32, window=160000, sr=16000, n_src=1, min_len=0.0, limit=1.0: l.sedt_soundscape(
        None, 0, None, None, n_src, None, None, None, B, window, sr, M, min_len, 1, limit, None, None, None, None, None, None, None)
    for B, M in ((0, 32), (1025, 32), (-1, 32), (4, 0), (4, 64)):
        assert call(B, M) != 0
        msg = l.sedt_last_error().decode()
        assert f'B={B} max_targets={M} outside the envelope' in msg and '1024' in msg and '63' in msg, msg
    assert call(window=0) != 0 and 'window=0' in l.sedt_last_error().decode()
    assert call(window=2 ** 31) != 0 and 'window=2147483648' in l.sedt_last_error().decode()
    assert call(sr=0) != 0 and 'sr=0' in l.sedt_last_error().decode()
    assert call(n_src=0) != 0 and 'n_src=0' in l.sedt_last_error().decode()
    assert call(min_len=float('nan')) != 0 and 'min_event_seconds is NaN' in l.sedt_last_error().decode()
    for limit in (float('nan'), 0.0, -1.0):
        assert call(limit=limit) != 0 and 'peak_limit' in l.sedt_last_error().decode()
    assert call(1024, 63) != 0 and 'null pointer' in l.sedt_last_error().decode()          # inside the envelope: the pointers are looked at
    assert l.sedt_bank_stats(None, 0, None, None, 0, None, None, None) != 0 and 'n_src=0' in l.sedt_last_error().decode()
    assert l.sedt_bank_stats(None, -1, None, None, 1, None, None, None) != 0 and 'flat_len=-1' in l.sedt_last_error().decode()
    assert l.sedt_bank_stats(None, 0, None, None, 3, None, None, None) != 0 and 'null pointer' in l.sedt_last_error().decode()


# ---------------------------------------------------------------------------------------------------- the designed GPU inputs
@pytest.mark.parametrize('W', K.WINDOWS)
def test_designed_inputs_contain_what_they_are_there_for(W):
    sounds, classes, backgrounds = K.bank()
    sources = sounds + backgrounds
    lens = [len(s) for s in sources]
    assert lens == K.EVENT_LENS + K.BG_LENS == [1, 3, 700, 5000, 20000, 700, 20000] and classes == [0, 1, 2, 3, 4]
    chosen = K.clips(W)
    bg, ev, off = K.records(chosen)
    on = S.soundscape(sources, bg, ev, off, W, K.SR, 63, 0.0, True, 1.0)
    offc = S.soundscape(sources, bg, ev, off, W, K.SR, 63, 0.0, False, 1.0)
    wave, peak, scale, targets, status = on
    assert not status.any() and not offc[4].any() and np.array_equal(wave, offc[0])
    n_on, n_off = [len(t[0]) for t in targets], [len(t[0]) for t in offc[3]]
    assert sum(a < b for a, b in zip(n_on, n_off)) >= 3                                    # collapse removes an event in three clips
    assert sum(len(e) == 0 for _, e in chosen) >= 2 and n_on[1] == 0 and n_on[0] > 0 and n_on[2] > 0
    assert (scale < 1).any() and scale[5] < 1 and peak[5] > 1 and abs(np.abs(wave[5]).max() - 1.0) < 1e-6
    assert peak[2] == np.float32(1.0) and scale[2] == np.float32(1.0) and wave[2][W - 1] == 1.0 and not wave[2][:W - 1].any()
    assert (699 + W - 1) // 700 >= (3 if W > 2048 else 1) and (2 + W - 1) // 3 >= 3        # the backgrounds wrap
    assert not wave[1].any() and peak[1] == 0 and scale[1] == 1 and wave[6].any() and n_on[6] == 0
    # clip 0: nested pair of class 1 is one target with collapse, two without; clip 8: four targets in onset order
    assert targets[0][0].tolist() == [1, 2, 3] and offc[3][0][0].tolist() == [1, 1, 2, 3]
    assert targets[8][0].tolist() == [3, 2, 1, 0] and targets[7][0].tolist() == [9, 9] and targets[4][0].tolist() == [6, 7]
    assert targets[3][0].tolist() == ([5, 4] if W == 4096 else [4]) and offc[3][3][0].tolist() == ([5, 5, 4, 4] if W == 4096 else [4, 4])
    assert np.array_equal(targets[3][1][-1], np.asarray([(W - 300) / W, 600 / W], np.float32))       # touching pair merged; cut at the window
    # the shapes asked for
    onsets, fades = set(ev['onset'].tolist()), set(ev['fade'].tolist())
    assert {0, 1, 2, 3, 2047, 2048} <= onsets and {0, 160} <= fades and 1 in set(ev['n'].tolist())
    assert any(e['fade'] > e['n'] / 2 > 0 for e in ev) and any(e['onset'] + e['n'] == W for e in ev) and any(e['onset'] + e['n'] > W for e in ev)
    assert set(ev['src'].tolist()) == {0, 1, 2, 3, 4} and any(g is not None and g[:2] == (5, 699) for g, _ in chosen)
    # capacity at max_targets = 3: exactly three survivors in clip 0 (status 0), four in clip 8 (status 1, the first three written)
    _, _, _, t3, s3 = S.soundscape(sources, bg, ev, off, W, K.SR, 3, 0.0, True, 1.0)
    assert n_on[0] == 3 and n_on[8] == 4 and s3[0] == 0 and s3[8] == 1 and t3[8][0].tolist() == [3, 2, 1]
    assert s3.tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1]
    # the later call with fewer events
    assert sum(len(chosen[i][1]) for i in K.QUIET) < len(ev) / 3
    # bad records: every clip status 2, its good event the only target, and the wave that of the good event alone
    bad = K.bad_clips(W)
    b_bg, b_ev, b_off = K.records(bad)
    b_wave, _, _, b_t, b_s = S.soundscape(sources, b_bg, b_ev, b_off, W, K.SR, 63, 0.0, True, 1.0)
    g_bg, g_ev, g_off = K.records([(None, [(2, 9, 0, 50, 5, 0.5, 0)])])
    alone = S.soundscape(sources, g_bg, g_ev, g_off, W, K.SR, 63, 0.0, True, 1.0)
    assert (b_s == 2).all() and len(bad) == 11
    for b in range(len(bad)):
        assert b_t[b][0].tolist() == [9] and np.array_equal(b_wave[b], alone[0][0]) and np.array_equal(b_t[b][1], alone[3][0][1])


def test_reference_mix_rounds_every_operation_on_its_own():
    """one sample by hand in float32: the background product, then per event (g * w) * x added in plan order"""
    sounds, _, backgrounds = K.bank()
    sources = sounds + backgrounds
    W = 1003
    bg, ev, off = K.records(K.pick(W, 1))
    wave, peak, scale, _, _ = S.soundscape(sources, bg, ev, off, W, K.SR, 63)
    f = np.float32
    for t in (0, 1, 2, 3, 5, 40, 52, 159, 160, 400, 699, 700, 900, 1002):
        acc = f(0.5) * sources[5][(699 + t) % 700]
        for e in ev:
            i = t - int(e['onset'])
            if 0 <= i < min(int(e['n']), W - int(e['onset'])):
                n, fade = int(e['n']), int(e['fade'])
                w_in = f(np.float64(i + 1) / np.float64(fade + 1)) if i < fade else f(1)
                w_out = f(np.float64(n - i) / np.float64(fade + 1)) if n - 1 - i < fade else f(1)
                acc = f(acc + f(f(e['gain'] * min(w_in, w_out)) * sources[e['src']][int(e['src_start']) + i]))
        assert wave[0][t] == acc and scale[0] == 1, t
    assert peak[0] == np.abs(wave[0]).max()
    assert S.fade_weight(np.arange(50), 50, 40).tolist() == [f(min(i + 1, 50 - i) / 41.0) for i in range(50)]       # the ramps overlap
