"""GPU: sedt_loudness and sedt_scale_sources (csrc/loudness.hip) through the ctypes ABI against tests/loudness_ref.py, the public stage
utilities.loudness.DeviceLoudness, and the level='lufs' mode of SoundscapeClips.

Cases (tests/loudness_cases.py; tests/test_loudness_cpu.py checks on the reference alone that no block lies within 1e-6 of a gate
threshold): 16, 22.05 and 48 kHz (H = 1600, 2205, 4800); sources of 1, H - 1, 4H - 1, 4H, 4H + 1, 5H - 1, 5H and 23H + 7 samples, at 16 kHz
also 259H + 3 and 260H (a second round of hops); 1, 3 and 70 sources back to back; stepped noise, noise, zeros, noise under the absolute
gate, noise on a DC offset.

zbar is held to 1e-10 relative of the float64 reference: a hop's sum of at most 4800 squares errs by at most 4800 2^-53 = 5e-13, and the
filter's rounding, amplified by 1 / (1 - r) = 200 at the high-pass pole (r = 0.995 at 48 kHz), is of order 1e-13; the bound leaves two
orders.  Counts are exact.  After a normalisation to -23 LUFS the sources sit within 1e-4 LU of it (the float32 gain and the float32
products bound the error near 1e-6 LU)."""
import math

import numpy as np
import pytest
import torch

import loudness_cases as K
import loudness_ref as R
import soundscape_ref as S

pytestmark = pytest.mark.gpu

SR = 16000
LABELS = [f'c{i}' for i in range(10)]


def _stage(sources):
    """(flat on the device, offsets, lengths) of sources laid back to back"""
    lens = np.asarray([len(x) for x in sources], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return torch.from_numpy(np.concatenate(sources)).cuda(), off, lens


def _call(flat, off, lens, sr, work_len=None, fill=-7.0):
    """one sedt_loudness call through the ABI: (zbar, counts, work) as host arrays; the outputs are pre-filled with `fill`"""
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities import loudness as M
    H = M.hop_samples(sr)
    words = M.work_doubles(lens, H)
    assert words == int(sum(n // H + 1 for n in lens.tolist()))
    work_len = words if work_len is None else work_len
    consts = torch.from_numpy(np.concatenate([M.k_weighting(sr), M.hop_map(sr).reshape(-1)])).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    work = torch.full((words + 8,), fill, dtype=torch.float64, device='cuda')
    zbar = torch.full((len(lens),), fill, dtype=torch.float64, device='cuda')
    counts = torch.full((len(lens), 4), -9, dtype=torch.int32, device='cuda')
    L.check(L.load().sedt_loudness(L.p(flat), flat.numel(), L.p(d_off), L.p(d_len), len(lens), L.p(consts), L.p(consts[10:]), H, M.Z_ABS,
                                   L.p(work), work_len, L.p(zbar), L.p(counts), L.stream_ptr()), 'loudness')
    return zbar.cpu().numpy(), counts.cpu().numpy(), work.cpu().numpy()


def _compare(zbar, counts, ref, who):
    worst = 0.0
    for i, m in enumerate(ref):
        assert counts[i].tolist() == [m['J'], m['n_abs'], m['n_rel'], int(m['short'])], (who, i, counts[i], m['J'], m['n_abs'], m['n_rel'])
        if m['zbar'] == 0.0:
            assert zbar[i] == 0.0, (who, i, zbar[i])
        else:
            worst = max(worst, abs(zbar[i] - m['zbar']) / m['zbar'])
    print(f'{who}: worst relative error of zbar {worst:.3e}')
    assert worst < 1e-10, (who, worst)


@pytest.mark.parametrize('sr,n_src', K.CASES)
def test_loudness_against_the_float64_reference(sr, n_src):
    sources, ref = K.sources(sr, n_src), K.reference(sr, n_src)
    flat, off, lens = _stage(sources)
    zbar, counts, work = _call(flat, off, lens, sr)
    _compare(zbar, counts, ref, (sr, n_src))
    words = len(work) - 8
    assert (work[words:] == -7.0).all()                            # nothing behind the workspace is written
    # the hop energies themselves: source 0's against the serial filter
    H = R.hop_samples(sr)
    y = R.k_filter(sources[0], sr)
    e = np.asarray([np.sum(y[h * H:(h + 1) * H] ** 2) for h in range(len(y) // H)])
    if len(e) and e.min() > 0:
        assert np.abs(work[:len(e)] - e).max() <= 1e-11 * e.max()
    # two calls into the same kind of buffers: the same bits
    zbar2, counts2, work2 = _call(flat, off, lens, sr)
    assert zbar.tobytes() == zbar2.tobytes() and counts.tobytes() == counts2.tobytes() and work.tobytes() == work2.tobytes()


def test_workspace_one_short_is_refused():
    """the lengths live on the device and the call does not synchronise: the entry point refuses what it can see (fewer words than
    sources), the launch refuses the source whose hop energies would not fit - NaN, counts -1, nothing written - and the stage raises"""
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities import loudness as M
    sources, ref = K.sources(SR, 3), K.reference(SR, 3)
    flat, off, lens = _stage(sources)
    words = M.work_doubles(lens, 1600)
    zbar, counts, work = _call(flat, off, lens, SR, work_len=words - 1)
    assert math.isnan(zbar[2]) and counts[2].tolist() == [-1] * 4
    _compare(zbar[:2], counts[:2], ref[:2], 'one short')
    last = words - (int(lens[2]) // 1600 + 1)
    assert (work[last:] == -7.0).all() and (work[:last] != -7.0).all()
    with pytest.raises(RuntimeError, match='the workspace does not hold the hop energies of source 2'):
        M.DeviceLoudness.result(torch.from_numpy(zbar), torch.from_numpy(counts))
    with pytest.raises(RuntimeError, match='work_len=2 is too small'):
        d = torch.zeros(64, dtype=torch.float64, device='cuda')
        L.check(L.load().sedt_loudness(L.p(flat), flat.numel(), L.p(d), L.p(d), 3, L.p(d), L.p(d), 1600, M.Z_ABS, L.p(d), 2, L.p(d), L.p(d),
                                       L.stream_ptr()), 'loudness')


def test_device_loudness_measures_and_refuses():
    from sound_event_detection_transformer_amd.utilities.loudness import DeviceLoudness
    sources, ref = K.sources(22050, 3), K.reference(22050, 3)
    loud = DeviceLoudness(22050)
    res = loud.measure_waves(list(sources))
    assert res.lufs.dtype == np.float64 and res.short.tolist() == [m['short'] for m in ref]
    assert res.blocks.tolist() == [m['J'] for m in ref] and res.n_abs.tolist() == [m['n_abs'] for m in ref]
    assert res.n_rel.tolist() == [m['n_rel'] for m in ref]
    assert all(abs(a - m['lufs']) < 1e-9 for a, m in zip(res.lufs, ref))
    flat, off, lens = _stage(sources)
    again = loud.measure(flat, off, lens)
    assert again.zbar.tobytes() == res.zbar.tobytes()
    pcm = (np.clip(sources[1], -1, 1) * 32767).astype(np.int16)                             # 16-bit PCM is widened as the mel stage widens it
    got = loud.measure_waves([pcm, np.zeros(3000, np.float32)])
    assert abs(got.lufs[0] - R.measure(pcm.astype(np.float32) * np.float32(1.0 / 32768.0), 22050)['lufs']) < 1e-9
    assert got.lufs[1] == -np.inf and got.zbar[1] == 0.0 and got.short[1]
    for bad in (np.nan, np.inf):
        x = sources[1].copy()
        x[len(x) // 2] = bad
        with pytest.raises(ValueError, match='source 1 holds non-finite samples'):
            loud.measure_waves([sources[1], x])
    with pytest.raises(ValueError, match='does not lie inside'):
        loud.measure(flat, off, lens + 1)


def test_normalize_to_minus_23_lufs():
    from sound_event_detection_transformer_amd.utilities.loudness import DeviceLoudness
    gen = np.random.default_rng(41)
    H = 1600
    loud_spiky = 0.02 * gen.standard_normal(9 * H + 5)
    loud_spiky[777] = 0.9                                          # a peak the target gain would push past the limit
    sources = [(0.1 * gen.standard_normal(23 * H + 7)).astype(np.float32), (0.003 * gen.standard_normal(4 * H - 1)).astype(np.float32),
               loud_spiky.astype(np.float32), (1e-5 * gen.standard_normal(6 * H + 3)).astype(np.float32),
               K.content('steps', 30 * H + 1, gen), np.zeros(5, np.float32)]
    flat, off, lens = _stage(sources)
    loud = DeviceLoudness(SR)
    out = loud.normalize(flat, off, lens, -23.0, peak_limit=1.0)
    assert out.silent.tolist() == [False, False, False, True, False, True] and out.limited.tolist() == [False, False, True, False, False, False]
    assert out.gains.dtype == np.float32 and out.gains[3] == 1.0 and out.gains[5] == 1.0
    after, host = loud.measure(flat, off, lens), flat.cpu().numpy()
    for i in (0, 1, 4):
        want = np.float32(10.0 ** ((-23.0 - out.before.lufs[i]) / 20.0))
        assert out.gains[i] == want and abs(after.lufs[i] + 23.0) < 1e-4, (i, after.lufs[i])
        assert np.array_equal(host[off[i]:off[i] + lens[i]], sources[i] * out.gains[i])    # one float32 product per sample
    peak = np.abs(sources[2]).max()
    new = host[off[2]:off[2] + lens[2]]
    assert np.abs(new).max() == np.float32(peak * out.gains[2]) <= np.float32(1.0) and np.array_equal(new, sources[2] * out.gains[2])
    assert out.gains[2] < 10.0 ** ((-23.0 - out.before.lufs[2]) / 20.0) and after.lufs[2] < -23.0 - 1e-3
    for i in (3, 5):                                                # -inf: untouched, bit for bit
        assert host[off[i]:off[i] + lens[i]].tobytes() == sources[i].tobytes()
    assert after.lufs[3] == -np.inf and out.before.lufs[3] == -np.inf


@pytest.fixture(scope='module')
def bank():
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    gen = np.random.default_rng(19)
    t = np.arange(3 * SR) / SR
    rumble = 0.2 * np.sin(2 * np.pi * 55.0 * t) + 0.01 * gen.standard_normal(3 * SR)       # energy where the high-pass acts
    barks = np.zeros(2 * SR)
    barks[2000:6000] = 0.3 * gen.standard_normal(4000)                                     # pauses: the gates drop them
    sounds = [rumble.astype(np.float32), barks.astype(np.float32), (0.1 * gen.standard_normal(SR // 2 + 3)).astype(np.float32),
              (0.05 * gen.standard_normal(777)).astype(np.float32)]
    backgrounds = [(0.02 * gen.standard_normal(2 * SR)).astype(np.float32), np.zeros(900, np.float32),
                   (1e-5 * gen.standard_normal(SR)).astype(np.float32)]
    return dict(sounds=sounds, classes=[1, 4, 4, 7], backgrounds=backgrounds, mel=DeviceMelSpectrogram.dcase())


def _scapes(bank, level, window=2 * SR, **kw):
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    s = SoundscapeClips(bank['mel'], LABELS, window / SR, level=level, **kw)
    return s.add_events(bank['sounds'], bank['classes']).add_backgrounds(bank['backgrounds'])


def test_soundscape_clips_in_lufs_mode(bank):
    from sound_event_detection_transformer_amd.utilities.loudness import DeviceLoudness
    from sound_event_detection_transformer_amd.utilities.soundscape import gains
    s = _scapes(bank, 'lufs')
    sources = bank['sounds'] + bank['backgrounds']
    # the staged bank's loudness is DeviceLoudness' on the same vector, by its bits
    res = DeviceLoudness(SR).measure(s.flat, s.src_off[:-1], s.ns)
    assert s.lufs.tobytes() == res.lufs.tobytes() and s.lufs.shape == (7,)
    assert np.array_equal(s.level_amp, np.float64(10.0) ** (s.lufs / 20.0)) and s.level_amp[5] == 0.0 == s.level_amp[6]
    assert s.lufs[5] == -np.inf and s.lufs[6] == -np.inf and s.rms[6] > 0                   # a background under the gate is allowed
    assert all(abs(s.lufs[i] - R.measure(sources[i], SR)['lufs']) < 1e-9 for i in range(5))
    # K-weighting and gating move the level: the rumble sits far under its RMS level, the barks over theirs
    rms_db = 20.0 * np.log10(s.rms[:5])
    assert s.lufs[0] < rms_db[0] - 3.0 and s.lufs[1] > rms_db[1] + 3.0
    # an event bank with a source under the absolute gate is refused, and the bank stays as it was
    with pytest.raises(ValueError, match='source 1 lies under the absolute gate'):
        s.add_events([bank['sounds'][2], bank['backgrounds'][2]], ['c1', 'c2'])
    assert len(s) == 7 and s.lufs.shape == (7,)
    # a drawn plan: level_amp stands where the RMS stands; the mixing is unchanged
    np.random.seed(21)
    plan = s.draw(6, n_events=(1, 4), ref_db=-35.0, max_event_seconds=0.6)
    for e in plan.ev:
        assert 0 < float(e['gain']) and np.isfinite(e['gain'])
    np.random.seed(21)
    bg, ev, off = S.draw(6, s.ns, s.level_amp, s.by_class, s.backgrounds, s.window, SR, (1, 4), (6.0, 30.0), -35.0, 0.6, 0.01)
    assert plan.bg.tobytes() == bg.tobytes() and plan.ev.tobytes() == ev.tobytes()
    assert all(g['gain'] == (gains(-35.0, 0.0, s.level_amp[g['src']]) if g['src'] == 4 else 1.0) for g in plan.bg)
    want = S.soundscape(sources, plan.bg, plan.ev, plan.ev_off, s.window, SR, s.max_targets, s.min_event_seconds, s.collapse, s.peak_limit)
    wave, _, dt = s.mix(plan)
    assert np.array_equal(wave.cpu().numpy().view(np.int32), want[0].view(np.int32)) and not dt.status.any().item()


def test_a_background_at_ref_db_measures_ref_db_lufs(bank):
    """the feature end to end: a window-long stationary background from sample 0, no events, ref_db = -30 - the clip measures -30 LUFS
    under level='lufs' and does not under level='rms'"""
    from sound_event_detection_transformer_amd.utilities.loudness import DeviceLoudness
    from sound_event_detection_transformer_amd.utilities.soundscape import gains
    loud = DeviceLoudness(SR)
    got = {}
    for level in ('lufs', 'rms'):
        s = _scapes(bank, level)
        assert s.ns[4] == s.window
        g = gains(-30.0, 0.0, s.level_amp[4] if level == 'lufs' else s.rms[4])
        wave, _, _ = s.mix(s.plan([(4, 0, g)], [[]]))
        assert float(s.last_scale.cpu()[0]) == 1.0                 # the peak limit stays off
        got[level] = float(loud.measure(wave.reshape(-1), [0], [s.window]).lufs[0])
    print('a background at ref_db = -30:', got)
    assert abs(got['lufs'] + 30.0) < 1e-4, got
    assert abs(got['rms'] + 30.0) > 1e-4 and abs(got['rms'] - got['lufs']) > 0.1, got
