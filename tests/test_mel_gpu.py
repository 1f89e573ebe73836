"""GPU: the mel front end (sedt_mel_spectrogram, utilities/mel.py) against the float64 restatement tests/mel_ref.py, for both of the
reference's configurations (URBAN-SED 44100 / 2048 / 1764 / 882, DCASE 16000 / 1024 / 1024 / 323), at the smallest shapes where the
kernel can go wrong: clips of the minimum length, of 3 hop - 1, 3 hop, 3 hop + 1 samples (the frame count steps at 3 hop; a workgroup
owns 4 frames, so these clips end inside one) and of sr + 37 samples (13 workgroups, the last one partly filled).

The bound: per frame, max over the bands of |got - ref| <= 2e-6 of the frame's largest band.  Its yardstick is the reference pipeline
run in f32 on the CPU (tests/test_mel_cpu.py prints it: 3.0e-7 URBAN, 2.0e-7 DCASE on the fixture clip); the device gets about 8x
that for another butterfly order and the rounded twiddle table.  Every comparison prints its figure before it asserts.

Measured on an MI355X (worst frame, as a fraction of the frame maximum): ragged batch 4.7e-7 URBAN / 2.6e-7 DCASE, fixture G21
4.6e-7 / 2.0e-7, pure tones and DC at most 4.3e-7, replayed graph 2.3e-7; dB features through DeviceBoxTransform at most 1.5e-5 dB from
the oracle (bound 0.02 dB).  DESIGN.md, "Mel front end", has the table."""
import functools
import os

import numpy as np
import pytest
import torch

import mel_ref as R

pytestmark = pytest.mark.gpu

CFGS = sorted(R.CONFIGS)
BOUND = 2e-6


@functools.lru_cache(maxsize=None)
def _mel(name):
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    return DeviceMelSpectrogram.urbansed() if name == 'urban' else DeviceMelSpectrogram.dcase()


def _lengths(cfg):
    return [cfg['n_fft'] // 2 + 1, 3 * cfg['hop'] - 1, 3 * cfg['hop'], 3 * cfg['hop'] + 1, cfg['sr'] + 37]


@functools.lru_cache(maxsize=None)
def _ragged(name):
    """the ragged batch of the framing test, its float64 references (computed once) and the device result as it came back"""
    cfg = R.CONFIGS[name]
    waves = [R.fixture_signal(300 + i, cfg['sr'], n) for i, n in enumerate(_lengths(cfg))]
    refs = [R.mel_spectrogram(y, **cfg) for y in waves]
    mel, nframes = _mel(name)(waves)
    torch.cuda.synchronize()
    return waves, refs, mel.cpu().numpy(), list(nframes)


def _frame_error(got, ref):
    """per frame: max over the bands of |got - ref| / max over the bands of ref"""
    return np.abs(got.astype(np.float64) - ref).max(axis=1) / ref.max(axis=1)


def _check(what, got, ref):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    err = _frame_error(got, ref)
    print(f'{what}: worst frame {int(err.argmax())} of {len(err)}: {err.max():.3e} of its maximum (bound {BOUND:.0e})')
    assert np.isfinite(got).all() and err.max() <= BOUND, what


@pytest.mark.parametrize('name', CFGS)
def test_framing_edges_of_a_ragged_batch(name):
    from sound_event_detection_transformer_amd.utilities.mel import frames_of
    cfg = R.CONFIGS[name]
    waves, refs, got, nframes = _ragged(name)
    assert nframes == [frames_of(len(y), cfg['hop']) for y in waves] == [len(r) for r in refs]
    assert nframes[0] == 2 and nframes[1:4] == [3, 4, 4]
    assert got.shape == (len(waves), max(nframes), cfg['n_mels'])
    for i, ref in enumerate(refs):
        _check(f'{name} clip {i} ({len(waves[i])} samples, {nframes[i]} frames)', got[i, :nframes[i]], ref)
        assert (got[i, nframes[i]:] == 0).all() and not np.signbit(got[i, nframes[i]:]).any(), 'rows past the clip are exactly 0'


@pytest.mark.parametrize('name', CFGS)
def test_fixture_g21_accuracy(name, golden_dir):
    g = np.load(os.path.join(golden_dir, 'g21_mel.npz'))
    cfg = R.CONFIGS[name]
    y = R.fixture_signal(int(g[f'{name}_seed']), cfg['sr'], int(g[f'{name}_n']))
    feats = _mel(name).features([y])
    assert len(feats) == 1
    _check(f'{name} fixture clip', feats[0], g[f'{name}_mel'])


@pytest.mark.parametrize('name', CFGS)
def test_bin_indexing_with_pure_tones_and_dc(name):
    """tones at the centres of bins 1, 2 and n_fft/2 - 1, and a constant: the brightest band of every frame is the one the reference
    names, and the frame is within the bound.  Bin 0 feeds no band, so the constant clip's band energies are window leakage alone."""
    cfg = R.CONFIGS[name]
    N, n = cfg['n_fft'], 4 * cfg['hop'] + 11
    waves = [R.pure_tone(n, N, k) for k in (1, 2, N // 2 - 1)] + [np.full(n, 0.5, np.float32)]
    feats = _mel(name).features(waves)
    for what, y, got in zip(('bin 1', 'bin 2', f'bin {N // 2 - 1}', 'DC'), waves, feats):
        ref = R.mel_spectrogram(y, **cfg)
        _check(f'{name} {what}', got, ref)
        assert (got.argmax(axis=1) == ref.argmax(axis=1)).all(), (what, got.argmax(axis=1), ref.argmax(axis=1))
    W = R.mel_filterbank(cfg['sr'], N, cfg['n_mels'])
    assert (W[:, 0] == 0).all() and feats[3].max() > 0                      # leakage only - and the reference agrees it is not zero
    assert feats[2].argmax(axis=1).min() >= cfg['n_mels'] - 2 and feats[0].argmax(axis=1).max() <= 1


@pytest.mark.parametrize('name', CFGS)
def test_silence_gives_exact_zeros(name):
    cfg = R.CONFIGS[name]
    mel, nframes = _mel(name)([np.zeros(3 * cfg['hop'] + 1, np.float32), np.zeros(cfg['n_fft'], np.int16)])
    got = mel.cpu().numpy()
    assert nframes == [4, 1 + cfg['n_fft'] // cfg['hop']] and np.isfinite(got).all() and (got == 0).all() and not np.signbit(got).any()


@pytest.mark.parametrize('name', CFGS)
def test_int16_batch_equals_the_f32_batch_bit_for_bit(name):
    cfg = R.CONFIGS[name]
    rng = np.random.RandomState(7)
    pcm = [rng.randint(-32768, 32768, n).astype(np.int16) for n in (cfg['n_fft'] // 2 + 1, 3 * cfg['hop'] + 1, 6 * cfg['hop'] - 1)]
    pcm[1][:5] = [-32768, 32767, 0, 1, -1]
    a, na = _mel(name)(pcm)
    b, nb = _mel(name)([(x.astype(np.float32) / np.float32(32768.0)) for x in pcm])
    assert na == nb and a.dtype == b.dtype == torch.float32 and torch.equal(a, b) and float(a.max()) > 0
    # ... and as a (B, N) block already on the device
    blk = torch.from_numpy(np.stack([x[:cfg['n_fft'] // 2 + 1] for x in pcm])).cuda()
    c, nc = _mel(name)(blk)
    assert nc == [na[0]] * 3 and torch.equal(c[0], a[0, :nc[0]])


@pytest.mark.parametrize('name', CFGS)
def test_bits_do_not_depend_on_the_batch(name):
    waves, refs, got, nframes = _ragged(name)
    again, n2 = _mel(name)(waves)
    assert n2 == nframes and np.array_equal(again.cpu().numpy(), got), 'two runs of one batch'
    for i, y in enumerate(waves):
        alone, n1 = _mel(name)([y])
        assert n1 == [nframes[i]] and alone.shape == (1, nframes[i], 64)
        assert np.array_equal(alone[0].cpu().numpy(), got[i, :nframes[i]]), f'clip {i} alone (B = 1) against its rows in the batch'
    # another order and another row stride: still the same bits
    out = torch.full((len(waves), max(nframes) + 3, 64), float('nan'), device='cuda')
    rev, n3 = _mel(name)(waves[::-1], out=out)
    assert rev is out and n3 == nframes[::-1]
    rev = rev.cpu().numpy()
    for i in range(len(waves)):
        j = len(waves) - 1 - i
        assert np.array_equal(rev[j, :nframes[i]], got[i, :nframes[i]]) and (rev[j, nframes[i]:] == 0).all()


@pytest.mark.parametrize('name', CFGS)
def test_captured_call_replays_on_new_input(name):
    cfg = R.CONFIGS[name]
    B, n = 3, 5 * cfg['hop'] + 2
    first = torch.from_numpy(np.stack([R.fixture_signal(500 + i, cfg['sr'], n) for i in range(B)])).cuda()
    second = torch.from_numpy(np.stack([R.fixture_signal(600 + i, cfg['sr'], n) for i in range(B)])).cuda()
    buf, mel = first.clone(), _mel(name)
    out = torch.empty((B, 6, 64), device='cuda')
    mel(buf, out=out)                                                        # warm-up: everything the call allocates exists
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, nframes = mel(buf, out=out)
    assert nframes == [6] * B
    buf.copy_(second)
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    eager, _ = mel(second)
    assert torch.equal(out, eager) and not torch.equal(eager, mel(first)[0])
    _check(f'{name} replayed clip 0', out[0].cpu().numpy(), R.mel_spectrogram(second[0].cpu().numpy(), **cfg))


def test_refusals_launch_nothing():
    from sound_event_detection_transformer_amd import lib
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    l = lib.load()
    assert l.sedt_mel_ok(2048, 1764, 882, 64) == 1 and l.sedt_mel_ok(1024, 1024, 323, 64) == 1 and l.sedt_mel_ok(512, 400, 160, 128) == 1
    assert l.sedt_mel_ok(1536, 1024, 323, 64) == 0 and l.sedt_mel_ok(1024, 1025, 323, 64) == 0 and l.sedt_mel_ok(1024, 1024, 0, 64) == 0
    assert l.sedt_mel_ok(4096, 1024, 323, 64) == 0 and l.sedt_mel_ok(1024, 1024, 323, 129) == 0
    mel = _mel('dcase')
    with lib.launch_log() as log:
        with pytest.raises(RuntimeError, match=r'mel_spectrogram: n_fft=1536 .*outside the envelope'):
            DeviceMelSpectrogram(16000, 1536, 1024, 323)
        with pytest.raises(RuntimeError, match=r'mel_spectrogram: n_fft=1024 n_window=1025 .*outside the envelope'):
            DeviceMelSpectrogram(16000, 1024, 1025, 323)
        with pytest.raises(ValueError, match=r'mel_spectrogram: a clip of 512 samples is shorter than n_fft/2 \+ 1 = 513'):
            mel([np.ones(2000, np.float32), np.ones(512, np.float32)])
        with pytest.raises(ValueError, match='shorter than'):
            mel(torch.ones((2, 2000), device='cuda'), lengths=[2000, 100])
        assert log['mel_spectrogram'] == 0
        mel([np.ones(513, np.float32)])
        assert log['mel_spectrogram'] == 1
    # the entry point itself: a dtype code it does not know, null pointers
    t = torch.zeros(8, device='cuda')
    assert l.sedt_mel_spectrogram(lib.p(t), 1, 8, lib.p(t), 1, lib.p(t), 1, lib.p(t), lib.p(t), lib.p(t), lib.p(t), lib.p(t), 0, 1024, 1024,
                                  323, 64, None) != 0
    assert b'wave_dtype' in l.sedt_last_error()
    assert l.sedt_mel_spectrogram(None, 0, 8, lib.p(t), 1, lib.p(t), 1, lib.p(t), lib.p(t), lib.p(t), lib.p(t), lib.p(t), 0, 1024, 1024,
                                  323, 64, None) != 0
    assert b'null pointer' in l.sedt_last_error()


@pytest.mark.parametrize('name', CFGS)
def test_handoff_to_the_transform_and_the_scaler(name, golden_dir):
    """mel and nframes go straight into DeviceBoxTransform(frames, apply_log=True) - no scaler, no augmentation - and the dB features
    are those the transforms oracle makes of the float64 reference mel.  Bound, derived: a mel error of 2e-6 of the frame maximum on a
    band no smaller than 1.6e-3 of it is a relative error of 1.25e-3, i.e. 20 log10(e) * 1.25e-3 = 0.011 dB; 0.02 dB allowed (the
    f32 log10 of the transform kernel adds ~1e-5 dB).  The band floor is asserted on the reference, clip by clip."""
    from oracle import transforms_oracle as T
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    g = np.load(os.path.join(golden_dir, 'g21_mel.npz'))
    cfg = R.CONFIGS[name]
    waves = [R.fixture_signal(int(g[f'{name}_seed']), cfg['sr'], int(g[f'{name}_n'])), R.fixture_signal(42, cfg['sr'], cfg['sr'] // 2)]
    refs = [g[f'{name}_mel'], R.mel_spectrogram(waves[1], **cfg)]
    for r in refs:
        assert (r.min(axis=1) / r.max(axis=1)).min() >= 1.6e-3, 'the derivation of the bound needs this noise floor'
    frames = 40                                      # the first clip (50 / 51 frames) is truncated, the second padded
    assert len(refs[1]) < frames < len(refs[0])
    mel, nframes = _mel(name)(waves)
    x = DeviceBoxTransform(frames, apply_log=True)(mel, nframes=nframes)
    assert x.shape == (2, 1, frames, 64)
    x = x.cpu().numpy()
    for i, r in enumerate(refs):
        want = T.box_transform(r, frames, 0.0, 1.0)
        d = np.abs(x[i].astype(np.float64) - want).max()
        print(f'{name} clip {i}: dB features, max |diff| {d:.2e} dB (bound 0.02)')
        assert d <= 0.02
    sc = Scaler(frames).update(mel, nframes=nframes).finalize()
    assert sc.count_ == 2 and np.isfinite(sc.mean_).all()
    want_mean = x[:, 0].astype(np.float64).mean(axis=1).mean(axis=0)
    assert np.abs(sc.mean_ - want_mean).max() <= 1e-9 * np.abs(want_mean).max()
