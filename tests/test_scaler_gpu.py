"""GPU: the dataset Scaler fitted on the device (sedt_scaler_update, utilities/scaler.py) against fixture G20 - what the REFERENCE's
own Scaler computed over clips that passed through its own PadOrTrunc and ToTensor - and, for the ApplyLog path, against the output of
the project's transform kernel, whose features the fit has to describe.

The tolerances on the statistics are derived, not tuned (tests/scaler_ref.py: summation_bounds): two correct float64 summations of
the same terms differ by at most 2 (n - 1) 2^-53 sum|x_i|, n = rows per clip + clips, times FACTOR = 2 for the two divisions and the
second-order terms.  Every comparison prints its worst diff / bound ratio before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import scaler_ref as R

pytestmark = pytest.mark.gpu


def _g20(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g20_scaler.npz'))
    return g, [g[f'in{i}'] for i in range(len(g['nraw']))], int(g['frames'])


def _within(name, got, want, bound):
    d = np.abs(got - want)
    print(f'{name}: max |diff| {d.max():.3e}, worst diff / bound {(d / np.maximum(bound, 1e-300)).max():.3f}')
    assert np.isfinite(got).all() and (d <= bound).all(), name


def test_g20_parity_with_the_reference_scaler(golden_dir):
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    g, clips, frames = _g20(golden_dir)
    sc = Scaler(frames, apply_log=False)
    mean, std = sc.calculate_scaler([clips])
    assert mean is sc.mean_ and std is sc.std_ and sc.count_ == len(clips)
    assert all(a.dtype == np.float64 and a.shape == (64,) for a in (sc.mean_, sc.mean_of_square_, sc.std_))
    b1, b2 = R.summation_bounds([R.features(c, frames, False) for c in clips], frames)
    _within('mean_', sc.mean_, g['mean_'], b1)
    _within('mean_of_square_', sc.mean_of_square_, g['mean_of_square_'], b2)
    assert np.array_equal(sc.std_, np.sqrt(sc.mean_of_square_ - sc.mean_ ** 2))
    zb, cb = int(g['zero_band']), int(g['const_band'])
    assert sc.std_[zb] == 0.0 == g['std_'][zb]                                   # variance exactly 0
    assert sc.mean_[cb] == g['mean_'][cb] and sc.mean_of_square_[cb] == g['mean_of_square_'][cb] and sc.std_[cb] == g['std_'][cb]
    # the same data set as (clips, targets) pairs, one clip per batch: what a driver's loader yields
    sc2 = Scaler(frames, apply_log=False)
    sc2.calculate_scaler(([c], [{'labels': None}]) for c in clips)
    assert np.array_equal(sc2.sum_, sc.sum_) and sc2.count_ == sc.count_
    # ... and the JSON it writes is the reference's format
    assert set(sc.state_dict()) == set(json.loads(str(g['json'])))


@pytest.mark.parametrize('frames', [496, 500])
def test_fit_describes_what_the_transform_kernel_produces(frames):
    """apply_log=True at the bench geometries (B = 64 clips, 64 mel bands): the reference statistics are float64 means of the output of
    DeviceBoxTransform(frames, apply_log=True) - no augmentation, no scaler - and of its f32 squares"""
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    rng = np.random.RandomState(frames)
    B = 64
    nraw = [int(n) for n in rng.randint(frames - 90, frames + 60, B)]
    nraw[0], nraw[1], nraw[2] = frames, frames - 90, frames + 59
    assert min(nraw) < frames < max(nraw)
    clips = [np.abs(rng.randn(n, 64)).astype(np.float32) * np.float32(10 ** rng.uniform(-3, 1)) for n in nraw]
    clips[3][:40] = 0.0                                                          # silence: amin and the 80 dB floor
    clips[2][frames:] *= 1e3                                                     # the clip maximum sits in rows PadOrTrunc cuts off
    out = DeviceBoxTransform(frames, apply_log=True)(clips)
    v = out[:, 0].cpu().numpy()
    assert v.shape == (B, frames, 64) and v.dtype == np.float32
    want_mean = v.astype(np.float64).mean(axis=1).mean(axis=0)
    want_mos = (v * v).astype(np.float32).astype(np.float64).mean(axis=1).mean(axis=0)
    b1, b2 = R.summation_bounds(list(v), frames)
    sc = Scaler(frames, apply_log=True)
    sc.calculate_scaler([clips])
    assert sc.count_ == B
    _within(f'{frames} x 64 mean_', sc.mean_, want_mean, b1)
    _within(f'{frames} x 64 mean_of_square_', sc.mean_of_square_, want_mos, b2)
    assert (sc.std_ > 0).all()


def _sums(sc):
    sc.finalize()
    return sc.sum_.copy(), sc.count_


@pytest.mark.parametrize('apply_log', [False, True])
def test_streaming_is_bit_identical_however_the_clips_are_cut(apply_log):
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    rng = np.random.RandomState(11)
    frames, F = 100, 64                                                          # 100: the divisions round
    nraw = [100, 87, 131, 60, 100, 117, 93, 140, 75, 102, 99, 128]
    clips = [np.abs(rng.randn(n, F)).astype(np.float32) * np.float32(10 ** rng.uniform(-2, 1)) + np.float32(1e-3) for n in nraw]
    if not apply_log:
        clips = [np.float32(10) * np.log10(c) for c in clips]
    one = Scaler(frames, apply_log=apply_log).update(clips)
    ref, count = _sums(one)
    assert count == len(clips) and np.isfinite(ref).all() and (ref[1] > 0).all()
    again, _ = _sums(Scaler(frames, apply_log=apply_log).update(clips))
    assert np.array_equal(again, ref)                                            # two runs
    cut = Scaler(frames, apply_log=apply_log)
    for lo, hi in ((0, 5), (5, 6), (6, 12)):
        cut.update(clips[lo:hi])
    got, n = _sums(cut)
    assert n == count and np.array_equal(got, ref)                               # several batches
    # device-resident: one (B, stride, F) tensor, rows beyond each clip's length filled with values that would show if read
    stride = max(nraw)
    block = np.full((len(clips), stride, F), 1e4, np.float32)
    for i, c in enumerate(clips):
        block[i, :len(c)] = c
    got, n = _sums(Scaler(frames, apply_log=apply_log).update(torch.from_numpy(block).cuda(), nframes=nraw))
    assert n == count and np.array_equal(got, ref)
    # ... and without nframes every clip is `stride` rows long: equal to the list of those full-length clips
    full, _ = _sums(Scaler(frames, apply_log=apply_log).update(torch.from_numpy(block).cuda()))
    lst, _ = _sums(Scaler(frames, apply_log=apply_log).update(list(block)))
    assert np.array_equal(full, lst) and not np.array_equal(full, ref)
    # the order of the clips is the order of the sum: the restatement in that order agrees to the bound, and reproduces the bits
    # wherever the features are the same f32 numbers (apply_log=False)
    if not apply_log:
        sums, _ = R.fit(clips, frames, False)
        assert np.array_equal(sums, ref)
    # means() starts a fresh fit
    one.means([clips[:4]])
    assert one.count_ == 4


def test_fitted_scaler_feeds_the_transform_end_to_end(golden_dir):
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform, DeviceViewTransform
    g, clips, frames = _g20(golden_dir)
    sc = Scaler(frames, apply_log=False)
    sc.calculate_scaler([clips[:3], clips[3:]])
    two = [clips[i] for i in g['normalized']]
    want = np.stack([g[f'norm{i}'] for i in g['normalized']])
    out = DeviceBoxTransform(frames, scaler=sc, apply_log=False)(two).cpu().numpy()
    assert out.shape == want.shape == (2, 1, frames, 64)
    assert np.isnan(want[..., int(g['zero_band'])]).all()                         # 0 / 0 in the band of zeros, on both sides
    np.testing.assert_allclose(out, want, rtol=2e-6, atol=2e-5)                   # the tolerance of the G13 test (test_input_gpu.py)
    same = DeviceBoxTransform(frames, sc.mean_, sc.std_, apply_log=False)(two).cpu().numpy()
    assert np.array_equal(out, same, equal_nan=True)                              # scaler= is the two vectors, nothing else
    x0, x1 = DeviceViewTransform(frames, scaler=sc, apply_log=False, noise_p=0.0)(two)
    assert np.array_equal(x0.cpu().numpy(), out, equal_nan=True) and np.array_equal(x1.cpu().numpy(), out, equal_nan=True)


def test_one_launch_per_batch_and_the_lds_limit(golden_dir):
    from sound_event_detection_transformer_amd import lib
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    g, clips, frames = _g20(golden_dir)
    sc = Scaler(frames, apply_log=False)
    with lib.launch_log() as log:
        sc.update(clips[:3]).update(clips[3:4]).update(clips[4:])
        sc.finalize()
    assert dict(log) == {'sedt_scaler_update': 3}                                 # nothing else went through the C ABI
    assert np.array_equal(sc.mean_, Scaler(frames, apply_log=False).calculate_scaler([clips])[0])
    with pytest.raises(RuntimeError, match='LDS'):                                # 700 x 64 f32 + partials > 160 KB: an error, no launch
        Scaler(700).update([np.ones((10, 64), np.float32)])
    with pytest.raises(ValueError):
        Scaler(frames).update([np.ones((10, 32), np.float32)])                    # 32 bands into a 64-band scaler
