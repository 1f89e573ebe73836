"""CPU: the host side of the dataset Scaler (utilities/scaler.py) against fixture G20, which the REFERENCE's own Scaler, PadOrTrunc,
ToTensor and Normalize produced (tests/golden/make_golden_scaler.py): the NumPy restatement of the fit the GPU tests lean on, the JSON
round trip in the reference's format, std_, merge, and the validation of the scaler= argument of the transforms."""
import json
import os

import numpy as np
import pytest

import scaler_ref as R


@pytest.fixture(scope='module')
def g20(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g20_scaler.npz'))
    return g, [g[f'in{i}'] for i in range(len(g['nraw']))], int(g['frames'])


def test_restatement_reproduces_g20(g20):
    g, clips, frames = g20
    assert [len(c) for c in clips] == g['nraw'].tolist() and frames in g['nraw'] and g['nraw'].min() < frames < g['nraw'].max()
    sums, count = R.fit(clips, frames, apply_log=False)
    mean, mos, std = R.finish(sums, count)
    b1, b2 = R.summation_bounds([R.features(c, frames, False) for c in clips], frames)
    d1, d2 = np.abs(mean - g['mean_']), np.abs(mos - g['mean_of_square_'])
    print('mean_: max diff / bound', (d1 / np.maximum(b1, 1e-300)).max(), ' mean_of_square_:', (d2 / np.maximum(b2, 1e-300)).max())
    assert (d1 <= b1).all() and (d2 <= b2).all()
    zb, cb = int(g['zero_band']), int(g['const_band'])
    assert mean[zb] == 0 and mos[zb] == 0 and std[zb] == 0 and g['std_'][zb] == 0        # the band of zeros: variance exactly 0
    for a, b in ((mean, g['mean_']), (mos, g['mean_of_square_']), (std, g['std_'])):      # the band of integers: every sum exact
        assert a[cb] == b[cb]
    # std_ through the variance: |dvar| <= b2 + (2 |mean| + b1) b1, plus the roundings of square, difference, root and re-squaring
    # (each at most 2^-52 of the larger operand, mean_of_square_)
    dvar = np.abs(std ** 2 - g['std_'] ** 2)
    assert (dvar <= b2 + (2 * np.abs(g['mean_']) + b1) * b1 + 4 * 2.0 ** -52 * g['mean_of_square_']).all()


def test_json_round_trip_in_the_reference_format(g20, tmp_path):
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    g = g20[0]
    text = str(g['json'])
    ref_path = tmp_path / 'reference.json'
    ref_path.write_text(text)
    sc = Scaler()
    assert sc.mean_ is None and sc.std_ is None
    sc.load(str(ref_path))
    for k in ('mean_', 'mean_of_square_', 'std_'):
        a = getattr(sc, k)
        assert a.dtype == np.float64 and np.array_equal(a, g[k]), k                      # exactly: repr round-trips float64
    assert np.array_equal(sc.std_, np.sqrt(g['mean_of_square_'] - g['mean_'] ** 2))      # bit for bit the reference's formula
    assert np.array_equal(sc.std(sc.variance(sc.mean_, sc.mean_of_square_)), sc.std_)
    out = tmp_path / 'ours.json'
    sc.save(str(out))
    want, got = json.loads(text), json.loads(out.read_text())
    assert set(got) == {'mean_', 'mean_of_square_'} and got == want and isinstance(got['mean_'], list)
    assert sc.state_dict() == want
    sc2 = Scaler()
    sc2.load_state_dict(got)
    assert np.array_equal(sc2.std_, g['std_'])
    with pytest.raises(RuntimeError):
        Scaler().state_dict()                                                            # nothing fitted, nothing loaded


def test_host_normalize_matches_reference_normalize(g20):
    import torch
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    g, clips, frames = g20
    sc = Scaler()
    sc.load_state_dict(json.loads(str(g['json'])))
    for i in g['normalized']:
        x = np.zeros((1, frames, 64), np.float32)
        keep = min(len(clips[i]), frames)
        x[0, :keep] = clips[i][:keep]
        with np.errstate(invalid='ignore'):
            y = sc.normalize(torch.from_numpy(x))
            y64 = sc.normalize(x)
        assert y.dtype == torch.float32 and np.array_equal(y.numpy(), g[f'norm{i}'], equal_nan=True)
        assert y64.dtype == np.float64


def test_merge_of_two_halves_equals_the_whole(g20):
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    g, clips, frames = g20
    whole = Scaler.from_sums(*R.fit(clips, frames))
    h = len(clips) // 2
    a, b = Scaler.from_sums(*R.fit(clips[:h], frames)), Scaler.from_sums(*R.fit(clips[h:], frames))
    assert a.merge(b) is a and a.count_ == len(clips) == whole.count_ and b.count_ == len(clips) - h
    # the merged sums are the same per-clip terms added in another order: 2 (n - 1) u sum|term| over the n clips; the division by
    # the count rounds once on each side (u |value| each)
    terms = np.stack([R.clip_stats(R.features(c, frames, False), frames) for c in clips])
    n = len(clips)
    bound = (2 * (n - 1) * R.U * np.abs(terms).sum(0)) / n + 2 * R.U * np.abs(np.stack([whole.mean_, whole.mean_of_square_]))
    got = np.stack([a.mean_, a.mean_of_square_])
    d = np.abs(got - np.stack([whole.mean_, whole.mean_of_square_]))
    print('merge: max diff / bound', (d / np.maximum(bound, 1e-300)).max())
    assert (d <= bound).all()
    assert np.array_equal(a.std_, np.sqrt(a.mean_of_square_ - a.mean_ ** 2))
    loaded = Scaler()
    loaded.load_state_dict(whole.state_dict())
    with pytest.raises(ValueError):
        whole.merge(loaded)                                                              # a JSON file carries no count
    with pytest.raises(ValueError):
        Scaler.from_sums(np.zeros((3, 64)), 4)


def test_batches_may_be_pairs_and_fit_needs_frames():
    from sound_event_detection_transformer_amd.utilities import scaler as S
    clip = np.zeros((5, 64), np.float32)
    assert S._is_batch([clip, clip]) and S._is_batch(np.zeros((2, 5, 64))) and not S._is_batch(clip)
    with pytest.raises(ValueError):
        S.Scaler().update([clip])                                                        # frames not given: raised before any device work
    with pytest.raises(RuntimeError):
        S.Scaler(128).finalize()


def test_scaler_kwarg_of_the_transforms_validates(g20):
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform, DeviceViewTransform
    g = g20[0]
    sc = Scaler()
    sc.load_state_dict(json.loads(str(g['json'])))
    for cls in (DeviceBoxTransform, DeviceViewTransform):
        with pytest.raises(ValueError, match='not both'):
            cls(128, g['mean_'], g['std_'], scaler=sc)
        with pytest.raises(ValueError, match='not both'):
            cls(128, scaler_mean=g['mean_'], scaler=sc)
        with pytest.raises(ValueError, match='fitted or loaded'):
            cls(128, scaler=Scaler(128))
        tf = cls(128)                                                                    # the default: no scaler, no statistics
        assert tf.mean is None and tf.std is None
