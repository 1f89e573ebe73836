"""CPU: the paired (teacher, student) input transform of the mean-teacher recipe - fixture G19 (the reference's own transform
objects run through Transform.__call__, tests/golden/make_golden_noise.py) against our restatement of the noise step and of the
pair's draw order (tests/noise_views_ref.py), the host-side draws of DeviceViewTransform, the record's size, and the statistics of
the counter-based normal stream the kernel draws from (on its numpy mirror; tests/test_noise_views_gpu.py ties the device to the
mirror within 1e-4 per sample)."""
import os

import numpy as np
import pytest

import noise_views_ref as R

G19_P = dict(tm=(0.0, 0.1, 0.6), fm=(0.03, 0.4, 0.6), fs=(0.6, 4, 0, 2))          # the raised probabilities the fixture used


def _g19(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g19_noise_views.npz'))
    return g, [g[f'in{i}'] for i in range(len(g['seeds']))]


def test_g19_restated_chain_reproduces_the_reference_pair(golden_dir):
    g, clips = _g19(golden_dir)
    frames, F = int(g['frames']), clips[0].shape[1]
    on = g['params'][:, R.NOISE] > 0
    long_ = g['nraw'] > frames
    assert (on & long_).any() and (on & ~long_).any() and (~on & long_).any() and (~on & ~long_).any()
    for i, clip in enumerate(clips):
        np.random.seed(int(g['seeds'][i]))
        row, z = R.draw_pair(len(clip), F, float(g['p']), **G19_P)
        np.testing.assert_array_equal(row, g['params'][i])
        v0, v1 = R.views(clip, row, z, frames, g['scaler_mean'], g['scaler_std'], float(g['snr']))
        # tolerance of test_g13_transform_kernel_matches_reference_classes: the only new arithmetic is one addition
        np.testing.assert_allclose(v0, g[f'out{i}_v0'], rtol=2e-6, atol=2e-5)
        np.testing.assert_allclose(v1, g[f'out{i}_v1'], rtol=2e-6, atol=2e-5)
        assert (z is not None) == bool(on[i])
        if on[i]:
            assert np.abs(v1 - v0).max() > 1e-3


def test_draw_batch_host_mode_follows_the_reference_order(golden_dir):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceViewTransform
    g, clips = _g19(golden_dir)
    frames, F = int(g['frames']), clips[0].shape[1]
    tf = DeviceViewTransform(frames, g['scaler_mean'], g['scaler_std'], noise_snr=float(g['snr']), noise_p=float(g['p']), time_mask=True,
                             freq_mask=True, freq_shift=True, noise='host', apply_log=False, device='cpu', **G19_P)
    want = R.records(g['params'], g['nraw'], frames, F)
    for i, clip in enumerate(clips):
        np.random.seed(int(g['seeds'][i]))
        rec, normals = tf.draw_batch([len(clip)])
        assert rec[0] == want[i], (rec[0], want[i])
        if g['params'][i, R.NOISE]:
            assert normals[0].shape == clip.shape and normals[0].dtype == np.float64
            np.testing.assert_array_equal(normals[0].reshape(-1)[:8], g['normals_head'][i])
        else:
            assert normals[0] is None
    # a whole batch consumes the generator clip by clip: two clips after one seed = the two single draws back to back
    np.random.seed(7)
    a, na = tf.draw_batch([120, 150])
    np.random.seed(7)
    b0, n0 = tf.draw_batch([120])
    b1, n1 = tf.draw_batch([150])
    assert a[0] == b0[0] and a[1] == b1[0]
    # mode 'device': no normals on the host, so the later draws of a seeded run differ from mode 'host' once a clip takes the noise
    td = DeviceViewTransform(frames, noise_p=float(g['p']), time_mask=True, freq_mask=True, freq_shift=True, device='cpu', **G19_P)
    np.random.seed(int(g['seeds'][1]))
    rec, normals = td.draw_batch([len(clips[1])])
    assert normals is None and rec['noise_on'][0] == 1 and rec[0] != want[1]
    np.random.seed(int(g['seeds'][0]))                              # noise not applied: the same stream in both modes
    assert td.draw_batch([len(clips[0])])[0][0] == want[0]


def test_record_size_and_unsupported_branch():
    from sound_event_detection_transformer_amd import _build, lib
    from sound_event_detection_transformer_amd.utilities.transforms import _AUG, _VAUG, DeviceViewTransform
    _build.build()
    assert lib.load().sedt_sizeof(12) == _VAUG.itemsize == 2 * _AUG.itemsize + 8
    assert _VAUG.fields['noise_on'][1] == 2 * _AUG.itemsize
    with pytest.raises(ValueError, match='snr branch'):
        DeviceViewTransform(496, noise_snr=None, noise_std=0.5, device='cpu')
    with pytest.raises(ValueError, match='snr branch'):
        DeviceViewTransform(496, noise_std=0.5, device='cpu')
    with pytest.raises(ValueError):
        DeviceViewTransform(496, noise='numpy', device='cpu')


def test_recipe_helper_builds_the_paired_transform():
    from sound_event_detection_transformer_amd.utilities import synthetic as S
    tf = S.semi_pair_transform(496, 'cpu')
    assert tf.noise == 'device' and tf.noise_snr == 30.0 and tf.noise_p == 0.5 and tf.time_mask and tf.freq_mask and not tf.freq_shift
    assert float(tf.mean[0]) == S.SEMI_SCALER[0] and float(tf.std[0]) == S.SEMI_SCALER[1]


# ---- the drawn stream at C5's size: 64 clips x 496 frames x 64 bands.  These are conditions (5 sigma of the estimator under the null,
# the 0.1 % Kolmogorov-Smirnov critical value), fixed before the generator was run; the seeds are fixed, not selected.
NB, NT, NF = 64, 496, 64
N = NB * NT * NF
STREAM_SEEDS = [0, 1, 12345, 0xdeadbeef]


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize('seed', STREAM_SEEDS)
def test_drawn_stream_is_standard_normal_and_uncorrelated(seed):
    from scipy import stats
    z = R.normals(seed, 0, N)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5 / np.sqrt(N)
    assert abs(z.std() - 1) < 5 / np.sqrt(2 * N)
    c = z.reshape(NB, NT, NF)
    lim = 5 / np.sqrt(N)
    assert abs(_corr(c[:, :-1].ravel(), c[:, 1:].ravel())) < lim           # along time
    assert abs(_corr(c[:, :, :-1].ravel(), c[:, :, 1:].ravel())) < lim     # along mel (within and across Box-Muller pairs)
    assert abs(_corr(c[:-1].ravel(), c[1:].ravel())) < lim                 # between consecutive clips
    d = stats.kstest(z, 'norm').statistic
    assert d < 1.95 / np.sqrt(N), d
    n = 1 << 20                                                            # the step-to-step case: seed and seed + 1
    assert abs(_corr(z[:n], R.normals(seed + 1, 0, n))) < 5 / np.sqrt(n)


def test_stream_offset_continues_the_stream():
    a = R.normals(5, 0, 4096)
    assert np.array_equal(R.normals(5, 1024, 1024), a[1024:2048])
    assert np.array_equal(R.normals(5, 2 ** 33 + 2, 64), R.normals(5, 2 ** 33, 66)[2:])       # the high index word takes part
    assert not np.array_equal(R.normals(5, 2 ** 32, 64), a[:64])
    assert np.abs(a).max() <= np.sqrt(-2 * np.log(2.0 ** -24))
