"""GPU: both mean-teacher views from one raw clip in one launch (sedt_box_transform_views, utilities.transforms.DeviceViewTransform)
- against fixture G19 (the reference's own transform objects), the float64 oracle chain at the real shape, and the numpy mirror of
the kernel's counter-based normal stream (tests/noise_views_ref.py; its distribution is checked in tests/test_noise_views_cpu.py).

Bounds and where they come from:
  G19, injected normals        rtol 2e-6, atol 2e-5 (that of the single-view G13 test): the device adds in f32 where the reference
                               adds an f32 to an f64; |x| <= 100, scaler std >= 7.7 -> at most 2 * 2^-24 * 100 / 7.7 = 1.5e-6
  log chain, injected / drawn  rtol 2e-5, atol 2e-4 (that of test_full_pipeline_with_log_matches_oracle); drawn mode adds
                               8.7 * 1e-4 * 0.0316 * 1.08 / 0.27 / 10 = 1.1e-5 for a 1e-4 difference in z
  drawn z against the mirror   |z_dev - z_mirror| <= 1e-4: moves the empirical CDF by at most 0.4 * 1e-4 = 4e-5, far under the 1.37e-3
                               limit on the Kolmogorov-Smirnov distance the CPU test holds the mirror to"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import transforms_oracle as TO
import noise_views_ref as R

pytestmark = pytest.mark.gpu

G19_P = dict(tm=(0.0, 0.1, 0.6), fm=(0.03, 0.4, 0.6), fs=(0.6, 4, 0, 2))


def _views_tf(frames, mean=None, std=None, **kw):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceViewTransform
    return DeviceViewTransform(frames, mean, std, **kw)


def _plain(nraws, noise_on=1):
    """records without masks or shifts"""
    from sound_event_detection_transformer_amd.utilities.transforms import _VAUG
    r = np.zeros(len(nraws), _VAUG)
    r['view']['nframes_raw'] = np.asarray(nraws)[:, None]
    r['noise_on'] = noise_on
    return r


def _oracle(amp, rec, k, frames, mean, std):
    q = rec['view'][k]
    return TO.box_transform(amp, frames, mean, std, (q['tm_t'] > 0, q['tm_t'] / frames + 1e-9, q['tm_t0'] / frames + 1e-9),
                            (bool(q['fm_on']), q['fm_f'] / 64 + 1e-9, q['fm_f0'] / 64 + 1e-9), (q['fs_shift'] != 0, int(q['fs_shift'])))


def test_g19_injected_normals_match_reference_pair(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g19_noise_views.npz'))
    n = len(g['seeds'])
    clips = [g[f'in{i}'] for i in range(n)]
    frames = int(g['frames'])
    tf = _views_tf(frames, g['scaler_mean'], g['scaler_std'], noise_snr=float(g['snr']), noise_p=float(g['p']), time_mask=True,
                   freq_mask=True, freq_shift=True, noise='host', apply_log=False, **G19_P)
    recs, normals = [], []
    for i, c in enumerate(clips):                                 # one seed per clip, as the fixture was made
        np.random.seed(int(g['seeds'][i]))
        r, z = tf.draw_batch([len(c)])
        recs.append(r[0])
        normals.append(z[0])
    recs = np.stack(recs)
    assert (recs == R.records(g['params'], g['nraw'], frames, 64)).all()
    x0, x1 = tf(clips, params=recs, normals=normals)
    assert x0.shape == x1.shape == (n, 1, frames, 64) and x0.dtype == x1.dtype == torch.float32
    x0, x1 = x0.cpu().numpy(), x1.cpu().numpy()
    for i in range(n):
        print('G19 clip', i, 'noise', int(recs['noise_on'][i]), 'max |diff| v0 %.3g v1 %.3g' %
              (np.abs(x0[i] - g[f'out{i}_v0']).max(), np.abs(x1[i] - g[f'out{i}_v1']).max()))
    for i in range(n):
        np.testing.assert_allclose(x0[i], g[f'out{i}_v0'], rtol=2e-6, atol=2e-5)
        np.testing.assert_allclose(x1[i], g[f'out{i}_v1'], rtol=2e-6, atol=2e-5)


def test_full_pipeline_with_log_injected_normals_matches_oracle():
    rng = np.random.RandomState(19)
    nraws = [400, 431, 496, 497, 520, 470]
    clips = [(10.0 ** (rng.randn(n, 64) / 2)).astype(np.float32) for n in nraws]
    mean, std = rng.randn(64) * 3 - 30, rng.rand(64) * 5 + 8
    tf = _views_tf(496, mean, std, noise_snr=30.0, noise_p=0.5, time_mask=True, freq_mask=True, freq_shift=True, noise='host',
                   tm=(0.0, 0.1, 0.6))
    np.random.seed(24)
    recs, normals = tf.draw_batch(nraws)
    assert 0 < recs['noise_on'].sum() < len(nraws) and (recs['view'][:, 1]['tm_t'] > 0).any() and recs['view']['fm_on'].any()
    normals = [None if z is None else z.astype(np.float32) for z in normals]          # what the device is given, exactly
    x0, x1 = (t.cpu().numpy() for t in tf(clips, params=recs, normals=normals))
    for i, c in enumerate(clips):
        noisy = c.astype(np.float64) + R.band_std(c, 30.0).astype(np.float64) * normals[i] if recs['noise_on'][i] else c
        r0, r1 = _oracle(c, recs[i], 0, 496, mean, std), _oracle(noisy, recs[i], 1, 496, mean, std)
        print('log chain clip', i, 'noise', int(recs['noise_on'][i]), 'max |diff| v0 %.3g v1 %.3g' %
              (np.abs(x0[i] - r0).max(), np.abs(x1[i] - r1).max()))
        np.testing.assert_allclose(x0[i], r0, rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(x1[i], r1, rtol=2e-5, atol=2e-4)


def test_drawn_normals_equal_the_mirror():
    B, T, F, seed, offset = 64, 496, 64, 12345, 2 * 10 ** 6
    gen = torch.Generator().manual_seed(7)
    x = (torch.rand(B, T, F, generator=gen) * 8 - 4)
    tf = _views_tf(T, apply_log=False, seed=seed)
    tf.offset = offset
    x0, x1 = tf(x.cuda(), params=_plain([T] * B))
    assert tf.offset == offset + B * T * F
    x0, x1 = x0.cpu().numpy()[:, 0].astype(np.float64), x1.cpu().numpy()[:, 0].astype(np.float64)
    assert np.array_equal(x0, x.numpy())
    sd = R.band_std(x.numpy().astype(np.float64), 30.0)[:, None, :]
    z_dev = (x1 - x0) / sd
    z_ref = R.normals(seed, offset, B * T * F).reshape(B, T, F)
    d = np.abs(z_dev - z_ref)
    print('drawn z: max |z_dev - z_mirror| %.3g, mean %.3g, max |z| %.3g' % (d.max(), d.mean(), np.abs(z_dev).max()))
    assert d.max() <= 1e-4
    # the device word added to the seed selects the stream of seed + word
    tf.offset = offset
    tf.seed_ptr = torch.tensor([3], dtype=torch.int32, device='cuda')
    y1 = tf(x[:2].cuda(), params=_plain([T] * 2))[1].cpu().numpy()[:, 0].astype(np.float64)
    z3 = R.normals(seed + 3, offset, 2 * T * F).reshape(2, T, F)
    assert np.abs((y1 - x0[:2]) / sd[:2] - z3).max() <= 1e-4


def test_drawn_mode_with_log_matches_oracle_fed_the_mirror():
    rng = np.random.RandomState(29)
    nraws = [520, 400, 496, 450]
    clips = [rng.uniform(0.5, 1.5, (n, 64)).astype(np.float32) for n in nraws]
    mean, std = np.zeros(64), np.full(64, 10.0)
    tf = _views_tf(496, mean, std, noise_snr=30.0, noise_p=1.0, time_mask=True, freq_mask=True, seed=77, tm=(0.0, 0.1, 0.6))
    tf.offset = 4096
    np.random.seed(31)
    recs, normals = tf.draw_batch(nraws)
    assert normals is None and recs['noise_on'].all()
    x0, x1 = (t.cpu().numpy() for t in tf(clips, params=recs))
    stride = max(nraws)
    z = R.normals(77, 4096, len(clips) * stride * 64).reshape(len(clips), stride, 64)
    for i, c in enumerate(clips):
        noisy = c.astype(np.float64) + R.band_std(c, 30.0).astype(np.float64) * z[i, :nraws[i]]
        assert np.abs(noisy).min() > 0.27
        r0, r1 = _oracle(c, recs[i], 0, 496, mean, std), _oracle(noisy, recs[i], 1, 496, mean, std)
        print('drawn log chain clip', i, 'max |diff| v0 %.3g v1 %.3g' % (np.abs(x0[i] - r0).max(), np.abs(x1[i] - r1).max()))
        np.testing.assert_allclose(x0[i], r0, rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(x1[i], r1, rtol=2e-5, atol=2e-4)


def test_behaviour_determinism_and_identity_with_the_single_view_kernel():
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    rng = np.random.RandomState(37)
    nraws = [431, 520, 496, 300, 470, 510]
    clips = [(10.0 ** (rng.randn(n, 64) / 2)).astype(np.float32) for n in nraws]
    clips[2][:, 5] = 0.0                                          # a band of zeros: std 0
    clips[3][:] = 0.0                                             # a silent clip
    mean, std = rng.randn(64) * 3 - 30, rng.rand(64) * 5 + 8
    kw = dict(time_mask=True, freq_mask=True, freq_shift=True, tm=(0.0, 0.1, 0.6))
    tf = _views_tf(496, mean, std, noise_p=0.5, seed=5, **kw)
    one = DeviceBoxTransform(496, mean, std, **kw)
    np.random.seed(41)
    recs, _ = tf.draw_batch(nraws)
    recs['noise_on'] = [1, 0, 1, 1, 0, 1]
    a0, a1 = tf(clips, params=recs)
    assert tf.offset == len(clips) * 520 * 64
    b0, b1 = tf(clips, params=recs)                               # the next call: other noise
    tf.offset = 0
    c0, c1 = tf(clips, params=recs)                               # the same (seed, offset): the same bits
    assert torch.equal(a0, c0) and torch.equal(a1, c1) and torch.equal(a0, b0)
    s0 = one(clips, params=np.ascontiguousarray(recs['view'][:, 0]))
    s1 = one(clips, params=np.ascontiguousarray(recs['view'][:, 1]))
    assert torch.equal(a0, s0)                                    # view 0 == the single-view kernel, bit for bit
    for i, on in enumerate(recs['noise_on']):
        if on and i != 3:
            assert not torch.equal(a1[i], s1[i]) and not torch.equal(a1[i], b1[i])
        if not on:
            assert torch.equal(a1[i], s1[i]) and torch.equal(b1[i], s1[i])
    assert torch.equal(a1[3], s1[3])                              # silence stays silence: every band has std 0
    for t in (a0, a1, b1):
        assert torch.isfinite(t).all()
    tn = _views_tf(496, apply_log=False, seed=5)                  # the zero band without the log: exactly no noise there
    n0, n1 = tn(clips[2:3], params=_plain([496]))
    assert torch.equal(n1[0, 0, :, 5], n0[0, 0, :, 5]) and not torch.equal(n1[0, 0, :, 6], n0[0, 0, :, 6]) and torch.isfinite(n1).all()


def test_prefetcher_yields_pairs_and_a_graphed_semi_step_takes_them():
    from sound_event_detection_transformer_amd import runtime, sedt
    from sound_event_detection_transformer_amd.engine import GraphedSemiStep, build_optimizer
    from sound_event_detection_transformer_amd.utilities.prefetch import DevicePrefetcher
    from sound_event_detection_transformer_amd.utilities.synthetic import semi_pair_transform, seeded_state_dict
    from sound_event_detection_transformer_amd.utilities.utils import EMA
    sys.path.insert(0, GOLDEN)
    import inputs as GI
    ns, nw, nu = 5, 5, 6
    B = ns + nw + nu
    rng = np.random.RandomState(43)
    batches = []
    for i in range(3):
        clips = [(10.0 ** (rng.randn(rng.randint(400, 520), 64) / 2)).astype(np.float32) for _ in range(B)]
        tg = GI.sparse_targets(B, 700 + i)
        for t in tg[ns:]:
            t['boxes'] = torch.zeros(0, 2)
        for t in tg[ns + nw:]:
            t['labels'] = torch.zeros(0, dtype=torch.int64)
        batches.append((clips, tg))
    tf = semi_pair_transform(496, 'cuda', seed=9)
    np.random.seed(47)
    want = [tuple(t.cpu() for t in tf(c)) for c, _ in batches]
    np.random.seed(47)
    tf.offset = 0
    got = []
    for inp, tgt in DevicePrefetcher(batches, transform=tf, targets_to_device=False):
        assert isinstance(inp, tuple) and len(inp) == 2 and inp[0].is_cuda and inp[1].is_cuda
        got.append((inp, tgt))
    assert len(got) == 3
    for (inp, _), w in zip(got, want):
        assert torch.equal(inp[0].cpu(), w[0]) and torch.equal(inp[1].cpu(), w[1]) and not torch.equal(w[0], w[1])
    # ---- the pair is what GraphedSemiStep takes: (x_teacher, x_student)
    runtime.set_compute_dtype('f32')
    model, crit, _ = sedt.build_model(sedt.default_args(enc_layers=6, num_queries=20, dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2023))
    model.cuda().train()
    crit.cuda()
    ema = EMA(model, 0.9)
    ema.register()
    opt = build_optimizer(model)
    masks = dict(mask_strong=slice(ns), mask_weak=slice(ns, ns + nw), mask_label=slice(ns + nw), mask_unlabel=slice(ns + nw, B))
    thr = torch.full((10,), 0.115).cuda()
    (xt, xs), tg = got[0]
    stepper = GraphedSemiStep(model, ema, crit, opt, xt, xs, tg, classwise_threshold=thr, mix_up_ratio=0.6, **masks)
    np.random.seed(3)
    losses = [float(stepper(inp[0], inp[1], tgt)[0]) for inp, tgt in got]
    torch.cuda.synchronize()
    assert len(losses) == 3 and np.isfinite(losses).all(), losses
