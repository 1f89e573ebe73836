"""CPU: the resampler's host half (utilities/resample.py: resample_plan, resample_table) and the float64 restatement the GPU tests
measure against (tests/resample_ref.py).

  1. plans and output lengths;
  2. the product's f32 table against the restatement's float64 one: 2^-24 of the largest coefficient;
  3. the restatement against scipy.signal.upfirdn over the dense prototype filter, 1e-12;
  4. the filter is what it claims: unit tones against their analytic resampled values away from the ends, within 2 delta,
     delta = 10^(-A / 20), A = beta / 0.1102 + 8.7 (Kaiser's formula; one delta for pass-band ripple, one for aliased images):
     1.5e-7 for kaiser_best, 9.7e-5 for kaiser_fast.  Measured here (restatement alone): at most 4.7e-8 / 5.4e-5.  A stop-band
     tone is one the source can hold: at or above the source's own Nyquist frequency the sampled sequence IS its alias, a tone of
     unit amplitude below it, and no resampler can tell the two apart - so 1.3 nyq is not a case for 48000 -> 44100 (28.7 kHz at
     48 kHz is 19.3 kHz) and neither stop-band tone is one for 16000 -> 44100, where every tone the source holds is pass-band
     or transition band;
  5. refusals."""
import math

import numpy as np
import pytest
import scipy.signal

import resample_ref as R

RATIOS, TONES, tone_case = R.RATIOS, R.TONES, R.tone_case


def test_plans_and_lengths():
    from sound_event_detection_transformer_amd.utilities.resample import resample_plan, resampled_length
    p = resample_plan(44100, 16000, 'kaiser_best')
    assert (p.L, p.M, p.H, p.taps) == (160, 441, 176, 354) and p.s == 160 / 441
    assert [resampled_length(n, p) for n in (441, 442, 1, 882, 883)] == [160, 161, 1, 320, 321]
    assert resampled_length(13_500_000, p) == math.ceil(13_500_000 * 160 / 441) == 4_897_960
    up = resample_plan(16000, 44100, 'kaiser_fast')
    assert (up.L, up.M, up.s, up.H, up.taps) == (441, 160, 1.0, 16, 34) and [resampled_length(n, up) for n in (1, 160, 161)] == [3, 441, 444]
    assert (resample_plan(48000, 16000).L, resample_plan(48000, 16000).M, resample_plan(48000, 16000).taps) == (1, 3, 386)
    assert (resample_plan(48000, 44100).L, resample_plan(48000, 44100).M, resample_plan(48000, 44100).taps) == (147, 160, 2 * 69 + 2)
    ident = resample_plan(44100, 44100, 'kaiser_fast')
    assert (ident.L, ident.M, ident.H, ident.taps) == (1, 1, 0, 1) and resampled_length(12345, ident) == 12345
    for o, t, q in [(44100, 16000, 'kaiser_best'), (16000, 44100, 'kaiser_fast'), (22050, 44100, 'kaiser_best'), (7, 7, 'kaiser_best')]:
        p = resample_plan(o, t, q)
        assert (p.L, p.M, p.H, p.taps) == tuple(np.array(R.plan(o, t, q))[[0, 1, 3, 4]].astype(int))
        assert all(resampled_length(n, p) == R.n_out(n, o, t) for n in (1, 2, 7, 441, 442, 1003, 10 ** 9 + 7))


@pytest.mark.parametrize('o,t,q', [(44100, 16000, 'kaiser_best'), (48000, 16000, 'kaiser_best'), (48000, 44100, 'kaiser_fast'),
                                   (16000, 44100, 'kaiser_fast'), (22050, 44100, 'kaiser_best'), (16000, 16000, 'kaiser_best')])
def test_product_table_against_the_restatement(o, t, q):
    from sound_event_detection_transformer_amd.utilities.resample import device_table, resample_plan, resample_table
    plan = resample_plan(o, t, q)
    T, ref = resample_table(plan), R.table(o, t, q)
    assert T.dtype == np.float32 and T.shape == ref.shape == (plan.L, plan.taps)
    err = np.abs(T.astype(np.float64) - ref).max()
    print(f'{o}->{t} {q}: table {T.shape}, {T.nbytes} bytes, max |T - ref| = {err:.2e}, bound {2.0 ** -24 * np.abs(ref).max():.2e}')
    assert err <= 2.0 ** -24 * np.abs(ref).max()
    D = device_table(T, plan)                                      # [taps][L], column n mod L
    assert D.shape == (plan.taps, plan.L)
    for n in (0, 1, plan.L - 1, plan.L, 3 * plan.L + 2):
        assert np.array_equal(D[:, n % plan.L], T[(n * plan.M) % plan.L])


@pytest.mark.parametrize('o,t,q', [(44100, 16000, 'kaiser_best'), (48000, 44100, 'kaiser_fast'), (16000, 44100, 'kaiser_fast'),
                                   (22050, 44100, 'kaiser_best'), (48000, 16000, 'kaiser_fast')])
def test_restatement_against_upfirdn(o, t, q):
    L, M, s, H, taps = R.plan(o, t, q)
    Z = R.QUALITY[q][0]
    half = math.ceil(Z * L / s)
    pad = (-half) % M                                              # zeros in front: the filter's centre lands on a multiple of M
    h = np.concatenate([np.zeros(pad), s * R.w(s * (np.arange(-half, half + 1, dtype=np.float64) / L), q)])
    c = (half + pad) // M
    rng = np.random.default_rng(o + t)
    worst = 0.0
    for N in (1, 2, 7, 441, 442, 1003):
        x = rng.standard_normal(N)
        n = R.n_out(N, o, t)
        want = scipy.signal.upfirdn(h, x, up=L, down=M)[c:c + n]
        got = R.resample(x, o, t, q)
        assert got.shape == want.shape == (n,)
        worst = max(worst, np.abs(got - want).max())
        if N <= 442:
            assert np.abs(R.resample_direct(x, o, t, q) - want).max() <= 1e-12
    print(f'{o}->{t} {q}: restatement vs upfirdn {worst:.2e}')
    assert worst <= 1e-12


@pytest.mark.parametrize('q', sorted(TONES))
@pytest.mark.parametrize('o,t', RATIOS)
def test_unit_tones(o, t, q):
    bound = 2.0 * R.kaiser_delta(q)
    assert abs(bound - {'kaiser_best': 1.5e-7, 'kaiser_fast': 9.7e-5}[q]) < 0.04 * bound
    cases = [(frac, tone_case(o, t, q, frac)) for frac in TONES[q][0] + TONES[q][1]]
    assert sum(c is None for _, c in cases) == {(44100, 16000): 0, (48000, 44100): 1 if q == 'kaiser_best' else 2, (16000, 44100): 2}[(o, t)]
    for frac, case in cases:
        if case is None:
            continue
        x, inner, ideal = case
        assert len(inner) > 500
        err = np.abs(R.resample_at(x, o, t, q, inner) - ideal).max()
        print(f'{o}->{t} {q}: tone at {frac} nyq, {len(inner)} outputs: {err:.2e} (bound {bound:.2e})')
        assert err <= bound


def test_refusals():
    from sound_event_detection_transformer_amd.utilities.resample import resample_plan
    for o, t in [(0, 16000), (16000, 0), (-44100, 16000), (44100.5, 16000), (True, 16000)]:
        with pytest.raises(ValueError, match='positive integers'):
            resample_plan(o, t)
    with pytest.raises(ValueError, match='quality'):
        resample_plan(44100, 16000, 'sinc_best')
    with pytest.raises(ValueError, match='envelope'):
        resample_plan(44101, 16000)                                # L = 16000
    with pytest.raises(ValueError, match='envelope'):
        resample_plan(16000, 16001)                                # M = 16000
    with pytest.raises(ValueError, match='envelope'):
        resample_plan(48000, 1000, 'kaiser_best')                  # a workgroup's input span: 1024 * 48 + 6146 floats
    assert resample_plan(48000, 8000, 'kaiser_best').taps == 770
