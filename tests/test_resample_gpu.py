"""GPU: the resampler (sedt_resample, utilities/resample.py) against the float64 restatement tests/resample_ref.py.

The bound is derived, not measured, and holds per output sample:

    |got - ref| <= (taps + 4) 2^-24 sum_k |T[p][k] m[i + k]|        (the sum from the float64 restatement)

the forward error of an f32 FMA summation of ``taps`` terms in any order, plus one rounding each for the coefficient, the mix
and the store.  Every comparison prints its worst ratio to this bound, and beside it what the restatement run sequentially in
f32 on the CPU differs from float64 by (absolute).

Shapes: the smallest at which the kernel can go wrong.  Ratios 44100 -> 16000 kaiser_best (L = 160, a 221 KB table, beyond LDS),
48000 -> 16000 kaiser_best (L = 1), 48000 -> 44100 kaiser_fast, 16000 -> 44100 kaiser_fast (up, L = 441), 22050 -> 44100 kaiser_best
(L = 2); lengths 1, 2, H - 1, H, H + 1, 2 H + 3 (the filter overhangs both ends at once), lengths giving BLK - 1, BLK, BLK + 1 and
3 BLK + 1 outputs (BLK = lib.RESAMPLE_BLK outputs per workgroup; up-sampling steps over some output counts: there the first
length that gives at least as many), and two lengths with N L mod M equal to 0 and to 1.

Measured on an MI355X ("Resampling and down-mix", has the paragraph): worst ratio to the bound 0.030 for the kaiser_best
ragged batches (354 / 386 taps), 0.070 for 22050 -> 44100, 0.15 for kaiser_fast (34 / 36 taps); stereo / 3-channel / int16 input
0.021 - 0.036; 13.5 M samples 0.024 around n M = 2^31 and 0.034 at the end.  |got - ref| is 4e-7 .. 2.4e-6 on unit-variance noise and
unit tones, and the sequential f32 restatement on the CPU is the same 4e-7 .. 2.4e-6 from float64.  Tones: kaiser_best 4.0e-7 .. 8.5e-7
from the analytic value in the pass band, at most 1.3e-7 in the stop band; kaiser_fast at most 5.4e-5 (0.54 of 2 delta + the f32 bound)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu

CASES = [(44100, 16000, 'kaiser_best'), (48000, 16000, 'kaiser_best'), (48000, 44100, 'kaiser_fast'), (16000, 44100, 'kaiser_fast'),
         (22050, 44100, 'kaiser_best')]
GUARD = float('nan')


@functools.lru_cache(maxsize=None)
def _rs(o, t, q):
    from sound_event_detection_transformer_amd.utilities.resample import DeviceResampler
    return DeviceResampler(o, t, q)


def _blk():
    from sound_event_detection_transformer_amd import lib
    return lib.RESAMPLE_BLK


def _lengths(o, t, q):
    L, M, s, H, taps = R.plan(o, t, q)
    ns = [1, 2, H - 1, H, H + 1, 2 * H + 3]
    for target in (_blk() - 1, _blk(), _blk() + 1, 3 * _blk() + 1):
        N = max(target * M // L, 1)
        while R.n_out(N, o, t) < target:
            N += 1
        ns.append(N)
    inv = pow(L, -1, M) if M > 1 else 1
    ns += [3 * M, inv + 2 * M]                                     # N L mod M = 0 and = 1
    assert (ns[-2] * L) % M == 0 and (ns[-1] * L) % M == 1 % M
    return [n for n in ns if n >= 1]


@functools.lru_cache(maxsize=None)
def _ragged(o, t, q):
    """the ragged batch of one ratio: inputs, the device result of ONE launch as it came back, and the float64 references"""
    rng = np.random.default_rng(o + 7 * t)
    xs = [rng.standard_normal(n).astype(np.float32) for n in _lengths(o, t, q)]
    out, ns = _rs(o, t, q)(xs)
    torch.cuda.synchronize()
    refs = [R.resample(x, o, t, q, with_abs=True) for x in xs]
    return xs, out.cpu().numpy(), ns, refs


def _ratio(got, ref, a, taps):
    """worst |got - ref| over the derived bound (0 where both are exactly 0)"""
    bound = (taps + 4) * 2.0 ** -24 * a
    err = np.abs(got.astype(np.float64) - ref)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def _check(what, got, x, o, t, q, idx=None):
    idx = range(R.n_out(np.asarray(x).shape[0], o, t)) if idx is None else idx
    ref, a = R.resample_at(x, o, t, q, idx, with_abs=True)
    seq = R.resample_at(x, o, t, q, idx, dtype=np.float32)
    taps = R.plan(o, t, q)[4]
    ratio = _ratio(got, ref, a, taps)
    print(f'{what}: {len(ref)} outputs, worst {ratio:.3f} of the bound; |got - ref| <= {np.abs(got - ref).max():.2e}, sequential f32 on '
          f'the CPU {np.abs(seq - ref).max():.2e}')
    assert got.dtype == np.float32 and np.isfinite(got).all() and ratio <= 1.0, what
    return ratio


# ---------------------------------------------------------------------------------------------------------------- 1. ragged batches
@pytest.mark.parametrize('o,t,q', CASES)
def test_ragged_batch_at_the_edges(o, t, q):
    xs, got, ns, refs = _ragged(o, t, q)
    taps = R.plan(o, t, q)[4]
    assert ns == [R.n_out(len(x), o, t) for x in xs] and got.shape == (len(xs), max(ns))
    if o > t:
        assert {_blk() - 1, _blk(), _blk() + 1, 3 * _blk() + 1} <= set(ns)
    worst = 0.0
    for i, (x, (ref, a)) in enumerate(zip(xs, refs)):
        worst = max(worst, _ratio(got[i, :ns[i]], ref, a, taps))
        assert (got[i, ns[i]:] == 0).all(), 'samples past n_out are 0'
    seq = max(np.abs(R.resample(x, o, t, q, dtype=np.float32) - ref).max() for x, (ref, _) in zip(xs[-3:], refs[-3:]))
    print(f'{o}->{t} {q}: lengths {[len(x) for x in xs]} -> {ns}: worst {worst:.3f} of the bound; sequential f32 on the CPU {seq:.2e}')
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. input forms
def test_int16_gives_the_bits_of_the_scaled_f32_batch():
    o, t, q = 48000, 16000, 'kaiser_best'
    rng = np.random.default_rng(16)
    pcm = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (1, 777, 3 * _blk() + 5)]
    pcm[1][:2] = (-32768, 32767)
    a, ns = _rs(o, t, q)(pcm)
    b, _ = _rs(o, t, q)([p.astype(np.float32) / np.float32(32768.0) for p in pcm])
    assert torch.equal(a, b)
    _check('int16 mono', a[2, :ns[2]].cpu().numpy(), pcm[2], o, t, q)


@pytest.mark.parametrize('channels', [2, 3])
def test_interleaved_channels_against_the_restatement(channels):
    o, t, q = 44100, 16000, 'kaiser_best'
    rng = np.random.default_rng(channels)
    f = rng.standard_normal((2 * _blk() * 441 // 160 + 13, channels)).astype(np.float32)
    i = rng.integers(-32768, 32768, (1501, channels)).astype(np.int16)
    out, ns = _rs(o, t, q)([f, i, f[:, 0].copy()])
    got = out.cpu().numpy()
    _check(f'{channels} channels f32', got[0, :ns[0]], f, o, t, q)
    _check(f'{channels} channels int16', got[1, :ns[1]], i, o, t, q)
    _check('mono beside them', got[2, :ns[2]], f[:, 0], o, t, q)


def test_identity_plan():
    rs = _rs(16000, 16000, 'kaiser_best')
    assert (rs.plan.L, rs.plan.M, rs.plan.taps) == (1, 1, 1)
    rng = np.random.default_rng(1)
    mono = rng.standard_normal(2 * _blk() + 3).astype(np.float32)
    mono[:2] = (-0.0, np.float32(-3e38))
    stereo = rng.standard_normal((_blk() + 1, 2)).astype(np.float32)
    pcm = rng.integers(-32768, 32768, (300, 2)).astype(np.int16)
    out, ns = rs([mono, stereo, pcm])
    got = out.cpu().numpy()
    assert ns == [len(mono), len(stereo), len(pcm)]
    assert np.array_equal(got[0, :ns[0]].view(np.uint32), mono.view(np.uint32)), 'a mono f32 input comes out bit for bit'
    assert np.array_equal(got[1, :ns[1]], stereo.astype(np.float64).mean(axis=1).astype(np.float32)), 'a stereo input comes out as its mean'
    assert np.array_equal(got[2, :ns[2]], (pcm.astype(np.float64).mean(axis=1) / 32768.0).astype(np.float32))
    assert (got[1, ns[1]:] == 0).all() and (got[2, ns[2]:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize('o,t,q', [CASES[0], CASES[1], CASES[3]])
def test_bits_do_not_depend_on_the_batch(o, t, q):
    xs, got, ns, _ = _ragged(o, t, q)
    rs = _rs(o, t, q)
    for i in range(len(xs)):                                       # alone
        alone, n1 = rs([xs[i]])
        assert n1 == [ns[i]] and np.array_equal(alone.cpu().numpy()[0].view(np.uint32), got[i, :ns[i]].view(np.uint32)), i
    wide = torch.full((len(xs), max(ns) + 2 * _blk() + 7), GUARD, device='cuda')     # reversed, into a wider output
    out, nr = rs(xs[::-1], out=wide)
    assert out is wide and nr == ns[::-1]
    back = wide.cpu().numpy()[::-1]
    for i in range(len(xs)):
        assert np.array_equal(back[i, :ns[i]].view(np.uint32), got[i, :ns[i]].view(np.uint32)), i
        assert (back[i, ns[i]:] == 0).all() and not np.signbit(back[i, ns[i]:]).any(), 'rows past n_out are written as 0'


def test_captured_launch_replays_on_new_input():
    o, t, q = 44100, 16000, 'kaiser_best'
    rs = _rs(o, t, q)
    rng = np.random.default_rng(3)
    n = [2 * _blk() * 441 // 160 + 1, 500]
    first = [rng.standard_normal((n[0], 2)).astype(np.float32), rng.integers(-32768, 32768, n[1]).astype(np.int16)]
    second = [rng.standard_normal((n[0], 2)).astype(np.float32), rng.integers(-32768, 32768, n[1]).astype(np.int16)]
    src = [torch.from_numpy(x).cuda() for x in first]
    ns = [rs.n_out(v) for v in n]
    dst = torch.full((2, max(ns) + 5), GUARD, device='cuda')
    clips = [(src[0], n[0], 2), (src[1], n[1], 1)]
    run = rs.prepare(clips, dst.view(-1), [0, dst.shape[1]], [dst.shape[1]] * 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for batch in (first, second):
        for s, x in zip(src, batch):
            s.copy_(torch.from_numpy(x))
        dst.fill_(GUARD)
        g.replay()
        torch.cuda.synchronize()
        eager, _ = rs(batch)
        assert torch.equal(dst[:, :eager.shape[1]], eager) and (dst[:, eager.shape[1]:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4. tones
@pytest.mark.parametrize('q', sorted(R.TONES))
@pytest.mark.parametrize('o,t', R.RATIOS)
def test_unit_tones_on_the_device(o, t, q):
    """the tones of tests/test_resample_cpu.py: |got - ideal| <= 2 delta + the derived f32 bound, away from the ends"""
    cases = [(frac, R.tone_case(o, t, q, frac)) for frac in R.TONES[q][0] + R.TONES[q][1]]
    cases = [(frac, c) for frac, c in cases if c is not None]
    xs = [c[0].astype(np.float32) for _, c in cases]
    out, ns = _rs(o, t, q)(xs)
    got = out.cpu().numpy()
    taps = R.plan(o, t, q)[4]
    for k, (frac, (_, inner, ideal)) in enumerate(cases):
        ref, a = R.resample_at(xs[k], o, t, q, inner, with_abs=True)
        err = np.abs(got[k, inner].astype(np.float64) - ideal)
        allowed = 2.0 * R.kaiser_delta(q) + (taps + 4) * 2.0 ** -24 * a
        seq = np.abs(R.resample_at(xs[k], o, t, q, inner, dtype=np.float32) - ref).max()
        print(f'{o}->{t} {q}: tone at {frac} nyq: |got - ideal| <= {err.max():.2e}, worst {float((err / allowed).max()):.3f} of 2 delta + f32 bound; '
              f'|got - ref| <= {np.abs(got[k, inner] - ref).max():.2e}, sequential f32 on the CPU {seq:.2e}')
        assert (err <= allowed).all(), frac


# ---------------------------------------------------------------------------------------------------------------- 5. 64-bit indices
def test_indices_past_2_to_the_31():
    o, t, q, N = 44100, 16000, 'kaiser_best', 13_500_000
    L, M = 160, 441
    assert N * L > 2 ** 31
    x = np.random.default_rng(31).standard_normal(N).astype(np.float32)
    out, ns = _rs(o, t, q)([torch.from_numpy(x)])
    assert ns == [4_897_960] == [R.n_out(N, o, t)] and out.shape == (1, ns[0])
    around = np.arange(4_869_557 - 1000, 4_869_557 + 1000)
    assert (around[0] * M < 2 ** 31 <= around[-1] * M)             # n M passes 2^31 inside the window
    last = np.arange(ns[0] - 2000, ns[0])
    first = np.arange(0, 500)
    for what, idx in (('around n M = 2^31', around), ('the last outputs', last), ('the first outputs', first)):
        _check(f'13.5 M samples, {what}', out[0, torch.from_numpy(idx).cuda()].cpu().numpy(), x, o, t, q, idx)


# ---------------------------------------------------------------------------------------------------------------- 6. envelope
def test_envelope_predicate_and_entry_point_agree():
    from sound_event_detection_transformer_amd import lib
    l = lib.load()
    bogus = ctypes.c_void_p(8)                                     # never read: B = 0, or the refusal comes first
    inside = [(160, 441, 354, 176, 1, 1), (1, 3, 386, 192, 64, 1 << 40), (441, 160, 34, 16, 2, 10), (1, 1, 1, 0, 1, 1), (4096, 4095, 130, 64, 1, 1),
              (1, 6, 770, 384, 3, 5), (1, 1, 8192, 8191, 1, 1), (2, 1, 130, 64, 1, 1)]
    outside = [(0, 1, 1, 0, 1, 1), (4097, 1, 130, 64, 1, 1), (1, 4097, 130, 64, 1, 1), (1, 1, 0, 0, 1, 1), (1, 1, 8193, 0, 1, 1), (1, 1, 2, 2, 1, 1),
               (1, 1, 2, -1, 1, 1), (4096, 4095, 1026, 512, 1, 1), (1, 48, 6146, 3072, 1, 1), (1, 16, 2050, 1024, 1, 1), (160, 441, 354, 176, 0, 1),
               (160, 441, 354, 176, 65, 1), (160, 441, 354, 176, 1, 0), (160, 441, 354, 176, 1, (1 << 40) + 1)]
    for args, want in [(a, 1) for a in inside] + [(a, 0) for a in outside]:
        assert l.sedt_resample_ok(*args) == want, args
        status = l.sedt_resample(bogus, 0, 1, bogus, *args, None)
        assert (status == 0) == bool(want), args
        if not want:
            assert 'envelope' in l.sedt_last_error().decode()
            assert l.sedt_resample(None, 1, 1, None, *args, None) != 0 and 'envelope' in l.sedt_last_error().decode()
    assert l.sedt_resample(None, 1, 1, None, 160, 441, 354, 176, 1, 1, None) != 0 and 'null pointer' in l.sedt_last_error().decode()
    assert l.sedt_resample(bogus, 65536, 1, bogus, 160, 441, 354, 176, 1, 1, None) != 0 and 'B=65536' in l.sedt_last_error().decode()
    assert l.sedt_resample(bogus, 1, 0, bogus, 160, 441, 354, 176, 1, 1, None) != 0 and 'max_out=0' in l.sedt_last_error().decode()


def test_python_refusals():
    rs = _rs(44100, 16000, 'kaiser_best')
    with pytest.raises(ValueError, match='float32 or int16'):
        rs([np.zeros(10, np.float64)])
    with pytest.raises(ValueError, match='at least one'):
        rs([np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match='channels'):
        rs([np.zeros((4, 65), np.float32)])
    with pytest.raises(ValueError, match='lengths'):
        rs([np.zeros(4, np.float32)], lengths=[5])
    with pytest.raises(ValueError, match='out:'):
        rs([np.zeros(4410, np.float32)], out=torch.empty((1, 100), device='cuda'))
    dst = torch.empty(100, device='cuda')
    with pytest.raises(ValueError, match='does not fit'):
        rs.launch([(torch.zeros(10, device='cuda'), 11, 1)], dst, [0], [100])
    with pytest.raises(ValueError, match='does not fit'):
        rs.launch([(torch.zeros(10, device='cuda'), 10, 1)], dst, [1], [100])
