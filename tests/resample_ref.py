"""Float64 restatement of the resampler's definition (the issue's text, not the product code):

    L / M = target_sr / orig_sr in lowest terms, s = min(1, L / M), quality (Z, rolloff, beta)
    w(u) = rolloff sinc(rolloff u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta) for |u| <= Z, else 0
    m[j] = mean over the channels of frame j;  int16 is worth x / 32768
    y[n] = sum_{0 <= j < N} s w(s (n M / L - j)) m[j],  n = 0 .. ceil(N L / M) - 1
    polyphase: i = (n M) div L, p = (n M) mod L, taps k = -H .. H + 1, H = floor(Z / s), T[p][k] = s w(s (p / L - k))
    identity (orig_sr == target_sr): one tap of weight 1.

Everything here is NumPy float64 with Python integers for n M and N L."""
import math
from fractions import Fraction

import numpy as np

QUALITY = {'kaiser_best': (64, 0.9475937167399596, 14.769656459379492), 'kaiser_fast': (16, 0.85, 8.555504641634386)}


def plan(orig_sr, target_sr, quality):
    """(L, M, s, H, taps): the identity has H = 0 and one tap"""
    f = Fraction(int(target_sr), int(orig_sr))
    L, M = f.numerator, f.denominator
    if L == M:
        return 1, 1, 1.0, 0, 1
    Z = QUALITY[quality][0]
    s = min(Fraction(1), f)
    H = math.floor(Z / s)
    return L, M, float(s), H, 2 * H + 2


def n_out(N, orig_sr, target_sr):
    f = Fraction(int(target_sr), int(orig_sr))
    return math.ceil(N * f)


def w(u, quality):
    Z, rolloff, beta = QUALITY[quality]
    u = np.asarray(u, np.float64)
    x = np.clip(1.0 - (u / Z) ** 2, 0.0, None)
    val = rolloff * np.sinc(rolloff * u) * np.i0(beta * np.sqrt(x)) / np.i0(beta)
    return np.where(np.abs(u) <= Z, val, 0.0)


def table(orig_sr, target_sr, quality):
    """T float64 [L][taps], column k + H holding tap k"""
    L, M, s, H, taps = plan(orig_sr, target_sr, quality)
    if L == M:
        return np.ones((1, 1))
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(-H, H + 2, dtype=np.float64)[None, :]
    return s * w(s * ((p - k * L) / L), quality)


def downmix(x):
    """float64 mono samples of a 1-D or interleaved (frames, channels) float32 / int16 array"""
    x = np.asarray(x)
    m = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    return m if m.ndim == 1 else m.mean(axis=1)


def resample_at(x, orig_sr, target_sr, quality, n_indices, with_abs=False, dtype=np.float64):
    """y[n] for the chosen n (a sequence of ints), through the polyphase form; with_abs: also sum_k |T[p][k] m[i + k]|, the
    quantity the f32 error bound scales with.  dtype = float32 runs the same sum sequentially in f32 (table and mix rounded first)."""
    L, M, s, H, taps = plan(orig_sr, target_sr, quality)
    T = table(orig_sr, target_sr, quality)
    m = downmix(x)
    N = len(m)
    if dtype == np.float32:
        T, m = T.astype(np.float32), m.astype(np.float32)
    n = [int(v) for v in n_indices]
    i = np.array([(v * M) // L for v in n], np.int64)
    p = np.array([(v * M) % L for v in n], np.int64)
    y = np.zeros(len(n), dtype)
    a = np.zeros(len(n), np.float64)
    for c in range(taps):                                   # tap k = c - H, ascending: the order the kernel sums in
        j = i + (c - H)
        ok = (j >= 0) & (j < N)
        term = T[p, c] * np.where(ok, m[np.clip(j, 0, N - 1)], 0)
        y = (y + term).astype(dtype)
        a += np.abs(term.astype(np.float64))
    return (y, a) if with_abs else y


def resample(x, orig_sr, target_sr, quality, with_abs=False, dtype=np.float64):
    N = np.asarray(x).shape[0]
    return resample_at(x, orig_sr, target_sr, quality, range(n_out(N, orig_sr, target_sr)), with_abs, dtype)


def resample_direct(x, orig_sr, target_sr, quality):
    """the defining sum itself, every j, no polyphase indexing - for short inputs"""
    L, M, s, H, taps = plan(orig_sr, target_sr, quality)
    m = downmix(x)
    N = len(m)
    if L == M:
        return m.copy()
    n = np.arange(n_out(N, orig_sr, target_sr), dtype=np.float64)[:, None]
    j = np.arange(N, dtype=np.float64)[None, :]
    return (s * w(s * ((n * M - j * L) / L), quality)) @ m


def kaiser_delta(quality):
    """Kaiser's formula: stop-band attenuation A = beta / 0.1102 + 8.7 dB, ripple delta = 10^(-A / 20)"""
    return 10.0 ** (-(QUALITY[quality][2] / 0.1102 + 8.7) / 20.0)


# the unit tones of the filter test, as fractions of nyq = min(orig_sr, target_sr) / 2: (pass-band, stop-band) per quality
RATIOS = [(44100, 16000), (48000, 44100), (16000, 44100)]
TONES = {'kaiser_best': ((0.0125, 0.5, 0.8), (1.073, 1.3)), 'kaiser_fast': ((0.0125, 0.5), (1.173, 1.3))}


def tone_case(o, t, q, frac, N=6000):
    """(x, inner output indices, their analytic values: zeros for a stop-band tone), or None for a tone the source cannot hold"""
    L, M, s, H, taps = plan(o, t, q)
    f = frac * min(o, t) / 2.0
    if f >= o / 2.0:
        return None
    x = np.cos(2.0 * np.pi * f * np.arange(N) / o + 0.3)
    n = np.arange(n_out(N, o, t))
    i = (n * M) // L
    inner = n[(i - H >= 0) & (i + H + 1 < N)]
    return x, inner, (np.cos(2.0 * np.pi * f * inner / t + 0.3) if frac < 1.0 else np.zeros(len(inner)))
