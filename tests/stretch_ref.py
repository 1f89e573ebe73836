"""The float64 restatement of "Pitch shift and time stretch on the device" (include/sedt_hip.h: sedt_stretch), one
function per stage so that the device can be checked stage by stage from what it produced itself - the end-to-end map is
ill-conditioned wherever a bin is nearly empty (its phase is arbitrary, yet it is accumulated into later frames).

Every stage takes ``dtype``: np.float64 is the reference, np.float32 the float32 restatement (below), and ``fault``: one of FAULTS
planted into the stage, for the tests of the tests.

The bounds.  eps = 2^-24 (float32's unit roundoff).  Each has the form the arithmetic gives; the constant in front is measured on the
device against this reference (largest error / bound with the constant at 1) and fixed at about four times that - DESIGN quotes both.
  stft      |D - D_ref| <= C_FFT eps log2(N) sum_i |x_i w_i| per frame: log2(N) butterfly levels, each rounding what it adds up
  vocoder   |S - S_ref| <= C_VOC mag (eps + (u + 1) 2^-52 (omega_k (u + 1) + 2 pi)): the rounding of S to float32 - the magnitude's own -
            and the angle error times the magnitude: magnitudes, angles and the phase are float64 on both sides, so the angle differs
            by the float64 rounding of a phase of size omega_k (u + 1) + 2 pi, once per step so far
  inverse   |z - z_ref| <= C_OLA eps log2(N) sum_u (2 / N) sum_k |S_u[k]| w[q - u hop] / ws[q]: the frames' FFT bounds over the
            window sum (without the quotient where ws <= WS_MIN)
  resample  |y - y_ref| <= C_RES eps sqrt(taps) sum_j |tap_j z_j|: the f32 sum of `taps` terms in ascending j, whose partial sums are
            each rounded - the roundings add up like a random walk, so the error grows with the square root of their number (33 taps
            for kaiser_fast upwards, 257 for kaiser_best an octave down); the table is rounded once for both sides, so its rounding
            is no difference - its f32 interpolation is, by a few eps of each tap

The float32 restatement keeps what the device keeps in float32 - samples, window, spectra, frames, the overlap-add, the filter taps
and their sum - and in float64 what the device computes in float64: the vocoder's magnitudes, angles and phase."""
import functools
import math

import numpy as np

EPS = 2.0 ** -24
WS_MIN = 1e-8
TABLE_RES = 512
QUALITIES = {'kaiser_best': (64, 0.9475937167399596, 14.769656459379492), 'kaiser_fast': (16, 0.85, 8.555504641634386)}
FAULTS = ('swap_a', 'no_wrap', 'omega_off', 'ws_plain', 'no_scale', 'nearest', 'round_step')
# measured on the MI355X with the constant at 1, the largest error / bound over the case table (tests/test_stretch_gpu.py prints the
# ratios): stft 0.196, vocoder 0.990, inverse 0.324, resample 1.093 - each fixed at about four times that (DESIGN.md quotes both)
C_FFT, C_VOC, C_OLA, C_RES = 0.8, 4.0, 1.3, 4.5


def lengths(n, f, p, N):
    """(m, m1, r, alpha, T, U); g == 1: r = 1, T = U = 0"""
    alpha = float(np.float64(2.0) ** (np.float64(p) / np.float64(12.0)))
    g = float(f) * alpha
    m, m1 = int(math.floor(n * float(f) + 0.5)), int(math.floor(n * g + 0.5))
    if g == 1.0:
        return m, n, 1.0, alpha, 0, 0
    r = 1.0 / g
    T = 1 + n // (N // 4)
    U = 0
    while U * r < T:                                       # the steps u with fl64(u r) < T
        U += 1
    return m, m1, r, alpha, T, U


def hann(N):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)


def frames_of(x, N, dtype=np.float64):
    """(T, N): the windowed frames, zero outside [0, n)"""
    hop, n = N // 4, len(x)
    T = 1 + n // hop
    pad = np.zeros(N // 2 + T * hop + N, dtype)
    pad[N // 2:N // 2 + n] = x
    w = hann(N).astype(dtype)
    return np.stack([pad[t * hop:t * hop + N] * w for t in range(T)])


def stft(x, N, dtype=np.float64):
    """D complex (T, K)"""
    return np.fft.rfft(frames_of(np.asarray(x, dtype), N, dtype), axis=1)


def stft_bound(x, N):
    """per frame (T,)"""
    return C_FFT * EPS * math.log2(N) * np.abs(frames_of(np.asarray(x, np.float64), N)).sum(axis=1)


def _arg(D, dtype):
    a = np.arctan2(D.imag.astype(dtype), D.real.astype(dtype))
    return np.where((D.real == 0) & (D.imag == 0), dtype(0), a).astype(dtype)


def vocoder(D, r, U, N, dtype=np.float64, fault=None):
    """(S complex (U, K), phi float64 (U, K), mag (U, K)) from D (T, K)"""
    T, K = D.shape
    hop = N // 4
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    Dz = np.concatenate([D.astype(ctype), np.zeros((2, K), ctype)])
    k = np.arange(K, dtype=np.float64)
    if fault == 'omega_off':
        k = k + 1.0
    omega = (2.0 * np.pi * hop * k) / N
    Dw = Dz.astype(np.complex128)                          # the spectrum is stored in ``dtype``; what follows is float64, as on the device
    mags, args = np.abs(Dw), _arg(Dw, np.float64)
    phi = args[0].astype(np.float64)
    S, P, Mg = np.zeros((U, K), ctype), np.zeros((U, K)), np.zeros((U, K))
    for u in range(U):
        s = np.float64(u) * np.float64(r)
        i = int(np.round(s)) if fault == 'round_step' else int(np.floor(s))
        a = s - np.floor(s)
        i = min(max(i, 0), T)
        wa, wb = (a, 1.0 - a) if fault == 'swap_a' else (1.0 - a, a)
        mag = wa * mags[i] + wb * mags[i + 1]
        S[u] = (mag * np.cos(phi) + 1j * (mag * np.sin(phi))).astype(ctype)
        P[u], Mg[u] = phi, mag
        d = (args[i + 1] - args[i]) - omega
        if fault != 'no_wrap':
            d = d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))
        phi = phi + (omega + d)
    return S, P, Mg


def vocoder_bound(mag, N):
    """(U, K) from the reference's magnitudes"""
    u = np.arange(mag.shape[0], dtype=np.float64)[:, None]
    omega = (2.0 * np.pi * (N // 4) * np.arange(mag.shape[1], dtype=np.float64)[None, :]) / N
    return C_VOC * mag * (EPS + (u + 1.0) * 2.0 ** -52 * (omega * (u + 1.0) + 2.0 * np.pi))


def window_sum(U, N, length, plain=False):
    hop, w = N // 4, hann(N)
    ws = np.zeros(max(length, (U - 1) * hop + N))
    for u in range(U):
        ws[u * hop:u * hop + N] += w if plain else w * w
    return ws


def istft(S, N, m1, dtype=np.float64, fault=None):
    """z (m1,) from S (U, K)"""
    U, hop = S.shape[0], N // 4
    S = S.copy()
    S[:, 0], S[:, -1] = S[:, 0].real, S[:, -1].real
    w = hann(N).astype(dtype)
    fr = np.fft.irfft(S, N, axis=1).astype(dtype) * w
    total = max(N // 2 + m1, (U - 1) * hop + N)
    acc = np.zeros(total, dtype)
    for u in range(U):                                     # ascending frame order per sample
        acc[u * hop:u * hop + N] += fr[u]
    ws = window_sum(U, N, total, plain=fault == 'ws_plain').astype(dtype)
    z = np.where(ws > dtype(WS_MIN), acc / np.where(ws > dtype(WS_MIN), ws, 1), acc)
    return z[N // 2:N // 2 + m1].astype(dtype)


def istft_bound(S, N, m1):
    U, hop = S.shape[0], N // 4
    w = hann(N)
    per = (2.0 / N) * np.abs(S).sum(axis=1)
    total = max(N // 2 + m1, (U - 1) * hop + N)
    acc = np.zeros(total)
    for u in range(U):
        acc[u * hop:u * hop + N] += per[u] * w
    ws = window_sum(U, N, total)
    b = np.where(ws > WS_MIN, acc / np.where(ws > WS_MIN, ws, 1.0), acc)
    return C_OLA * EPS * math.log2(N) * b[N // 2:N // 2 + m1]


def kaiser_sinc(u, Z, rolloff, beta):
    u = np.asarray(u, np.float64)
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (u / Z) ** 2, 0.0, None))) / np.i0(beta)
    return np.where(np.abs(u) <= Z, rolloff * np.sinc(rolloff * u) * win, 0.0)


@functools.lru_cache(maxsize=None)
def filter_table(quality):
    Z, rolloff, beta = QUALITIES[quality]
    return kaiser_sinc(np.arange(Z * TABLE_RES + 1, dtype=np.float64) / TABLE_RES, Z, rolloff, beta).astype(np.float32), Z


def _taps(i, alpha, m1, quality, dtype, fault):
    """for outputs i (block,): (j (block, taps) clipped, weights (block, taps) with 0 outside)"""
    tab, Z = filter_table(quality)
    tab = tab.astype(dtype)
    sd = 1.0 / alpha if alpha > 1.0 else 1.0
    t = i.astype(np.float64) * np.float64(alpha)
    half = Z / sd
    span = int(math.ceil(2 * half)) + 2
    j = np.ceil(t - half)[:, None] + np.arange(span, dtype=np.float64)[None, :]
    pos = np.abs(sd * (t[:, None] - j)) * TABLE_RES
    q = np.floor(pos)
    ok = (q < Z * TABLE_RES) & (j >= 0) & (j < m1) & (j <= np.floor(t + half)[:, None])
    qi = np.clip(q.astype(np.int64), 0, Z * TABLE_RES - 1)
    frac = (pos - q).astype(dtype)
    if fault == 'nearest':
        w = np.where(frac < 0.5, tab[qi], tab[qi + 1])
    else:
        w = tab[qi] + frac * (tab[qi + 1] - tab[qi])
    scale = dtype(1) if fault == 'no_scale' else dtype(sd)
    return np.clip(j, 0, max(m1 - 1, 0)).astype(np.int64), np.where(ok, scale * w, dtype(0)).astype(dtype)


def resample(z, alpha, m, quality='kaiser_best', dtype=np.float64, fault=None, bound=False):
    """y (m,) from z (m1,); with ``bound`` the resampler's bound (m,) instead"""
    z = np.asarray(z, dtype)
    m1 = len(z)
    if alpha == 1.0:
        return np.zeros(m) if bound else z[:m].copy()
    out = np.zeros(m, np.float64 if bound else dtype)
    if m1 == 0:
        return out
    for lo in range(0, m, 4096):
        i = np.arange(lo, min(lo + 4096, m))
        j, w = _taps(i, alpha, m1, quality, np.float64 if bound else dtype, fault)
        terms = w * z[j]
        if bound:
            out[i] = C_RES * EPS * np.sqrt((w != 0).sum(axis=1)) * np.abs(terms).sum(axis=1)
        elif dtype == np.float64:
            out[i] = terms.sum(axis=1)
        else:
            out[i] = np.cumsum(terms, axis=1, dtype=dtype)[:, -1]          # ascending j, every partial sum rounded
    return out


def chain(x, f, p, N, quality='kaiser_best', dtype=np.float64):
    """dict D, S, z, y of the whole definition from x"""
    n = len(x)
    m, m1, r, alpha, T, U = lengths(n, f, p, N)
    x = np.asarray(x, dtype)
    if T == 0:
        D = S = None
        z = x.copy()
    else:
        D = stft(x, N, dtype)
        S = vocoder(D, r, U, N, dtype)[0]
        z = istft(S, N, m1, dtype)
    return dict(D=D, S=S, z=z, y=resample(z, alpha, m, quality, dtype), m=m)
