"""The float64 restatement of "Reverberation on the device" (include/sedt_hip.h: sedt_reverb, sedt_reverb_spectra,
sedt_reverb_bed), one function per stage so that the device can be checked stage by stage from what it produced itself, and -
independently of any FFT - the direct form np.convolve(fade(x), h).

N = n_fft, Bs = N / 2, K = N / 2 + 1.  A response h of L taps is P = ceil(L / Bs) partitions, H[p] = rfft(h[p Bs, (p + 1) Bs) | Bs zeros).
Input block j, 0 <= j < nb = ceil(n / Bs) + 1, is x[(j - 1) Bs, (j + 1) Bs) with zeros outside [0, n), x already faded; X[j] = its
rfft.  Output block j, 0 <= j < ceil((n + L - 1) / Bs): Y = sum over p ascending of X[j - p] H[p] (X[i] = 0 outside 0 .. nb - 1), the
inverse real FFT, its LAST Bs samples are wet[j Bs, (j + 1) Bs), clipped to n + L - 1.

Every stage takes ``dtype``: np.float64 is the reference, np.float32 the float32 restatement - samples, fades, spectra, products, sums
AND the transforms in float32 (``fft32``: a radix-2 Stockham FFT in complex64, twiddles float64 rounded once), as the device keeps
them.  ``mac_inverse`` takes ``fault``: one of FAULTS planted into the stage, for the tests of the tests.

The bounds.  eps = 2^-24 (float32's unit roundoff).  Each has the form the arithmetic gives; the constant in front is measured on the
device against this reference (largest error / bound with the constant at 1) and fixed at about four times that - DESIGN quotes both.
  spectra   |H - H_ref| <= C_H eps log2(N) sum_i |h_i| per partition: log2(N) butterfly levels, each rounding what it adds up
  blocks    |X - X_ref| <= C_X eps log2(N) sum_i |x_i w_i| per block: the same, the fade's one product included
  wet       |y - y_ref| <= C_Y eps (log2(N) + sqrt(P)) (2 / N) sum_k sum_p |X[j - p][k]| |H[p][k]| per output block: the P products of
            a bin are summed in ascending p with every partial sum rounded - a random walk, sqrt(P) - and the inverse transform's
            log2(N) levels round what they add up; (2 / N) sum_k is the weight of the bins in a sample of the frame"""
import math

import numpy as np

EPS = 2.0 ** -24
FAULTS = ('drop_last_partition', 'first_half', 'shift_x')
# measured on the MI355X with the constant at 1, the largest error / bound over the case table (tests/test_reverb_gpu.py prints the
# ratios): spectra 0.382, blocks 0.181, wet 0.271 - each fixed at about four times that (DESIGN.md quotes both)
C_H, C_X, C_Y = 1.5, 0.75, 1.1


def counts(n, L, N):
    """(nb input blocks, P partitions, output blocks, n + L - 1)"""
    Bs = N // 2
    return -(-n // Bs) + 1, -(-L // Bs), -(-(n + L - 1) // Bs), n + L - 1


def fade_weight(n, fade):
    """float32 [n]: the ramp of sedt_soundscape over n samples (float64 divisions rounded to float32, 1 outside the ramps)"""
    i = np.arange(n, dtype=np.int64)
    fade = max(int(fade), 0)
    w_in = np.where(i < fade, ((i + 1).astype(np.float64) / np.float64(fade + 1)).astype(np.float32), np.float32(1.0))
    w_out = np.where(n - 1 - i < fade, ((n - i).astype(np.float64) / np.float64(fade + 1)).astype(np.float32), np.float32(1.0))
    return np.minimum(w_in, w_out).astype(np.float32)


def faded(x, fade, dtype=np.float64):
    """x w in ``dtype`` (float32: one rounded product per sample, as the device's loader)"""
    x = np.asarray(x, np.float32)
    return (x.astype(dtype) * fade_weight(len(x), fade).astype(dtype)).astype(dtype)


# ---------------------------------------------------------------------------------------------------- transforms
def fft32(a):
    """the forward FFT over the last axis in complex64: radix-2 Stockham stages, every product and sum rounded to float32"""
    x = np.asarray(a, np.complex64)
    N = x.shape[-1]
    tw = np.exp(-2j * np.pi * np.arange(max(N // 2, 1), dtype=np.float64) / N).astype(np.complex64)
    j = np.arange(N // 2)
    Ns = 1
    while Ns < N:
        k = j % Ns
        w = tw[k * (N // (2 * Ns))]
        u0, u1 = x[..., :N // 2], (x[..., N // 2:] * w).astype(np.complex64)
        y = np.empty_like(x)
        j0 = (j - k) * 2 + k
        y[..., j0], y[..., j0 + Ns] = u0 + u1, u0 - u1
        x, Ns = y, Ns * 2
    return x


def rfft(v, dtype=np.float64):
    """bins 0 .. N/2 of real frames (.., N)"""
    N = v.shape[-1]
    if dtype == np.float64:
        return np.fft.rfft(np.asarray(v, np.float64), axis=-1)
    return fft32(np.asarray(v, np.float32).astype(np.complex64))[..., :N // 2 + 1]


def irfft(Y, N, dtype=np.float64):
    """real frames (.., N) from bins 0 .. N/2; the imaginary parts of bins 0 and N/2 are dropped"""
    Y = np.array(Y, np.complex128 if dtype == np.float64 else np.complex64)
    Y[..., 0], Y[..., -1] = Y[..., 0].real, Y[..., -1].real
    if dtype == np.float64:
        return np.fft.irfft(Y, N, axis=-1)
    full = np.concatenate([Y, np.conj(Y[..., -2:0:-1])], axis=-1)
    return (np.conj(fft32(np.conj(full))).real.astype(np.float32) * np.float32(1.0 / N)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the stages
def _frames_h(h, N):
    Bs, L = N // 2, len(h)
    P = -(-L // Bs)
    fr = np.zeros((P, N), np.asarray(h).dtype)
    pad = np.zeros(P * Bs, fr.dtype)
    pad[:L] = h
    fr[:, :Bs] = pad.reshape(P, Bs)
    return fr


def partition_spectra(h, N, dtype=np.float64):
    """H complex (P, K)"""
    H = rfft(_frames_h(np.asarray(h, dtype), N), dtype)
    return H if dtype == np.float64 else H.astype(np.complex64)


def spectra_bound(h, N):
    """per partition (P,)"""
    return C_H * EPS * math.log2(N) * np.abs(_frames_h(np.asarray(h, np.float64), N)).sum(axis=1)


def _frames_x(xf, N):
    Bs, n = N // 2, len(xf)
    nb = -(-n // Bs) + 1
    pad = np.zeros((nb + 1) * Bs, xf.dtype)
    pad[Bs:Bs + n] = xf
    return np.stack([pad[j * Bs:j * Bs + N] for j in range(nb)])


def block_spectra(x, fade, N, dtype=np.float64):
    """X complex (nb, K) of the dry sound x (float32) under its fade"""
    X = rfft(_frames_x(faded(x, fade, dtype), N), dtype)
    return X if dtype == np.float64 else X.astype(np.complex64)


def blocks_bound(x, fade, N):
    """per block (nb,)"""
    return C_X * EPS * math.log2(N) * np.abs(_frames_x(faded(x, fade), N)).sum(axis=1)


def mac_inverse(X, H, n, L, N, dtype=np.float64, fault=None):
    """wet (n + L - 1,) from given X (nb, K) and H (P, K)"""
    Bs = N // 2
    nb, P, nout, total = counts(n, L, N)
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    X, H = np.asarray(X).astype(ctype), np.asarray(H).astype(ctype)
    assert X.shape == (nb, N // 2 + 1) and H.shape == (P, N // 2 + 1)
    out = np.zeros(nout * Bs, dtype)
    for j in range(nout):
        acc = np.zeros(N // 2 + 1, ctype)
        for p in range(P - 1 if fault == 'drop_last_partition' else P):       # ascending p
            i = j - p - (1 if fault == 'shift_x' else 0)
            if 0 <= i < nb:
                acc = (acc + (X[i] * H[p]).astype(ctype)).astype(ctype)
        frame = irfft(acc, N, dtype)
        out[j * Bs:(j + 1) * Bs] = frame[:Bs] if fault == 'first_half' else frame[Bs:]
    return out[:total]


def wet_bound(X, H, n, L, N):
    """per sample (n + L - 1,), from the spectra the stage was fed"""
    Bs = N // 2
    nb, P, nout, total = counts(n, L, N)
    aX, aH = np.abs(np.asarray(X, np.complex128)), np.abs(np.asarray(H, np.complex128))
    per = np.zeros(nout)
    for j in range(nout):
        for p in range(P):
            if 0 <= j - p < nb:
                per[j] += (2.0 / N) * float(np.sum(aX[j - p] * aH[p]))
    return (C_Y * EPS * (math.log2(N) + math.sqrt(P)) * np.repeat(per, Bs))[:total]


def chain(x, h, fade, N, dtype=np.float64, fault=None):
    """dict H, X, wet of the whole partitioned definition"""
    H, X = partition_spectra(h, N, dtype), block_spectra(x, fade, N, dtype)
    return dict(H=H, X=X, wet=mac_inverse(X, H, len(x), len(h), N, dtype, fault))


def direct(x, h, fade):
    """the direct form in float64: np.convolve(fade(x), h), n + L - 1 samples - no FFT anywhere"""
    return np.convolve(faded(x, fade), np.asarray(h, np.float64))


# ---------------------------------------------------------------------------------------------------- soundscapes
def split(wet, m):
    """(head, tail): the first m samples of a wet row go to the mixing call as the event, the last L - 1 into the clip's bed"""
    return wet[:m], wet[m:]


def bed(window, background, start, g_bg, tails):
    """float32 [window], every operation rounded on its own: g_bg * bg[(start + t) mod len] (0 with background None); then for every
    (gain, wet row, onset, m) of ``tails`` in order, where m <= t - onset < len(wet): bed = bed + (gain * wet[t - onset])"""
    t = np.arange(window, dtype=np.int64)
    acc = np.zeros(window, np.float32)
    if background is not None:
        acc = (np.float32(g_bg) * np.asarray(background, np.float32)[(int(start) + t) % len(background)]).astype(np.float32)
    for gain, wet, onset, m in tails:
        lo, hi = int(onset) + int(m), min(int(onset) + len(wet), window)
        if hi > lo:
            term = (np.float32(gain) * np.asarray(wet, np.float32)[lo - int(onset):hi - int(onset)]).astype(np.float32)
            acc[lo:hi] = (acc[lo:hi] + term).astype(np.float32)
    return acc
