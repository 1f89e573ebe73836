"""ITU-R BS.1770-4 programme loudness of ONE channel (channel weight 1) restated in float64 - the reference of sedt_loudness
(csrc/loudness.hip) and utilities/loudness.py.  It claims parity with no package; DESIGN.md section 4, "Loudness (BS.1770) on the
device", holds the definition.  The filter runs SERIALLY over the whole source (scipy.signal.lfilter when it imports - transposed direct
form II from zero state, which is the definition - else the same recurrence as a plain loop); ``hop_map`` restates the state map that
lets the device filter the hops in parallel."""
import math

import numpy as np

try:
    from scipy.signal import lfilter
except ImportError:                                                 # no hard dependency: the same recurrence as a loop
    lfilter = None

Z_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)


def hop_samples(sr):
    return (int(sr) + 5) // 10


def stage(fs, f0, Q, shelf_db=None):
    """(b [3], a [3]) of one stage at sample rate fs: a shelf of shelf_db, or with None the high-pass"""
    K = math.tan(math.pi * f0 / float(fs))
    a0 = 1.0 + K / Q + K * K
    if shelf_db is None:
        b = [1.0, -2.0, 1.0]
    else:
        Vh = 10.0 ** (shelf_db / 20.0)
        Vb = Vh ** 0.4996667741545416
        b = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    return np.asarray(b, np.float64), np.asarray([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)


def k_weighting(sr):
    """[(b, a) of the shelf stage, (b, a) of the high-pass stage]"""
    return [stage(sr, 1681.974450955533, 0.7071752369554196, 3.999843853973347), stage(sr, 38.13547087602444, 0.5003270373238773)]


def biquad(b, a, x, state=(0.0, 0.0)):
    """transposed direct form II as a loop: (y, the state afterwards)"""
    s0, s1 = float(state[0]), float(state[1])
    b0, b1, b2, a1, a2 = float(b[0]), float(b[1]), float(b[2]), float(a[1]), float(a[2])
    y = np.empty(len(x), np.float64)
    for i, v in enumerate(np.asarray(x, np.float64).tolist()):
        o = b0 * v + s0
        s0 = b1 * v - a1 * o + s1
        s1 = b2 * v - a2 * o
        y[i] = o
    return y, (s0, s1)


def k_filter(x, sr):
    """the K-weighted signal in float64 from zero state: the shelf first, then the high-pass"""
    y = np.asarray(x, np.float32).astype(np.float64)
    for b, a in k_weighting(sr):
        y = lfilter(b, a, y) if lfilter is not None and len(y) else biquad(b, a, y)[0]
    return y


def hop_map(sr):
    """(4, 4) float64: the state of the cascade (shelf s0 s1, high-pass s0 s1) after H zero-input samples, column k from unit state k"""
    (b1, a1), (b2, a2) = k_weighting(sr)
    zeros = np.zeros(hop_samples(sr), np.float64)
    M = np.zeros((4, 4), np.float64)
    for k in range(4):
        unit = [0.0] * 4
        unit[k] = 1.0
        y, s_a = biquad(b1, a1, zeros, unit[:2])
        _, s_b = biquad(b2, a2, y, unit[2:])
        M[:, k] = s_a + s_b
    return M


def blocks(x, sr):
    """(z float64 [J], short): the mean squares of the 400 ms blocks with 75 % overlap; a source shorter than one block (no block in the
    standard) is ONE block over all its samples"""
    H, n = hop_samples(sr), len(x)
    y = k_filter(x, sr)
    if n < 4 * H:
        return np.asarray([np.sum(y * y) / n if n else 0.0], np.float64), True
    e = np.asarray([np.sum(y[h * H:(h + 1) * H] ** 2) for h in range(n // H)], np.float64)
    return (((e[:-3] + e[1:-2]) + e[2:-1]) + e[3:]) / np.float64(4 * H), False


def gates(z):
    """(zbar, n_abs, n_rel, the relative threshold) from the blocks' mean squares"""
    over = z > Z_ABS
    n_abs = int(over.sum())
    thr = 0.1 * (z[over].sum() / n_abs) if n_abs else 0.0
    both = over & (z > thr)
    n_rel = int(both.sum())
    return (float(z[both].sum() / n_rel) if n_rel else 0.0), n_abs, n_rel, thr


def lufs(zbar):
    return -0.691 + 10.0 * math.log10(zbar) if zbar > 0 else -math.inf


def measure(x, sr):
    """dict(zbar, lufs, J, n_abs, n_rel, short, z, thr) of one source"""
    z, short = blocks(x, sr)
    zbar, n_abs, n_rel, thr = gates(z)
    return dict(zbar=zbar, lufs=lufs(zbar), J=len(z), n_abs=n_abs, n_rel=n_rel, short=short, z=z, thr=thr)


def gate_clearance(z, thr):
    """the smallest relative distance of a block's z to either gate threshold (inf without blocks that could be compared)"""
    d = np.abs(z - Z_ABS) / Z_ABS
    if thr > 0:
        d = np.minimum(d, np.abs(z - thr) / thr)
    return float(d.min()) if len(d) else math.inf
