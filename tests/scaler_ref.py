"""A NumPy restatement of the dataset Scaler's fit as include/sedt_hip.h states it for sedt_scaler_update (written from that
description, not from the reference's text), and the summation bound the scaler tests share.

Per clip: the features v are f32 - the raw values themselves, or 10 log10(max(1e-10, x^2)) clamped from below at (maximum over ALL raw
rows) - 80.  Rows >= min(rows of the clip, frames) are zero padding: they add nothing and count in the divisor.  Band c gets two
float64 numbers: sum(v) / frames and sum(fl32(v * v)) / frames, each sum taken in the kernel's order (G = 1024 // F interleaved
partials over the rows, then the partials in index order).  The data set: the per-clip numbers added clip by clip, divided by the
number of clips at the end; std = sqrt(mean_of_square - mean ** 2)."""
import numpy as np

U = 2.0 ** -53                     # unit roundoff of float64


def features(clip, frames, apply_log):
    """the kept real rows of one clip as f32 features (keep x F)"""
    x = np.asarray(clip, np.float32)
    keep = min(len(x), frames)
    if not apply_log:
        return x[:keep]
    db = np.float32(10) * np.log10(np.maximum(np.float32(1e-10), x * x))
    return np.maximum(db[:keep], db.max() - np.float32(80)).astype(np.float32)


def clip_stats(v, frames):
    """v (keep x F) f32 -> [2][F] float64: the band means of v and of its f32 squares over `frames` rows, in the kernel's order"""
    keep, F = v.shape
    G = 1024 // F
    sq = (v * v).astype(np.float32)
    out = np.zeros((2, F), np.float64)
    for k, a in enumerate((v, sq)):
        part = np.zeros((G, F), np.float64)
        for r in range(keep):
            part[r % G] += a[r].astype(np.float64)
        s = np.zeros(F, np.float64)
        for g in range(G):
            s = s + part[g]
        out[k] = s / frames
    return out


def fit(clips, frames, apply_log=False):
    """(sums [2][F], count) over the clips in their order"""
    acc = None
    for c in clips:
        st = clip_stats(features(c, frames, apply_log), frames)
        acc = st if acc is None else acc + st
    return acc, len(clips)


def finish(sums, count):
    mean, mos = sums[0] / count, sums[1] / count
    return mean, mos, np.sqrt(mos - mean ** 2)


FACTOR = 2.0


def summation_bounds(feats, frames):
    """per band, how far two correct fits of the same features may lie apart.  Both compute
        (1 / B) sum_b [(1 / frames) sum_r x_{b,r}]
    in float64 with sums in some order.  A recursive sum of n terms in any order is within (n - 1) u sum|x_i| of the exact one (to first
    order in u = 2^-53), so two orders differ by at most 2 (n - 1) u sum|x_i|.  A term passes through at most (frames - 1) additions
    inside its clip and (B - 1) across the clips: n = frames + B stands for the whole chain, applied to the mean of |x|.  The two
    divisions add one rounding each, and terms of second order exist: FACTOR = 2 over the bound covers both (a constant <= 4, stated
    here and nowhere tuned).  feats: per clip the (keep x F) f32 features.  Returns (bound for mean_, bound for mean_of_square_)."""
    B = len(feats)
    a1 = sum(np.abs(v.astype(np.float64)).sum(0) for v in feats) / (frames * B)
    a2 = sum((v * v).astype(np.float32).astype(np.float64).sum(0) for v in feats) / (frames * B)
    n = frames + B
    return FACTOR * 2 * (n - 1) * U * a1, FACTOR * 2 * (n - 1) * U * a2
