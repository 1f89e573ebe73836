"""The designed inputs of the loudness tests, shared by tests/test_loudness_cpu.py (which checks on the float64 reference alone that no
block lies at a gate threshold, so that the counts can be compared exactly) and tests/test_loudness_gpu.py (which runs them on the
device).  A case is (sample rate, number of sources); its sources lie back to back in one flat vector, so most start at addresses
that are no multiple of 16 bytes.

Lengths (H = the 100 ms hop: 1600, 2205, 4800 samples): 1, H - 1, 4H - 1 (short), 4H (one block), 4H + 1, 5H - 1, 5H, and 23H + 7 (20
blocks, enough for both gates to act); at 16 kHz also 259H + 3 and 260H, which cross the boundary of a round of 256 hops.
Contents: 'steps' - seeded noise at 0.1 for a fifth of the source, 30 dB less for three fifths (over the absolute gate, under the
relative one), 1e-5 for the rest (under the absolute gate); 'noise' - seeded noise at 0.05; 'zero'; 'quiet' - noise at 1e-5, wholly under
the absolute gate; 'dc' - noise at 0.05 on an offset of 0.5."""
import functools

import numpy as np

import loudness_ref as R

RATES = (16000, 22050, 48000)
N_SRC = (1, 3, 70)
CASES = [(sr, n) for sr in RATES for n in N_SRC]
CONTENTS = ('steps', 'noise', 'zero', 'quiet', 'dc')
SEED = 7


def lengths(sr):
    H = R.hop_samples(sr)
    out = [1, H - 1, 4 * H - 1, 4 * H, 4 * H + 1, 5 * H - 1, 5 * H, 23 * H + 7]
    return out + ([259 * H + 3, 260 * H] if sr == 16000 else [])


def content(kind, n, gen):
    x = gen.standard_normal(n)
    if kind == 'steps':
        a, b = n // 5, n - n // 5
        x[:a] *= 0.1
        x[a:b] *= 0.1 * 10.0 ** (-30.0 / 20.0)
        x[b:] *= 1e-5
    elif kind == 'noise':
        x *= 0.05
    elif kind == 'zero':
        x *= 0.0
    elif kind == 'quiet':
        x *= 1e-5
    elif kind == 'dc':
        x = 0.5 + 0.05 * x
    return x.astype(np.float32)


def plan(sr, n_src):
    """[(length, content)] of a case: one source - the longest with steps; three - the two round-crossing lengths (16 kHz) or the two
    longest, and a short one; seventy - every length with every content, and so on round"""
    ls = lengths(sr)
    if n_src == 1:
        return [(ls[-1], 'steps')]
    if n_src == 3:
        return [(ls[-2], 'dc'), (ls[2], 'noise'), (ls[-1], 'steps')]
    short = [n for n in ls if n <= 23 * R.hop_samples(sr) + 7]         # (the round-crossing ones are in the cases of 1 and 3)
    pairs = [(n, k) for k in CONTENTS for n in short]
    return [pairs[i % len(pairs)] for i in range(n_src)]


@functools.lru_cache(maxsize=None)
def sources(sr, n_src):
    gen = np.random.default_rng(SEED + sr + n_src)
    return tuple(content(k, n, gen) for n, k in plan(sr, n_src))


@functools.lru_cache(maxsize=None)
def reference(sr, n_src):
    """the float64 reference of every source of a case, computed once and shared"""
    return tuple(R.measure(x, sr) for x in sources(sr, n_src))
