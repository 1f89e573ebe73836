"""The case table of the reverb stage (tests/test_reverb_cpu.py asserts that every named edge is reached and that the float64 partitioned
chain equals the direct form on every row; tests/test_reverb_gpu.py runs every stage of every row on the device).  A row is
(n_fft, n, L, fade, content, rir kind).

At n_fft 512 (Bs = 256): n covers one sample, either side of a block (255 / 256 / 257), a few blocks (600) and a dozen (3000, more
than one workgroup of the product launch); L covers one tap, two, either side of one partition (255 / 256 / 257), either side of two
(513) and a partly filled third (700); n + L - 1 lands on a multiple of Bs (600 + 169 - 1 = 768) and one past it; one response is as
long as the envelope allows (176 partitions); one fade is longer than half the sound.  RIR kinds: 'unit' an impulse at lag 0 (wet = dry
under its fade, then L - 1 zeros), 'lag' an impulse at lag L - 1 (wet = the dry sound shifted), 'noise' seeded noise under an
exponential decay.  Content: 'noise' seeded white noise plus a tone, 'tone' the tone alone."""
import functools

import numpy as np

import reverb_ref as R

MAX_PART = 176

ROWS = [
    (512, 1, 1, 0, 'noise', 'unit'),            # one sample through one tap
    (512, 1, 2, 0, 'noise', 'noise'),
    (512, 1, 700, 0, 'noise', 'noise'),          # the tail is all there is
    (512, 255, 1, 8, 'noise', 'unit'),           # wet = faded dry
    (512, 255, 255, 8, 'noise', 'noise'),
    (512, 255, 257, 0, 'noise', 'lag'),
    (512, 256, 2, 0, 'noise', 'noise'),
    (512, 256, 256, 16, 'noise', 'noise'),       # one full block through one full partition
    (512, 256, 513, 16, 'tone', 'noise'),
    (512, 257, 255, 0, 'noise', 'noise'),
    (512, 257, 256, 0, 'noise', 'lag'),          # the impulse in the last tap of a full partition
    (512, 257, 257, 30, 'noise', 'noise'),       # one tap in the second partition
    (512, 600, 1, 0, 'tone', 'unit'),
    (512, 600, 169, 16, 'noise', 'noise'),       # n + L - 1 = 768 = 3 Bs
    (512, 600, 170, 16, 'noise', 'noise'),       # ... and 769
    (512, 600, 513, 400, 'noise', 'noise'),      # a fade longer than n / 2
    (512, 600, 700, 16, 'noise', 'lag'),         # wet = dry shifted by 699
    (512, 600, MAX_PART * 256, 16, 'noise', 'noise'),     # the longest response of the envelope: 176 partitions
    (512, 3000, 2, 160, 'noise', 'noise'),
    (512, 3000, 256, 160, 'noise', 'noise'),
    (512, 3000, 257, 160, 'tone', 'noise'),
    (512, 3000, 513, 160, 'noise', 'lag'),
    (512, 3000, 700, 160, 'noise', 'noise'),
    (1024, 3000, 1300, 16, 'noise', 'noise'),    # 3 partitions, 7 input blocks
    (2048, 5000, 2500, 32, 'noise', 'noise'),    # 3 partitions, 6 input blocks
]
LENGTHS = (1, 255, 256, 257, 600, 3000)
TAPS = (1, 2, 255, 256, 257, 513, 700)


@functools.lru_cache(maxsize=None)
def signal(row):
    N, n, L, fade, content, kind = ROWS[row]
    gen = np.random.default_rng(2000 + row)
    t = np.arange(n, dtype=np.float64)
    x = 0.3 * np.sin(2.0 * np.pi * 20.0 * t / N + 0.3)
    if content == 'noise':
        x = x + 0.1 * gen.standard_normal(n)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def response(row):
    """the row's response, float32, as it is staged (normalize=None)"""
    N, n, L, fade, content, kind = ROWS[row]
    gen = np.random.default_rng(3000 + row)
    h = np.zeros(L, np.float64)
    if kind == 'unit':
        h[0] = 1.0
    elif kind == 'lag':
        h[L - 1] = 1.0
    else:
        h = gen.standard_normal(L) * np.exp(-6.0 * np.arange(L, dtype=np.float64) / L)
        h = h / np.sqrt(np.sum(h * h))
    h = h.astype(np.float32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def reference(row):
    """the float64 partitioned chain (H, X, wet) and the direct form, computed once and shared (read-only)"""
    N, n, L, fade, _, _ = ROWS[row]
    out = R.chain(signal(row), response(row), fade, N, np.float64)
    out['direct'] = R.direct(signal(row), response(row), fade)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restatement(row):
    """the float32 restatement's wet row (read-only)"""
    N, n, L, fade, _, _ = ROWS[row]
    wet = R.chain(signal(row), response(row), fade, N, np.float32)['wet']
    wet.setflags(write=False)
    return wet


def edges():
    """the named edges -> the rows that reach them"""
    hit = {k: [] for k in ('single_partition', 'last_partition_partial', 'zero_history', 'input_shorter_than_block',
                           'tail_longer_than_head', 'total_on_block', 'total_past_block', 'max_partitions', 'long_fade', 'n1024',
                           'n2048', 'unit', 'lag', 'noise')}
    for i, (N, n, L, fade, _, kind) in enumerate(ROWS):
        Bs = N // 2
        nb, P, nout, total = R.counts(n, L, N)
        if P == 1:
            hit['single_partition'].append(i)
        if L % Bs:
            hit['last_partition_partial'].append(i)
        if P > 1:
            hit['zero_history'].append(i)                  # output block 0 asks partition 1 for X[-1]: j < p
        if n < Bs:
            hit['input_shorter_than_block'].append(i)
        if L - 1 > n:
            hit['tail_longer_than_head'].append(i)
        if total % Bs == 0:
            hit['total_on_block'].append(i)
        if total % Bs == 1:
            hit['total_past_block'].append(i)
        if P == MAX_PART:
            hit['max_partitions'].append(i)
        if 2 * fade > n:
            hit['long_fade'].append(i)
        if N == 1024:
            hit['n1024'].append(i)
        if N == 2048:
            hit['n2048'].append(i)
        hit[kind].append(i)
    return hit
