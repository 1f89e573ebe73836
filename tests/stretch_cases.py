"""The case table of the stretch stage (tests/test_stretch_cpu.py asserts that every named edge is reached; tests/test_stretch_gpu.py runs
every stage of every row on the device).  A row is (n_fft, n, factor, semitones, content).

n covers one frame (n < hop), the frame-count steps (127 / 128 / 129, 255 / 257, 512) and excerpts shorter than half a window; the
factors 0.5 and 2.0 with p = 0 give r = 2 and r = 0.5, whose steps land on a frame every time or every second time, 0.8123 never does;
the shifts reach both ends of the envelope.  Content: 'noise' is seeded white noise plus a tone (broadband: the end-to-end check runs on
these rows), 'gap' a tone with a silent gap (nearly empty bins: stage parity only)."""
import functools

import numpy as np

import stretch_ref as R

ROWS = [
    (512, 1, 0.5, 0.0, 'noise'),            # T = 1, U = 1, one sample in, one out
    (512, 1, 2.0, 12.0, 'noise'),           # g = 4
    (512, 1, 0.5, -12.0, 'noise'),          # g = 1/4: m1 = 0, an empty z
    (512, 100, 0.8123, -3.0, 'noise'),
    (512, 127, 1.25, 3.0, 'noise'),
    (512, 128, 2.0, 0.0, 'noise'),          # r = 0.5; p = 0: no resampler
    (512, 129, 0.5, 12.0, 'noise'),         # g = 1, p != 0: no vocoder
    (512, 255, 0.5, 0.0, 'noise'),          # r = 2: T = 2, U = 1 ...
    (512, 257, 0.5, 0.0, 'noise'),          # ... T = 3, U = 2: either side of a step of U
    (512, 257, 1.0, 0.0, 'noise'),          # the identity through the stage: a copy
    (512, 512, 0.8123, -0.37, 'noise'),
    (512, 3000, 1.25, -12.0, 'noise'),
    (512, 3000, 2.0, 12.0, 'noise'),        # g = 4, the resampler's longest filter
    (512, 3000, 0.5, -12.0, 'noise'),       # g = 1/4
    (512, 3000, 2.0, -12.0, 'noise'),       # g = 1 again, alpha = 1/2
    (512, 3000, 1.25, 3.0, 'gap'),
    (512, 16000, 0.8123, 3.0, 'noise'),
    (512, 16000, 2.0, -0.37, 'noise'),
    (1024, 1300, 0.8123, 3.0, 'noise'),     # T = 6
    (2048, 2500, 1.25, -3.0, 'noise'),      # T = 5
]
LENGTHS = (1, 100, 127, 128, 129, 255, 257, 512, 3000, 16000)
FACTORS = (0.5, 0.8123, 1.25, 2.0)
SHIFTS = (-12.0, -3.0, -0.37, 0.0, 3.0, 12.0)
QUALITY = 'kaiser_fast'                     # the table that is staged in LDS; kaiser_best (read from memory) has rows of its own
BEST_ROWS = (4, 12)                         # rows run with kaiser_best as well


@functools.lru_cache(maxsize=None)
def signal(row):
    N, n, f, p, content = ROWS[row]
    gen = np.random.default_rng(1000 + row)
    t = np.arange(n, dtype=np.float64)
    if content == 'gap':
        x = 0.5 * np.sin(2.0 * np.pi * 40.0 * t / N)
        x[n // 3:2 * n // 3] = 0.0
    else:
        x = 0.1 * gen.standard_normal(n) + 0.3 * np.sin(2.0 * np.pi * 20.0 * t / N)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(row, quality=QUALITY):
    """the float64 chain from x, computed once and shared (read-only)"""
    N, n, f, p, _ = ROWS[row]
    out = R.chain(signal(row), f, p, N, quality, np.float64)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def edges():
    """the named edges -> the rows that reach them"""
    hit = {k: [] for k in ('one_frame', 'short', 'zero_frame', 'lands_always', 'lands_half', 'lands_never', 'g1_shifted', 'p0', 'empty_z',
                           'u_step', 'n1024', 'n2048', 'down', 'up')}
    for i, (N, n, f, p, _) in enumerate(ROWS):
        m, m1, r, alpha, T, U = R.lengths(n, f, p, N)
        if T == 1:
            hit['one_frame'].append(i)
        if n < N // 2:
            hit['short'].append(i)
        if T and int(np.floor((U - 1) * r)) + 1 >= T:
            hit['zero_frame'].append(i)
        if T and r == 2.0:
            hit['lands_always'].append(i)
        if T and r == 0.5:
            hit['lands_half'].append(i)
        if T and U > 2 and all((u * r) % 1.0 != 0.0 for u in range(1, U)):
            hit['lands_never'].append(i)
        if T == 0 and p != 0.0:
            hit['g1_shifted'].append(i)
        if p == 0.0:
            hit['p0'].append(i)
        if m1 == 0:
            hit['empty_z'].append(i)
        if N == 1024 and T <= 6:
            hit['n1024'].append(i)
        if N == 2048 and T <= 6:
            hit['n2048'].append(i)
        if alpha > 1.0:
            hit['down'].append(i)                          # s < 1: the filter is widened
        if alpha < 1.0:
            hit['up'].append(i)
        for j, (N2, n2, f2, p2, _) in enumerate(ROWS):
            o = R.lengths(n2, f2, p2, N2)
            if T and N2 == N and o[2] == r and o[4] == T + 1 and o[5] == U + 1:
                hit['u_step'].append((i, j))
    return hit
