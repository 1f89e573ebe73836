"""The designed inputs of the relevel tests, shared by tests/test_relevel_cpu.py (which checks on the float64 reference alone that no
block lies at a gate threshold, so that the counts can be compared exactly) and tests/test_relevel_gpu.py (which runs them on the
device).  All at 16 kHz (H = 1600).  A case is a number of jobs; its regions lie in one flat vector with gaps of 0.5 between them -
a read outside a region would move its level - and start at offsets that go round 0, 1, 2, 3 mod 4.

Lengths: 1, 255, 256, 257 (the edges of the RMS mode's 256 threads), H - 1, H, 4H - 1 (short), 4H (one block), 4H + 1, 6H + 3, and
257H + 3 - a second round of 256 hops, so the filter state is carried from one round into the next.
Contents: loudness_cases.CONTENTS - stepped noise, noise, zeros, noise under the absolute gate, noise on a DC offset.
Jobs: 1 - the longest with steps; 3 - the longest with steps, a short one, 6H + 3 on a DC offset; 270 (more than one workgroup's worth
of threads, and more workgroups than the chip has compute units) - every shorter length with every content, and so on round."""
import functools

import numpy as np

import loudness_cases as LC
import relevel_ref as R

SR, H = 16000, 1600
LENGTHS = (1, 255, 256, 257, H - 1, H, 4 * H - 1, 4 * H, 4 * H + 1, 6 * H + 3, 257 * H + 3)
N_JOBS = (1, 3, 270)
CONTENTS = LC.CONTENTS
SEED = 23
GAP = np.float32(0.5)


def plan(n_jobs):
    """[(length, content, offset mod 4)] of a case"""
    if n_jobs == 1:
        return [(LENGTHS[-1], 'steps', 1)]
    if n_jobs == 3:
        return [(LENGTHS[-1], 'steps', 3), (LENGTHS[6], 'noise', 2), (LENGTHS[9], 'dc', 1)]
    pairs = [(n, k) for k in CONTENTS for n in LENGTHS[:-1]]
    return [pairs[i % len(pairs)] + ((i + i // len(pairs)) % 4,) for i in range(n_jobs)]


def target_db(i):
    """the level job i shall have, in dB / LUFS"""
    return -36.0 + 2.5 * (i % 7)


@functools.lru_cache(maxsize=None)
def layout(n_jobs):
    """(flat float32, offsets int64 [E], lengths int64 [E]) of a case"""
    gen = np.random.default_rng(SEED + n_jobs)
    parts, offs, pos = [], [], 0
    for n, kind, res in plan(n_jobs):
        gap = 5 + (res - (pos + 5)) % 4                             # at least five samples of 0.5 in front of every region
        parts += [np.full(gap, GAP), LC.content(kind, n, gen)]
        offs.append(pos + gap)
        pos += gap + n
    parts.append(np.full(7, GAP))
    flat = np.concatenate(parts).astype(np.float32)
    flat.setflags(write=False)
    return flat, np.asarray(offs, np.int64), np.asarray([n for n, _, _ in plan(n_jobs)], np.int64)


def regions(n_jobs):
    flat, offs, ns = layout(n_jobs)
    return [flat[o:o + n] for o, n in zip(offs, ns)]


@functools.lru_cache(maxsize=None)
def reference(n_jobs, mode):
    """the float64 reference of every job of a case (relevel_ref.relevel), computed once and shared"""
    targets = [R.target_amplitude(target_db(i), mode) for i in range(n_jobs)]
    return tuple(R.relevel(regions(n_jobs), targets, SR, mode))
