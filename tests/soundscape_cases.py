"""The designed inputs of the soundscape tests: one small bank and hand-made clips, shared by tests/test_soundscape_cpu.py (which checks on
the NumPy reference alone that they contain what they are there for) and tests/test_soundscape_gpu.py (which runs them on the device).

Bank: five sounds of 1, 3, 700, 5000 and 20000 samples (classes 0 .. 4) and two background recordings of 700 and 20000 samples.
An event record is (src, cls, src_start, n, onset, gain, fade); a background (src, start, gain) or None."""
import numpy as np

import soundscape_ref as S

SR = 16000
LABELS = [f'c{i}' for i in range(10)]
EVENT_LENS = [1, 3, 700, 5000, 20000]
BG_LENS = [700, 20000]
N_SRC = len(EVENT_LENS) + len(BG_LENS)
WINDOWS = (1003, 4096)


def bank():
    """(sounds, their classes, backgrounds): float32 arrays from one seed; sounds 0 and 1 are hand-made so that a product is exact"""
    gen = np.random.default_rng(11)
    sounds = [np.asarray([0.5], np.float32), np.asarray([0.25, -0.5, 0.125], np.float32)]
    sounds += [(0.1 * gen.standard_normal(n)).astype(np.float32) for n in EVENT_LENS[2:]]
    backgrounds = [(0.05 * gen.standard_normal(n)).astype(np.float32) for n in BG_LENS]
    return sounds, list(range(len(sounds))), backgrounds


def clips(W):
    """the designed clips at a window of W samples: [(background, [events])]"""
    return [
        # 0: a 700-sample background from its last sample on; onsets 0, 1, 2, 3; an event nested in another of its class (collapse
        #    removes one); another class at the same time; fade 160, fade 0, and fade 40 > n / 2 = 25 (the ramps overlap)
        ((5, 699, 0.5), [(2, 1, 0, 700, 0, 1.0, 160), (2, 1, 100, 300, 1, 0.5, 0), (3, 2, 17, 900, 2, 0.3, 160),
                         (4, 3, 1001, 50, 3, 0.7, 40)]),
        # 1: nothing at all, between clips with events
        (None, []),
        # 2: n = 1, ending exactly at the window: 2 * 0.5 is the peak limit itself - scale 1
        (None, [(0, 0, 0, 1, W - 1, 2.0, 0)]),
        # 3: an event that runs past the window and one of its class that ends where it starts (touching: merged); onsets 2047 and 2048,
        #    overlapping (merged at 4096; behind the window at 1003)
        ((6, 12345, 0.8), [(4, 4, 5000, 3000, W - 500, 0.4, 160), (3, 4, 0, 100, W - 600, 0.4, 10), (1, 5, 0, 3, 2047, 1.0, 0),
                           (1, 5, 0, 3, 2048, 1.0, 1)]),
        # 4: a 3-sample background (it wraps hundreds of times); a chain of three events of one class (one target), another class across
        ((1, 2, 0.25), [(2, 6, 0, 300, 10, 0.5, 0), (2, 6, 100, 300, 200, 0.5, 5), (2, 6, 0, 300, 450, 0.5, 160),
                        (3, 7, 0, 700, 100, 0.2, 0)]),
        # 5: loud: the peak exceeds the limit and the clip is scaled
        (None, [(4, 8, 0, 900, 50, 40.0, 0)]),
        # 6: a background and no events
        ((5, 0, 1.0), []),
        # 7: disjoint events of one class (both kept) and an event of no samples (dropped)
        ((6, 0, 0.5), [(2, 9, 0, 100, 0, 1.0, 0), (2, 9, 0, 100, 500, 1.0, 0), (2, 9, 0, 0, 300, 1.0, 0)]),
        # 8: four classes, later onsets first in the plan: four targets in onset order
        (None, [(2, 0, 0, 20, 40, 0.5, 0), (2, 1, 0, 20, 30, 0.5, 3), (2, 2, 0, 20, 20, 0.5, 0), (2, 3, 0, 20, 10, 0.5, 0)]),
    ]


QUIET = [1, 6, 2]        # the clips of a later call with fewer events than the one before it


def bad_clips(W):
    """clips that each hold one record outside the bank (status 2) next to a good event of class 9, whose target must survive"""
    good = (2, 9, 0, 50, 5, 0.5, 0)
    n = N_SRC
    return [
        (None, [(-1, 1, 0, 10, 0, 1.0, 0), good]),                      # src below the bank
        (None, [good, (n, 1, 0, 10, 0, 1.0, 0)]),                       # src above it
        (None, [(2, 1, -1, 10, 0, 1.0, 0), good]),                      # src_start < 0
        (None, [(2, 1, 0, -1, 0, 1.0, 0), good]),                       # n < 0
        (None, [(2, 1, 600, 101, 0, 1.0, 0), good]),                    # src_start + n > len
        (None, [(1, 1, 0, 4, 0, 1.0, 0), good]),                        # n > len
        (None, [(2, 1, 0, 10, -1, 1.0, 0), good]),                      # onset < 0
        ((n, 0, 1.0), [good]),                                          # background above the bank
        ((-2, 0, 1.0), [good]),                                         # background below "none"
        ((5, 700, 1.0), [good]),                                        # background start == len
        ((5, -1, 1.0), [good]),                                         # background start < 0
    ]


def records(chosen):
    """[(background, [events])] -> (bg, ev, ev_off) as the reference and sedt_soundscape read them"""
    bg = np.zeros(len(chosen), S.BACKGROUND)
    bg['src'] = -1
    rows, off = [], [0]
    for b, (g, events) in enumerate(chosen):
        if g is not None:
            bg[b] = (g[0], 0, g[1], g[2], 0)
        rows += [tuple(e) for e in events]
        off.append(len(rows))
    return bg, (np.array(rows, S.EVENT) if rows else np.zeros(0, S.EVENT)), np.asarray(off, np.int32)


def pick(W, B, lo=0):
    """B designed clips, cycling from clip ``lo``"""
    all_ = clips(W)
    return [all_[(lo + i) % len(all_)] for i in range(B)]
