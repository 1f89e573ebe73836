""""Levels measured after the effects" restated in float64 - the reference of sedt_relevel (csrc/relevel.hip) and utilities/relevel.py,
built on tests/loudness_ref.py (measure) and tests/soundscape_ref.py (bank_stats).  DESIGN.md section 4 holds the definition.

A region x of n samples has the level  mode 'rms': (sum of x^2) / n;  mode 'lufs': zbar of loudness_ref.measure.  Its target amplitude
is 10^(target_db / 20) under 'rms' and 10^((target_db + 0.691) / 20) under 'lufs', so that L = -0.691 + 10 log10(g^2 zbar) = target_db.
g = float32(target / sqrt(level)); a level that is 0 or not finite: status 1, no gain.

``event_region`` says WHAT is measured of an event (the generators measure the processed event): the wet row, head and tail ONCE; the
stretched row; or the bank excerpt - and takes the planted faults of tests/test_relevel_cpu.py."""
import math

import numpy as np

import loudness_ref as LR
import soundscape_ref as S

MODES = ('rms', 'lufs')
FAULTS = ('tail_twice', 'whole_source', 'no_offset')


def target_amplitude(target_db, mode, fault=None):
    """float64: the amplitude a region at target_db has; fault 'no_offset' drops the 0.691 of L = -0.691 + 10 log10(zbar)"""
    assert mode in MODES
    db = np.float64(target_db) + (np.float64(0.691) if mode == 'lufs' and fault != 'no_offset' else np.float64(0.0))
    return np.float64(10.0) ** (db / np.float64(20.0))


def level(x, sr, mode):
    """dict(level float64, counts [4]; under 'lufs' also z, thr) of one region"""
    x = np.asarray(x, np.float32)
    if mode == 'rms':
        return dict(level=float(S.bank_stats([x])[0][0] / np.float64(len(x))), counts=[min(len(x), 2 ** 31 - 1), 0, 0, 0])
    m = LR.measure(x, sr)
    return dict(level=m['zbar'], counts=[m['J'], m['n_abs'], m['n_rel'], int(m['short'])], z=m['z'], thr=m['thr'])


def gain(target, lv):
    """(status, float32 gain or None)"""
    if not (math.isfinite(lv) and lv > 0.0):
        return 1, None
    return 0, np.float32(np.float64(target) / np.sqrt(np.float64(lv)))


def relevel(regions, targets, sr, mode):
    """[dict(level, counts, status, gain)] of regions (1-D float32 arrays) brought to ``targets`` (amplitudes)"""
    out = []
    for x, t in zip(regions, targets):
        m = level(x, sr, mode)
        m['status'], m['gain'] = gain(t, m['level'])
        out.append(m)
    return out


def event_region(source, src_start, n, row=None, head=None, fault=None):
    """the samples that are measured of an event: ``row`` - its stretched row, or its wet row with ``head`` the dry length - when it has
    one, else the excerpt source[src_start : src_start + n].  Faults: 'tail_twice' appends the wet row's tail once more;
    'whole_source' measures the whole source instead of the excerpt"""
    if row is not None:
        row = np.asarray(row, np.float32)
        return np.concatenate([row, row[head:]]) if fault == 'tail_twice' and head is not None else row
    source = np.asarray(source, np.float32)
    return source if fault == 'whole_source' else source[int(src_start):int(src_start) + int(n)]


def event_gain(target_db, sr, mode, source, src_start, n, row=None, head=None, fault=None):
    """(status, gain) of one event at target_db"""
    m = level(event_region(source, src_start, n, row, head, fault), sr, mode)
    return gain(target_amplitude(target_db, mode, fault), m['level'])


def measured_db(x, sr, mode):
    """the level of a mixed wave in dB of its RMS / in LUFS (-inf for silence)"""
    lv = level(x, sr, mode)['level']
    if not lv > 0:
        return -math.inf
    return 10.0 * math.log10(lv) - (0.691 if mode == 'lufs' else 0.0)
