"""TEST INFRASTRUCTURE, not product code: the "PSDS on recordings" definition restated on HOST numbers.

The product counts in csrc/recpsds.hip.  This module restates, in plain Python / NumPy float64, written from the definition's text and
importing nothing from the package, what that text adds to the clip-level oracle tests/psds_ref.counts - the WINDOWED form that makes
lists of any length affordable:

  * ``prefix_max``: per list of references the running maximum of the ends;
  * ``first_reference``: binary search for the first reference whose prefix maximum is > on_d, then a scan while on_g < off_d;
  * ``first_detection``: binary search for the first detection with max(on_d, off_d) > on_g (detections are disjoint, so that key
    ascends), then a scan while on_d < off_g;
  * the pass words: one 64-bit word per chunk of 64 detections, bit i % 64 of word i // 64 set when detection i passed the DTC.

The ORACLE the tests compare against is psds_ref.counts applied to WHOLE recordings as "clips", the reference passed in table order
(``oracle_counts``); ``status`` restates the two status values."""
import math

import numpy as np

import psds_ref

INCOMPLETE, UNORDERED = 1, 4


def sort_refs(events):
    """[(class, onset, offset)] in the table's order: by (onset, offset, input order)"""
    return [e for _, e in sorted(enumerate(events), key=lambda ie: (ie[1][1], ie[1][2], ie[0]))]


def prefix_max(ends):
    """the running maximum of one list's ends"""
    return list(np.maximum.accumulate(np.asarray(ends, np.float64))) if len(ends) else []


def first_reference(pmax, on_d):
    """the first j with pmax[j] > on_d (len(pmax) when there is none): no reference before it ends after on_d"""
    lo, hi = 0, len(pmax)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if pmax[mid] > on_d:
            hi = mid
        else:
            lo = mid + 1
    return lo


def first_detection(dets, on_g):
    """the first i with max(on_i, off_i) > on_g in a list of disjoint detections ascending by onset"""
    lo, hi = 0, len(dets)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if max(dets[mid][0], dets[mid][1]) > on_g:
            hi = mid
        else:
            lo = mid + 1
    return lo


def reference_sum(refs, pmax, on, off, dur):
    """sum of inter(d, g) / dur over refs [(onset, offset)] in table order, walking only from first_reference while on_g < off"""
    total = 0.0
    for j in range(first_reference(pmax, on), len(refs)):
        g_on, g_off = refs[j]
        if not g_on < off:
            break
        if not g_off - g_on > 0:
            continue
        inter = min(off, g_off) - max(on, g_on)
        if inter > 0:
            total = total + inter / dur
    return total


def recording_counts(dets, refs, rec_dur, n_classes, dtc=0.5, gtc=0.5, cttc=0.3):
    """ONE recording at ONE threshold through the windowed form: dets / refs [[(onset, offset)] per class] (detections ascending and
    disjoint, references in table order) -> (int64 [C, C + 1], pass words [[int] per class])"""
    C = n_classes
    cnt = np.zeros((C, C + 1), np.int64)
    pmax = [prefix_max([e[1] for e in refs[c]]) for c in range(C)]
    words = []
    for c in range(C):
        w = [0] * (-(-len(dets[c]) // 64))
        for i, (on, off) in enumerate(dets[c]):
            dur = off - on
            if not dur > 0:
                continue
            if reference_sum(refs[c], pmax[c], on, off, dur) >= dtc:
                w[i // 64] |= 1 << (i % 64)
                continue
            for o in range(C):
                if o != c and reference_sum(refs[o], pmax[o], on, off, dur) >= cttc:
                    cnt[c, o] += 1
            if (min(off, rec_dur) - max(on, 0.0)) / dur >= cttc:
                cnt[c, C] += 1
        for g_on, g_off in refs[c]:
            g_dur = g_off - g_on
            if not g_dur > 0:
                continue
            v = 0.0
            for i in range(first_detection(dets[c], g_on), len(dets[c])):
                on, off = dets[c][i]
                if not on < g_off:
                    break
                if not (w[i // 64] >> (i % 64)) & 1:
                    continue
                inter = min(off, g_off) - max(on, g_on)
                if inter > 0:
                    v = v + inter / g_dur
            if v >= gtc:
                cnt[c, c] += 1
        words.append(w)
    return cnt, words


def _table_refs(reference, name, labels):
    index = {l: i for i, l in enumerate(labels)}
    return sort_refs([(index[l] if l in index else int(l), float(a), float(b)) for l, a, b in reference[name]])


def windowed_counts(est, reference, filenames, durations, labels, K, dtc=0.5, gtc=0.5, cttc=0.3):
    """est {(k, r, c): [(onset, offset)]}, reference {filename: [(label, onset, offset)]} -> int64 [K, C, C + 1] through
    recording_counts; a filename outside the reference adds nothing"""
    C = len(labels)
    out = np.zeros((K, C, C + 1), np.int64)
    for r, name in enumerate(filenames):
        if name not in reference:
            continue
        table = _table_refs(reference, name, labels)
        refs = [[e[1:] for e in table if e[0] == c] for c in range(C)]
        for k in range(K):
            dets = [[(float(a), float(b)) for a, b in est.get((k, r, c), [])] for c in range(C)]
            out[k] += recording_counts(dets, refs, float(durations[r]), C, dtc, gtc, cttc)[0]
    return out


def oracle_counts(est, reference, filenames, durations, labels, K, dtc=0.5, gtc=0.5, cttc=0.3):
    """the ORACLE: psds_ref.counts with whole recordings as "clips" - clip r is filenames[r], its reference in table order (None
    for a filename outside the reference), its rows the detections class by class in onset order -> int64 [K, C, C + 1]"""
    C = len(labels)
    clips = [_table_refs(reference, name, labels) if name in reference else None for name in filenames]
    tables = [[(r, c, float(a), float(b)) for r in range(len(filenames)) for c in range(C) for a, b in est.get((k, r, c), [])]
              for k in range(K)]
    return np.asarray(psds_ref.counts(tables, clips, [float(d) for d in durations], labels, dtc, gtc, cttc), np.int64).reshape(K, C, C + 1)


def constants(reference, filenames, durations, labels):
    """psds_ref.constants over the evaluated recordings of one call (those in the reference): (n_c, T_c, T)"""
    clips = [reference.get(name) for name in filenames]
    return psds_ref.constants(clips, [float(d) for d in durations], labels)


def status(dets, refs, stitch_status=0, counts=None, cap=None):
    """the status of one (threshold, recording): dets / refs [[(onset, offset)] per class] as the kernel reads them"""
    if stitch_status != 0 or (counts is not None and any(n > cap for n in counts)):
        return INCOMPLETE
    for c in range(len(dets)):
        for lst, disjoint in ((dets[c], True), (refs[c], False)):
            for i, (on, off) in enumerate(lst):
                if not (math.isfinite(on) and math.isfinite(off)):
                    return UNORDERED
                if i and (not on >= lst[i - 1][0] or (disjoint and not on >= lst[i - 1][1])):
                    return UNORDERED
    return 0
