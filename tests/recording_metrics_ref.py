"""TEST INFRASTRUCTURE, not product code: the "Scoring recordings" definition restated on HOST numbers.

The product counts in csrc/recmetrics.hip.  This module restates, in plain Python / NumPy float64 and written from the definition's
text, the two things that text adds to the clip-level oracles:

  * the block decomposition (``blocks``, ``block_event_counts``): the two lists of a class merged by onset, a block closed between
    two consecutive items whose rounded float64 onset difference exceeds t_collar, blocks formed while both lists have items left, a
    block of more than 64 references or 64 estimates a status 2; inside a block the matchers of tests/event_metrics_ref.py
    (imported, not changed);
  * the word sweep (``sweep_segment_counts``): the recording walked in words of 64 segments with one cursor per list and the running
    maximum of the end segment for overlapping events.

The ORACLES the tests compare against are the clip-level restatements applied to a WHOLE recording's lists, without any limit:
event_metrics_ref.clip_event_counts / clip_tag_counts and segment_metrics_ref.clip_segment_counts (``recording_counts``).

``stitch_buffers`` builds stitch-layout buffers (count, out, status) from Python event lists through ops.stitch_events_views."""
import math

import numpy as np

import event_metrics_ref as E
import segment_metrics_ref as S

BLOCK = 64
INCOMPLETE, OVER_CAPACITY, UNORDERED = 1, 2, 4


def sort_refs(events):
    """[(class, onset, offset)] in the table's order: by (onset, offset, input order)"""
    return [e for _, e in sorted(enumerate(events), key=lambda ie: (ie[1][1], ie[1][2], ie[0]))]


def blocks(est_on, ref_on, t_collar):
    """the block decomposition of ONE class: est_on / ref_on ascending float64 onsets -> ([(ie, a, ir, b)], status): block = a estimates
    from ie and b references from ir.  Blocks are formed while both lists have items left; status 2 when a block would hold a 65th
    estimate or reference (the blocks before it are returned)"""
    out, ie, ir = [], 0, 0
    while ie < len(est_on) and ir < len(ref_on):
        a = b = 0
        last = None
        while ie + a < len(est_on) or ir + b < len(ref_on):
            he, hr = ie + a < len(est_on), ir + b < len(ref_on)
            take_e = he and (not hr or est_on[ie + a] <= ref_on[ir + b])
            x = float(est_on[ie + a] if take_e else ref_on[ir + b])
            if last is not None and (x - last) > t_collar:
                break
            if (a if take_e else b) == BLOCK:
                return out, OVER_CAPACITY
            a, b, last = a + take_e, b + (not take_e), x
        out.append((ie, a, ir, b))
        ie, ir = ie + a, ir + b
    return out, 0


def block_event_counts(refs, ests, n_classes, t_collar=0.2, pct=0.2, optimal=True):
    """one recording through the block decomposition: refs (sorted by sort_refs) / ests (class, onset, offset) with the estimates of a
    class ascending by onset -> (int64 [C, 3] {tp, n_ref, n_sys}, status)"""
    out, status = np.zeros((n_classes, 3), np.int64), 0
    for c in range(n_classes):
        r = [e for e in refs if e[0] == c]
        s = [e for e in ests if e[0] == c]
        bl, st = blocks([e[1] for e in s], [e[1] for e in r], t_collar)
        status = max(status, st)
        tp = sum(int(E.clip_event_counts(r[ir:ir + b], s[ie:ie + a], n_classes, t_collar, pct, optimal)[c, 0]) for ie, a, ir, b in bl)
        out[c] = (tp, len(r), len(s))
    return out, status


def _segment(q, n_seg):
    return 0 if q < 0 else (n_seg if q > n_seg else int(q))


def _word(events, cur, lo, rho, n_seg):
    """bits of the segments lo .. lo + 63 one list covers; cur = [cursor, reach] is advanced"""
    hi, m = lo + 64, 0
    if cur[1] > lo:
        m = (1 << (min(cur[1], hi) - lo)) - 1
    while cur[0] < len(events):
        s0 = _segment(math.floor(events[cur[0]][1] / rho), n_seg)
        if s0 >= hi:
            break
        s1 = _segment(math.ceil(events[cur[0]][2] / rho), n_seg)
        cur[0] += 1
        if s1 <= s0:
            continue
        cur[1] = max(cur[1], s1)
        if s1 <= lo:
            continue
        m |= ((1 << (min(s1, hi) - lo)) - 1) & ~((1 << (max(s0, lo) - lo)) - 1)
    return m


def sweep_segment_counts(refs, ests, n_classes, rho, n_words):
    """one recording through the word sweep: (int64 [C, 3] {tp, n_ref, n_sys}, int64 [3] {S, D, I}) over n_words words of 64 segments"""
    cw, sdi, n_seg = np.zeros((n_classes, 3), np.int64), np.zeros(3, np.int64), 64 * n_words
    lists = [([e for e in ests if e[0] == c], [e for e in refs if e[0] == c]) for c in range(n_classes)]
    cur = [([0, 0], [0, 0]) for _ in range(n_classes)]
    for w in range(n_words):
        me = [_word(lists[c][0], cur[c][0], 64 * w, rho, n_seg) for c in range(n_classes)]
        mr = [_word(lists[c][1], cur[c][1], 64 * w, rho, n_seg) for c in range(n_classes)]
        for c in range(n_classes):
            cw[c] += (bin(me[c] & mr[c]).count('1'), bin(mr[c]).count('1'), bin(me[c]).count('1'))
        for bit in range(64):
            nr, ns = sum((m >> bit) & 1 for m in mr), sum((m >> bit) & 1 for m in me)
            nt = sum((a >> bit) & (b >> bit) & 1 for a, b in zip(me, mr))
            sdi += (min(nr, ns) - nt, max(0, nr - ns), max(0, ns - nr))
    return cw, sdi


def n_words(rec_dur, refs, rho):
    """ceil(ceil(max(rec_dur, largest reference offset) / rho) / 64)"""
    return -(-math.ceil(max([rec_dur] + [e[2] for e in refs]) / rho) // 64)


# ---------------------------------------------------------------------------------------------------------------- whole recordings
def recording_counts(est, reference, filenames, labels, K, t_collar=0.2, pct=0.2, optimal=True, rho=None):
    """the ORACLE: est {(k, r, c): [(onset, offset)]}, reference {filename: [(label, onset, offset)]} -> the counters of one fusion
    strategy, from the clip-level restatements applied to the whole recording: ev / tag [K, C, 3] (+ seg [K, C, 3], sdi [K, 3])"""
    C, index = len(labels), {l: i for i, l in enumerate(labels)}
    ev, tag = np.zeros((K, C, 3), np.int64), np.zeros((K, C, 3), np.int64)
    seg, sdi = np.zeros((K, C, 3), np.int64), np.zeros((K, 3), np.int64)
    for r, name in enumerate(filenames):
        if name not in reference:
            continue
        refs = sort_refs([(index[l] if l in index else int(l), float(a), float(b)) for l, a, b in reference[name]])
        for k in range(K):
            ests = [(c, a, b) for c in range(C) for a, b in est.get((k, r, c), [])]
            ev[k] += E.clip_event_counts(refs, ests, C, t_collar, pct, optimal)
            tag[k] += E.clip_tag_counts({e[0] for e in refs}, {e[0] for e in ests}, C)
            if rho is not None:
                cw, x = S.clip_segment_counts(refs, ests, C, rho)
                seg[k] += cw
                sdi[k] += x
    return (ev, tag, seg, sdi) if rho is not None else (ev, tag)


def stitch_buffers(est, K, R, C, cap, fill=0):
    """est {(k, r, c): [(onset, offset)]} -> (count [K,R,C], out [K,R,C,cap,8], status [K,R]) int32 in ops.stitch_events' layout: the
    first min(len, cap) events of every list written in order, count = len (it keeps counting past cap), everything else ``fill``"""
    from sound_event_detection_transformer_amd import ops
    count = np.zeros((K, R, C), np.int32)
    out = np.full((K, R, C, cap, ops.STITCH_WORDS), fill, np.int32)
    times, score, n_merged, window, query = ops.stitch_events_views(out)
    for (k, r, c), events in est.items():
        count[k, r, c] = len(events)
        for i, (on, off) in enumerate(events[:cap]):
            times[k, r, c, i] = (on, off)
            score[k, r, c, i], n_merged[k, r, c, i], window[k, r, c, i], query[k, r, c, i] = 0.5, 1, 0, i % 64
    return count, out, np.zeros((K, R), np.int32)
