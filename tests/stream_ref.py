"""NumPy / float64 restatement of the "Live streams" definition: the stitch sweep one window at a time with the
open set carried from step to step, and the waveform rings.  Written from that text, not from csrc/stitch.hip: the open set is a
Python list of merged events, a step is plain list handling, and the candidates of a window come from recording_ref.candidates
(the clipping rule is the offline one)."""
import math

import numpy as np

import recording_ref as R

WORKING_SET = 640
UNORDERED, OVERFLOW, EARLY, ROW = 1, 2, 4, 8
SKIP, ADD, FLUSH, ADD_FLUSH = 0, 1, 2, 3


class Stream(object):
    """the carried state of one (threshold, stream): the open merged events, the status, the windows seen, the last t_w and the
    running count per class"""

    def __init__(self, C):
        self.open, self.status, self.seen, self.last, self.count = [], 0, 0, 0.0, [0] * C


def _better(a, b):
    """the member that gives score, window and query: the highest score; among equal scores the first in (onset, window, slot)"""
    ka, kb = (a['pon'], a['win'], a['slot']), (b['pon'], b['win'], b['slot'])
    return a['score'] > b['score'] if a['score'] != b['score'] else ka < kb


def _leave(st, final):
    """final events leave in (class, onset) order: [(on, off, score, n, window, query, class)]"""
    final = sorted(final, key=lambda e: (e['cls'], e['on']))
    for e in final:
        st.count[e['cls']] += 1
    return [(e['on'], e['off'], e['score'], e['n'], e['win'], e['q'], e['cls']) for e in final]


def step(st, action, record, t_w, dur, win_index, Q, C, gap, row_ok=True):
    """one launch for one (threshold, stream): returns the events it emits, in order.  ``record`` [1 + 5 Q] int32"""
    if action == SKIP or st.status:
        return []
    out = []
    if action & ADD:
        t_w = float(t_w)
        if not row_ok:
            st.status = ROW
            return []
        if math.isnan(t_w) or (st.seen > 0 and not t_w >= st.last):
            st.status = UNORDERED
            return []
        cands = R.candidates(record, t_w, dur, Q, C)
        if any(c[0] < t_w for c in cands):
            st.status = EARLY
            return []
        final = [e for e in st.open if e['off'] + gap < t_w]
        rest = [e for e in st.open if not e['off'] + gap < t_w]
        if len(rest) + len(cands) > WORKING_SET:
            st.status = OVERFLOW
            return []
        out += _leave(st, final)
        for on, s, off, sc, cls, q in cands:                         # slot order
            new = {'on': on, 'off': off, 'pon': on, 'score': sc, 'n': 1, 'win': int(win_index), 'q': q, 'slot': s, 'cls': cls}
            touched = [e for e in rest if e['cls'] == cls and on <= e['off'] + gap and e['on'] <= off + gap]
            for e in touched:
                best = e if _better(e, new) else new
                new = {'on': min(new['on'], e['on']), 'off': max(new['off'], e['off']), 'pon': best['pon'], 'score': best['score'],
                       'n': new['n'] + e['n'], 'win': best['win'], 'q': best['q'], 'slot': best['slot'], 'cls': cls}
            rest = [e for e in rest if not any(e is t for t in touched)] + [new]
        st.open, st.seen, st.last = rest, st.seen + 1, t_w
    if action & FLUSH:
        out += _leave(st, st.open)
        st.open = []
    return out


def run(records, t, dur, C, gap, last_action=FLUSH):
    """a whole stream through ``step``: records [W, 1 + 5 Q], t [W], dur [W] (the duration every window is clipped against) ->
    (status, {class: [(on, off, score, n, window, query)]}); last_action FLUSH: every window with ADD and a final FLUSH;
    ADD_FLUSH: the last window with ADD_FLUSH"""
    records = np.asarray(records)
    Q = (records.shape[1] - 1) // 5
    st, out = Stream(C), []
    for w in range(len(t)):
        a = ADD_FLUSH if (last_action == ADD_FLUSH and w == len(t) - 1) else ADD
        out += step(st, a, records[w], t[w], dur[w], w, Q, C, gap)
    if last_action == FLUSH or not len(t):
        out += step(st, FLUSH, None, 0.0, 0.0, 0, Q, C, gap)
    by_class = {}
    if not st.status:
        for e in out:
            by_class.setdefault(e[6], []).append(e[:6])
    return st.status, by_class


def emit_words(events):
    """[(on, off, score, n, window, query, class)] -> int32 [n, 10] as the kernel writes them"""
    out = np.zeros((len(events), 10), np.int32)
    for i, (on, off, sc, n, w, q, c) in enumerate(events):
        out[i, 0:4] = np.array([on, off], np.float64).view(np.int32)
        out[i, 4] = np.array([sc], np.float32).view(np.int32)[0]
        out[i, 5:9] = (n, w, q, c)
    return out


class Rings(object):
    """the waveform rings: [S, ring] float32, append wraps, cut reads across the wrap point and zero-pads"""

    def __init__(self, S, ring):
        self.buf = np.zeros((S, ring), np.float32)

    def append(self, s, pos, x):
        ring = self.buf.shape[1]
        for i, v in enumerate(np.asarray(x, np.float32)):
            self.buf[s, (pos + i) % ring] = v

    def cut(self, jobs, B, window):
        ring = self.buf.shape[1]
        wave = np.zeros((B, window), np.float32)
        for s, pos, n, row in jobs:
            wave[row, :n] = self.buf[s, (pos + np.arange(n)) % ring]
        return wave
