"""NumPy / float64 restatement of the "Recordings of any length" definition: the window plan and the
stitching of per-window event records into one event list per (threshold, recording, class).  Written from that text, not from
csrc/stitch.hip: candidates are gathered for the whole recording, sorted by (on, w, s) and swept once per class; the status words
follow the text's own wording (the working-set rule is evaluated from scratch at every window)."""
import math

import numpy as np

WORKING_SET = 640
UNORDERED, OVERFLOW, EARLY, TABLE = 1, 2, 4, 8


def window_plan(n, window, hop, min_samples=1):
    if not 1 <= hop <= window:
        raise ValueError('hop')
    if n < max(min_samples, 1):
        raise ValueError('short')
    if n <= window:
        return [0]
    count = 1 + int(math.ceil((n - window) / hop))
    return [min(w * hop, n - window) for w in range(count)]


def _min(a, b):
    """min(a, b) = a > b ? b : a"""
    return b if a > b else a


def candidates(record, t_w, dur, Q, C):
    """the kept candidates of one window record [1 + 5 Q] int32: [(on, s, off, score f32, class, query)]"""
    n = int(record[0])
    if not 0 <= n <= Q:
        return []
    slots = record[1:].reshape(Q, 5)
    out = []
    for s in range(n):
        cls = int(slots[s, 0])
        on32, off32, sc = (np.float32(v) for v in slots[s, 1:4].view(np.float32))
        if not 0 <= cls < C or np.isnan(sc):
            continue
        with np.errstate(all='ignore'):
            on = _min(float(t_w) + float(on32), float(dur))
            off = _min(float(t_w) + float(off32), float(dur))
            if not (off - on > 0):
                continue
        out.append((on, s, off, sc, cls, int(slots[s, 4])))
    return out


def sweep(cands, gap):
    """cands [(on, w, s, off, score, query)] of ONE class -> merged events [(on, off, score, n, window, query)]"""
    events, cur = [], None
    for on, w, s, off, sc, q in sorted(cands, key=lambda c: (c[0], c[1], c[2])):
        if cur is not None and on <= cur[1] + gap:
            cur[1] = max(cur[1], off)
            cur[3] += 1
            if sc > cur[2]:
                cur[2], cur[4], cur[5] = sc, w, q
        else:
            if cur is not None:
                events.append(tuple(cur))
            cur = [on, off, sc, 1, w, q]
    if cur is not None:
        events.append(tuple(cur))
    return events


def _merge_all(per_window, C, gap):
    """per_window: [[(on, s, off, score, class, query)]] by window index -> {class: merged events}"""
    by_class = {}
    for w, cs in enumerate(per_window):
        for on, s, off, sc, cls, q in cs:
            by_class.setdefault(cls, []).append((on, w, s, off, sc, q))
    return {c: sweep(v, gap) for c, v in by_class.items()}


def stitch_one(records, t, dur, Q, C, gap, check_working_set=True):
    """one (threshold, recording): records [W_r, 1 + 5 Q], t [W_r] -> (status, {class: merged events})"""
    t = [float(v) for v in t]
    if any(math.isnan(v) for v in t) or any(not (t[i] >= t[i - 1]) for i in range(1, len(t))):
        return UNORDERED, {}
    per_window = []
    for w in range(len(t)):
        cs = candidates(records[w], t[w], dur, Q, C)
        if any(c[0] < t[w] for c in cs):
            return EARLY, {}
        if check_working_set:
            still_open = sum(1 for ev in _merge_all(per_window, C, gap).values() for e in ev if e[1] + gap >= t[w])
            if still_open + len(cs) > WORKING_SET:
                return OVERFLOW, {}
        per_window.append(cs)
    return 0, _merge_all(per_window, C, gap)


def stitch(records, win_off, win_start, rec_dur, C, merge_gap, check_working_set=True):
    """records [K, W_stride, 1 + 5 Q] int32 -> (count [K, R, C] int32, status [K, R] int32, events {(k, r, c): [(on, off, score, n,
    window, query)]}); a raised status leaves the recording's counts at 0"""
    records = np.asarray(records)
    K, W = records.shape[0], len(win_start)
    Q = (records.shape[2] - 1) // 5
    R = len(win_off) - 1
    count, status, events = np.zeros((K, R, C), np.int32), np.zeros((K, R), np.int32), {}
    for k in range(K):
        for r in range(R):
            w0, w1 = int(win_off[r]), int(win_off[r + 1])
            if w0 < 0 or w1 < w0 or w1 > W:
                status[k, r] = TABLE
                continue
            st, ev = stitch_one(records[k, w0:w1], win_start[w0:w1], rec_dur[r], Q, C, float(merge_gap), check_working_set)
            status[k, r] = st
            for c, lst in ev.items():
                count[k, r, c] = len(lst)
                events[(k, r, c)] = lst
    return count, status, events


def fill(out, events, cap):
    """``out`` [K, R, C, cap, 8] int32 (a copy of what the buffer held before the launch) with the first min(count, cap) slots of every
    list written as the kernel writes them: what the buffer must hold afterwards, word for word"""
    out = np.array(out, copy=True)
    for (k, r, c), lst in events.items():
        for i, (on, off, sc, n, w, q) in enumerate(lst[:cap]):
            out[k, r, c, i, 0:4] = np.array([on, off], np.float64).view(np.int32)
            out[k, r, c, i, 4] = np.array([sc], np.float32).view(np.int32)[0]
            out[k, r, c, i, 5:8] = (n, w, q)
    return out


def pack(windows, Q, K=1):
    """hand-written windows -> records [K, W, 1 + 5 Q]: ``windows`` is a list (per window) of event lists [(class, on32, off32, score)
    or (class, on32, off32, score, query)]; the slots past the events hold decode_events' filler {-1, 0, 0, 0, -1}; the same at every k"""
    rec = np.zeros((K, len(windows), 1 + 5 * Q), np.int32)
    slots = rec[:, :, 1:].reshape(K, len(windows), Q, 5)
    slots[..., 0] = slots[..., 4] = -1
    for w, evs in enumerate(windows):
        rec[:, w, 0] = len(evs)
        for s, e in enumerate(evs):
            slots[:, w, s, 0] = e[0]
            slots[:, w, s, 1:4] = np.array(e[1:4], np.float32).view(np.int32)
            slots[:, w, s, 4] = e[4] if len(e) > 4 else s
    return rec
