"""NumPy restatement of "Soundscapes synthesized on the device" (include/sedt_hip.h: sedt_bank_stats, sedt_soundscape; DESIGN.md section
4), written from the definition, not from the kernel: no chunks, no vectors, no waves - every sample of a clip, every event in plan order.

The plan (``draw``).  np.random is consumed clip by clip: the background's index randint(n_bg) and start randint(len_bg) (nothing with
background=False); K = randint(lo, hi + 1); per event the class randint(number of classes that have sounds), the sound
randint(sounds of the class), snr = uniform(lo, hi), n = min(len_src, max_event_samples, window), src_start = randint(len_src - n + 1),
onset = randint(window - n + 1).  Gains in float64, stored as float32: 10^(ref_db / 20) / rms_bg (1 for a silent background),
10^((ref_db + snr) / 20) / rms_src; fade = round(fade_seconds * sr).

The wave (``mix``).  float32, every operation rounded on its own: acc = g_bg * bg[(start + t) mod len] (0 without a background); for
every valid event k in plan order with onset <= t < e_k = min(onset + n, window), i = t - onset:
acc = acc + ((g * w(i)) * src[src_start + i]), w = min(w_in, w_out), w_in = i < fade ? float32((i + 1) / (fade + 1)) : 1,
w_out = n - 1 - i < fade ? float32((n - i) / (fade + 1)) : 1, the divisions in float64.  peak = max |acc|, scale = peak > peak_limit ?
float32(float64(peak_limit) / float64(peak)) : 1, the written sample acc * scale (acc itself when the scale is 1).

The targets (``clip_targets``).  Every valid event gives (cls, onset, e_k); with collapse the events of one class sorted by (onset, end)
are merged while onset <= the running end (``collapse``: data_utils/collapse_event.py on the integer grid); kept iff z - a > 0 and
z - a >= min_event_seconds with a = onset / sr, z = end / sr; ordered by (onset, end, cls); box (float32(((a + z) * 0.5) / W),
float32((z - a) / W)), W = window / sr.  status: 2 a record outside the bank (it contributes nothing), else 1 more than max_targets
kept events (the first max_targets are written), else 0."""
import numpy as np

EVENT = np.dtype([('src', '<i4'), ('cls', '<i4'), ('src_start', '<i8'), ('n', '<i8'), ('onset', '<i8'), ('gain', '<f4'), ('fade', '<i4')])
BACKGROUND = np.dtype([('src', '<i4'), ('pad', '<i4'), ('start', '<i8'), ('gain', '<f4'), ('pad2', '<i4')])
MAXEV = 63


# ---------------------------------------------------------------------------------------------------- the plan
def gain(ref_db, snr_db, rms):
    if float(rms) == 0.0:
        return np.float32(1.0)
    return np.float32(np.float64(10.0) ** ((np.float64(ref_db) + np.float64(snr_db)) / np.float64(20.0)) / np.float64(rms))


def draw(B, lens, rms, by_class, backgrounds, window, sr, n_events=(1, 9), snr_db=(6.0, 30.0), ref_db=-30.0, max_event_seconds=None,
         fade_seconds=0.01, background=True):
    """(bg BACKGROUND [B], ev EVENT [E], ev_off int32 [B + 1]) - consumes np.random as the module docstring says"""
    classes = [c for c, own in enumerate(by_class) if len(own)]
    cap = window if max_event_seconds is None else max(int(round(float(max_event_seconds) * sr)), 1)
    fade = int(round(float(fade_seconds) * sr))
    bg = np.zeros(B, BACKGROUND)
    bg['src'] = -1
    ev, off = [], [0]
    for b in range(B):
        if background:
            s = backgrounds[np.random.randint(len(backgrounds))]
            start = np.random.randint(lens[s])
            bg[b] = (s, 0, start, gain(ref_db, 0.0, rms[s]), 0)
        K = np.random.randint(n_events[0], n_events[1] + 1)
        for _ in range(K):
            c = classes[np.random.randint(len(classes))]
            s = by_class[c][np.random.randint(len(by_class[c]))]
            snr = np.random.uniform(snr_db[0], snr_db[1])
            n = min(lens[s], cap, window)
            src_start = np.random.randint(lens[s] - n + 1)
            onset = np.random.randint(window - n + 1)
            ev.append((s, c, src_start, n, onset, gain(ref_db, snr, rms[s]), fade))
        off.append(len(ev))
    return bg, (np.array(ev, EVENT) if ev else np.zeros(0, EVENT)), np.asarray(off, np.int32)


# ---------------------------------------------------------------------------------------------------- validity
def event_ok(e, lens):
    s = int(e['src'])
    if not 0 <= s < len(lens):
        return False
    return int(e['src_start']) >= 0 and int(e['n']) >= 0 and int(e['src_start']) + int(e['n']) <= lens[s] and int(e['onset']) >= 0


def background_state(g, lens):
    """'none', 'ok' or 'bad'"""
    s = int(g['src'])
    if s == -1:
        return 'none'
    if not 0 <= s < len(lens) or not 0 <= int(g['start']) < lens[s]:
        return 'bad'
    return 'ok'


# ---------------------------------------------------------------------------------------------------- the wave
def fade_weight(i, n, fade):
    """float32 [len(i)]: min(w_in, w_out) of event samples i (int64 array) of an event of n samples"""
    fade = max(int(fade), 0)
    w_in = np.where(i < fade, ((i + 1).astype(np.float64) / np.float64(fade + 1)).astype(np.float32), np.float32(1.0))
    w_out = np.where(n - 1 - i < fade, ((n - i).astype(np.float64) / np.float64(fade + 1)).astype(np.float32), np.float32(1.0))
    return np.minimum(w_in, w_out).astype(np.float32)


def mix_clip(sources, g, events, window, peak_limit):
    """(wave float32 [window], peak float32, scale float32) of one clip; sources: list of 1-D float32 arrays"""
    lens = [len(s) for s in sources]
    t = np.arange(window, dtype=np.int64)
    acc = np.zeros(window, np.float32)
    if background_state(g, lens) == 'ok':
        src = sources[int(g['src'])]
        acc = np.float32(g['gain']) * src[(int(g['start']) + t) % len(src)]
    for e in events:
        if not event_ok(e, lens):
            continue
        onset, n = int(e['onset']), int(e['n'])
        end = min(onset + n, window)
        if end <= onset:
            continue
        i = np.arange(end - onset, dtype=np.int64)
        x = sources[int(e['src'])][int(e['src_start']) + i]
        gw = (np.float32(e['gain']) * fade_weight(i, n, int(e['fade']))).astype(np.float32)
        term = (gw * x).astype(np.float32)
        acc[onset:end] = (acc[onset:end] + term).astype(np.float32)
    peak = np.float32(np.max(np.abs(acc))) if window else np.float32(0)
    limit = np.float32(peak_limit)
    scale = np.float32(np.float64(limit) / np.float64(peak)) if peak > limit else np.float32(1.0)
    if scale != np.float32(1.0):
        acc = (acc * scale).astype(np.float32)
    return acc.astype(np.float32), peak, scale


# ---------------------------------------------------------------------------------------------------- the targets
def collapse(events):
    """[(cls, onset, end)] -> the merged list: per class sorted by (onset, end); an event whose onset <= the running end of its
    predecessor joins it, the end becomes the maximum (data_utils/collapse_event.py: collapse, touching events included)"""
    out = []
    for c in sorted(set(e[0] for e in events)):
        own = sorted((e[1], e[2]) for e in events if e[0] == c)
        cur = None
        for on, end in own:
            if cur is not None and on <= cur[1]:
                cur[1] = max(cur[1], end)
            else:
                if cur is not None:
                    out.append((c, cur[0], cur[1]))
                cur = [on, end]
        if cur is not None:
            out.append((c, cur[0], cur[1]))
    return out


def clip_targets(g, events, lens, window, sr, max_targets, min_event_seconds=0.0, do_collapse=True):
    """(labels int64 (n,), boxes float32 (n, 2), status) of one clip"""
    bad = background_state(g, lens) == 'bad' or len(events) > MAXEV
    trip = []
    for e in events[:MAXEV]:
        if not event_ok(e, lens):
            bad = True
            continue
        onset = int(e['onset'])
        trip.append((int(e['cls']), onset, min(onset + int(e['n']), window)))
    if do_collapse:
        trip = collapse(trip)
    W = np.float64(window) / np.float64(sr)
    kept = []
    for c, on, end in trip:
        a, z = np.float64(on) / np.float64(sr), np.float64(end) / np.float64(sr)
        d = z - a
        if d > 0 and d >= np.float64(min_event_seconds):
            kept.append((on, end, c, np.float32(((a + z) * np.float64(0.5)) / W), np.float32(d / W)))
    kept.sort(key=lambda k: k[:3])
    status = 2 if bad else (1 if len(kept) > max_targets else 0)
    kept = kept[:max_targets]
    return (np.asarray([k[2] for k in kept], np.int64), np.asarray([(k[3], k[4]) for k in kept], np.float32).reshape(-1, 2), status)


def soundscape(sources, bg, ev, ev_off, window, sr, max_targets, min_event_seconds=0.0, do_collapse=True, peak_limit=1.0):
    """the whole call: (wave float32 [B, window], peak [B], scale [B], [(labels, boxes)] per clip, status int32 [B])"""
    B = len(bg)
    lens = [len(s) for s in sources]
    wave, peak, scale = np.zeros((B, window), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
    targets, status = [], np.zeros(B, np.int32)
    for b in range(B):
        events = ev[int(ev_off[b]):int(ev_off[b + 1])]
        wave[b], peak[b], scale[b] = mix_clip(sources, bg[b], events[:MAXEV], window, peak_limit)
        lab, box, status[b] = clip_targets(bg[b], events, lens, window, sr, max_targets, min_event_seconds, do_collapse)
        targets.append((lab, box))
    return wave, peak, scale, targets, status


def bank_stats(sources):
    """(sumsq float64, peak float32) per source"""
    return (np.asarray([np.sum(s.astype(np.float64) ** 2) for s in sources], np.float64),
            np.asarray([np.max(np.abs(s)) if len(s) else 0 for s in sources], np.float32))
