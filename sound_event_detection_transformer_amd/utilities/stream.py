"""Sound events in live streams.  utilities.recording.RecordingDetector needs a recording that has ended; here audio arrives in
chunks of any size on ``n_streams`` streams at once, every stream's last samples live in a ring on the device
(ops.stream_append / ops.stream_cut, csrc/stream.hip), each window that became due goes through the same graphed detect step as a
recording's windows - the streams are the batch of one replay - and the stitch sweep runs ONE window per launch with the open events
of every stream kept on the device between launches (ops.stitch_stream, csrc/stitch.hip).  An event is handed out once no later window
can change it.  DESIGN.md section 4 ("Live streams") holds the definition; the events a stream emits over its lifetime are those
RecordingDetector gives for the whole recording.

    det = StreamDetector(model, postprocessor, decoder, mel, transform, 10.0, 5.0, n_streams=2, names=['door', 'yard'])
    events = det.push([chunk_a, chunk_b]).result()                 # {at_m: StreamEvents}: what became final with these chunks
    last = det.finish().result()                                   # the streams end: everything still open

``stream_plan`` and ``stream_finish`` are the host half and need no GPU."""
import numpy as np
import torch

from .. import ops
from .predictions import COLUMNS, operating_point
from .recording import RecordingDetector, check_depth

MAX_STATE_BYTES = 1 << 30         # the open-set state of one fusion strategy
STATUS_REASONS = {1: 'its window starts are not ascending', 2: 'more events were open at once than the stitch kernel holds: use a '
                  'longer hop or a smaller merge_gap', 4: 'a window record holds an event with a negative onset: decode with a finite '
                  'max_len', 8: 'its window row is not a row of the batch'}
SKIP, ADD, FLUSH, ADD_FLUSH = 0, 1, 2, 3        # sedt_stitch_stream's actions


def stream_plan(received_before, received_now, window, hop):
    """the start samples (int64, ascending) of the windows that became due while a stream grew from ``received_before`` to
    ``received_now`` samples: window w starts at w * hop and is due once w * hop + window <= received"""
    a, b, win, hop = int(received_before), int(received_now), int(window), int(hop)
    if not 1 <= hop <= win:
        raise ValueError(f'stream_plan: hop {hop} outside 1 .. window {win}')
    if not 0 <= a <= b:
        raise ValueError(f'stream_plan: received {a} -> {b} samples')
    due = lambda n: 0 if n < win else (n - win) // hop + 1
    return np.arange(due(a), due(b), dtype=np.int64) * hop


def stream_finish(n, window, hop, min_samples=1):
    """the closing window of a stream that ends after ``n`` samples: None or (start sample, length).  n == 0: none; 0 < n <
    min_samples: ValueError, as window_plan raises; n < window: one window at 0 of length n; (n - window) % hop != 0: one at
    n - window, pulled back to end at the last sample; otherwise none (at n == window the regular window 0 was due already).
    The due windows of all pushes plus the closing one are exactly window_plan(n, window, hop, min_samples)."""
    n, win, hop = int(n), int(window), int(hop)
    if not 1 <= hop <= win:
        raise ValueError(f'stream_finish: hop {hop} outside 1 .. window {win}')
    if n == 0:
        return None
    if n < max(int(min_samples), 1):
        raise ValueError(f'stream_finish: a stream of {n} samples is shorter than the {max(int(min_samples), 1)} the front end needs')
    if n < win:
        return 0, n
    if (n - win) % hop != 0:
        return n - win, win
    return None


def check_state_bytes(K, S):
    """the bytes of one fusion strategy's open-set state [K, S]; more than 1 GiB is refused"""
    nbytes = ops.stitch_stream_state_bytes(K, S)
    if nbytes > MAX_STATE_BYTES:
        raise ValueError(f'the open-set state of {K} thresholds x {S} streams takes {nbytes} bytes (> {MAX_STATE_BYTES}): pass fewer '
                         'thresholds or fewer streams per detector')
    return nbytes


def check_stream_depth(window, hop, sr, window_seconds, merge_gap=0.0):
    """the plan of a long stream decides D (recording.check_depth): regular starts w * hop, then a closing window one sample
    after the last regular one - the closest a pulled-back last window can follow"""
    last = (ops.STITCH_MAX_DEPTH + 1) * int(hop)
    starts = np.concatenate([np.arange(ops.STITCH_MAX_DEPTH + 2) * int(hop), [last + 1]])
    return check_depth(starts / float(sr), float(window_seconds), float(merge_gap), 'StreamDetector')


class StreamEvents(object):
    """one fusion strategy's events that became final in one push (or finish), per threshold of the decoder's grid.  onset / offset
    are float64 seconds from the start of the stream, score float32.  Rows: streams in order, then (onset, class).  ``status``
    [K, S]; ``tags`` (W, C) 0/1 of the windows the call processed (None without audio tagging) with ``tag_stream`` (W,) and
    ``tag_start`` (W,) seconds.  Built from the host copies of ops.stitch_stream's outputs; a raised status is an error here."""

    def __init__(self, labels, thresholds, names, emit, emit_count, status, tags=None, tag_stream=(), tag_start=()):
        self.labels = np.asarray(list(labels), dtype=object)
        self.thresholds = [operating_point(t) for t in thresholds]
        self.names = np.asarray(list(names), dtype=object)
        self.status = np.array(status, copy=True)
        self.tags = tags
        self.tag_stream, self.tag_start = np.asarray(tag_stream, np.int64), np.asarray(tag_start, np.float64)
        emit, count = np.asarray(emit), np.asarray(emit_count)
        K, S, cap = emit.shape[:3]
        bad = np.argwhere(self.status != 0)
        if len(bad):
            k, s = bad[0]
            raise RuntimeError(f'stitch_stream: stream {self.names[s]!r} at threshold {self.thresholds[k]}: status '
                               f'{int(self.status[k, s])} ({STATUS_REASONS.get(int(self.status[k, s]), "unknown")})')
        if (count > cap).any():
            k, s = np.argwhere(count > cap)[0]
            raise RuntimeError(f'stitch_stream: stream {self.names[s]!r} at threshold {self.thresholds[k]}: {int(count[k, s])} events, '
                               f'the emit buffer holds {cap}')
        times, score, n_merged, window, query, cls = ops.stitch_stream_views(emit)
        self._tables = []
        for k in range(K):
            live = np.arange(cap)[None, :] < count[k][:, None]                         # [S, cap]
            s, _ = np.nonzero(live)
            on, off, c = times[k][..., 0][live], times[k][..., 1][live], cls[k][live]
            order = np.lexsort((c, on, s))                                              # stream, then (onset, class)
            self._tables.append({'event_label': self.labels[c[order]], 'onset': on[order].copy(), 'offset': off[order].copy(),
                                 'score': score[k][live][order], 'filename': self.names[s[order]],
                                 'n_merged': n_merged[k][live][order], 'window': window[k][live][order],
                                 'query': query[k][live][order], 'cls': c[order].astype(np.int32), 'stream': s[order]})

    def __len__(self):
        return len(self.thresholds)

    def at(self, k=0):
        """the column arrays at threshold k (a dict: COLUMNS with the stream's name as filename, n_merged, window, query, cls, stream)"""
        return self._tables[k]

    def to_rows(self, k=0):
        """[(event_label, onset, offset, score, stream_name)] with Python floats"""
        t = self._tables[k]
        return list(zip(*[t[c].tolist() for c in COLUMNS]))

    def tag_rows(self):
        """[(event_label, stream_name, window start)] for every tag that is 1, windows in order, classes ascending"""
        if self.tags is None:
            return []
        w, c = np.nonzero(self.tags == 1)
        return [(self.labels[j], self.names[self.tag_stream[i]], float(self.tag_start[i])) for i, j in zip(w.tolist(), c.tolist())]


class StreamDetector(object):
    """model, postprocessor, decoder, mel, transform, window_seconds, hop_seconds, merge_gap, at, threshold, graphed: as
    utilities.recording.RecordingDetector, with the same checks; ``n_streams`` streams (``names``: theirs, default '0', '1', ..)
    are the batch of the detect step, B = n_streams (B = 2 with a zero row for a single stream: the step takes no batch of one).  Every stream owns a ring of 2 * window samples on the device.

    ``push(chunks, streams=None)`` takes one 1-D float32 / int16 chunk (host or device, any length, 0 included) per named stream
    (None: all, in order) and returns a handle whose ``result()`` is {at_m: StreamEvents}: the events that became final.  The chunks
    go through one pinned buffer and one host-to-device copy and are appended in pieces of at most a window, so a ring never holds
    more than it can; after every piece, rounds run while any stream has a due window: one ops.stream_cut launch fills the (B, window)
    input (a stream without a due window has a zero row and action 0), mel + box transform write the graph's static input, one
    GraphedDetectStep replay, one ops.stitch_stream launch per fusion strategy.  Nothing is read back between rounds; the call ends
    with asynchronous copies of emit, emit_count, status and the rounds' audio tags into a ring of two pinned slots.
    ``finish(streams=None)`` ends the named streams: the closing window (stream_finish), if any, is processed and everything open
    is handed out; the streams' rings and state are reset, so a stream can start again at time 0.

    Duration policy: a regular window is clipped against dur = (start + window) / sr - what the offline path would pass if the
    recording ended there; the closing window against n / sr.  A stream then equals RecordingDetector on the whole recording whenever
    t_w + window_seconds <= dur holds in float64 for every regular window: always when window and hop are exact in binary at the
    sample rate, for example whole seconds at 16 kHz.

    Out of scope: ``sample_rates=`` (a streaming resampler needs filter state across chunks: streams arrive mono at mel.sr) and
    ``metrics=`` (streams are not scored)."""

    def __init__(self, model, postprocessor, decoder, mel, transform, window_seconds, hop_seconds, n_streams, names=None, merge_gap=0.0,
                 at=True, threshold=0.5, graphed=True):
        S = int(n_streams)
        if S < 1:
            raise ValueError(f'StreamDetector: n_streams {n_streams} (>= 1)')
        self.names = [str(i) for i in range(S)] if names is None else list(names)
        if len(self.names) != S or len(set(self.names)) != S:
            raise ValueError(f'StreamDetector: {S} distinct names expected, one per stream')
        window, hop = int(round(float(window_seconds) * mel.sr)), int(round(float(hop_seconds) * mel.sr))
        if 1 <= hop <= window and 0.0 <= float(merge_gap) < float('inf') and float(window_seconds) == decoder.max_len:
            check_stream_depth(window, hop, mel.sr, window_seconds, merge_gap)         # before anything is allocated
        check_state_bytes(decoder.K, S)
        # the front end, the step and the argument checks are the recording detector's, with the streams as its batch
        self.B = max(S, 2)                              # the detect step takes no batch of one: a single stream has a zero row beside it
        self._rd = rd = RecordingDetector(model, postprocessor, decoder, mel, transform, window_seconds, hop_seconds, batch_windows=self.B,
                                          merge_gap=merge_gap, at=at, threshold=threshold, graphed=graphed)
        self.S, self.decoder, self.mel, self.dev = S, decoder, mel, rd.dev
        self.window, self.hop, self.merge_gap = rd.window, rd.hop, rd.merge_gap
        self.window_seconds = rd.window_seconds
        self.ring_samples = 2 * self.window
        self.ring = torch.zeros((S, self.ring_samples), dtype=torch.float32, device=self.dev)
        self.state = {m: ops.stitch_stream_state(decoder.K, S, self.dev) for m in decoder.fusion}
        self.received = np.zeros(S, np.int64)          # samples pushed so far, per stream
        self.done = np.zeros(S, np.int64)              # regular windows processed so far
        self.keep_records = False                      # a test hook: keep every round's records in ``kept``
        self.kept = []
        self._host, self._serial = None, 0

    # ------------------------------------------------------------------ the host half
    def _indices(self, streams):
        if streams is None:
            return list(range(self.S))
        idx = [self.names.index(s) if not isinstance(s, (int, np.integer)) else int(s) for s in streams]
        if len(set(idx)) != len(idx) or any(not 0 <= i < self.S for i in idx):
            raise ValueError(f'StreamDetector: streams {list(streams)!r}: distinct streams of this detector expected')
        return idx

    def schedule(self, idx, lengths):
        """the whole push on the host, before the first launch: [(append jobs [(stream, ring position, source offset, n)], rounds)],
        a round being [(stream, start sample, window index)] - one window per stream at the most"""
        received, done = self.received.copy(), self.done.copy()
        left, src = [int(n) for n in lengths], np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        phases = []
        while any(left):
            jobs, due = [], {}
            for j, s in enumerate(idx):
                n = min(left[j], self.window)                  # a piece: what the ring held back is shorter than a window
                if n:
                    jobs.append((s, int(received[s] % self.ring_samples), int(src[j + 1]) - left[j], n))
                    due[s] = list(stream_plan(received[s], received[s] + n, self.window, self.hop))
                    received[s] += n
                    left[j] -= n
            rounds = []
            while any(due.values()):
                rounds.append([(s, int(d.pop(0)), int(done[s])) for s, d in due.items() if d])
                for s, _, _ in rounds[-1]:
                    done[s] += 1
            phases.append((jobs, rounds))
        return phases, received, done

    # ------------------------------------------------------------------ the device half
    def _stage(self, chunks):
        """the chunks as ONE float32 device vector (recording.stage_recordings: one pinned buffer, one copy; int16 widened x / 32768)"""
        from .recording import stage_recordings
        return stage_recordings(chunks, self.dev)

    def _round(self, cut, rows, emit, emit_count, tags, r):
        """one round: ``cut`` [(stream, ring position, length)], ``rows`` {stream: (action, t_w, dur, window index)}"""
        rd, S, up = self._rd, self.S, self._rd._up
        ints = np.zeros((4 + 3) * S, np.int32)
        jobs = np.asarray([(s, p, n, s) for s, p, n in cut], np.int32).reshape(-1, 4)
        ints[:jobs.size] = jobs.reshape(-1)
        f64 = np.zeros(2 * S, np.float64)
        for s, (a, t, d, w) in rows.items():
            ints[4 * S + s], ints[5 * S + s], ints[6 * S + s] = a, s, w
            f64[s], f64[S + s] = t, d
        d_int, d_f64 = up('stream_int', ints), up('stream_f64', f64)
        if len(cut):
            ops.stream_cut(self.ring, jobs, d_int[:4 * S], rd.wave)
            lengths = [self.window] * self.B
            for s, _, n in cut:
                lengths[s] = n
            amp, nframes = self.mel(rd.wave, lengths=lengths, out=rd.amp)
            x = rd.transform(amp, nframes=nframes, out=getattr(rd, 'x', None))
            _, _, (dev_rec, dev_tags) = rd._detect(x)
            self._last = dev_rec, dev_tags
            if tags is not None:
                tags[r].copy_(dev_tags[:S], non_blocking=True)
        dev_rec, _ = self._last
        if self.keep_records:
            self.kept.append(({m: dev_rec['dev'][m].clone() for m in self.decoder.fusion}, dict(rows)))
        for m in self.decoder.fusion:
            state, status = self.state[m]
            ops.stitch_stream(dev_rec['dev'][m], d_int[4 * S:5 * S], d_int[5 * S:6 * S], d_f64[:S], d_f64[S:], d_int[6 * S:],
                              self.decoder.C, self.merge_gap, state, emit[m], emit_count[m], status)

    def _run(self, rounds_total, body, tag_rows):
        """allocate the call's outputs, run ``body(emit, emit_count, tags)``, queue the copies to the host and return the handle"""
        K, S, dec = self.decoder.K, self.S, self.decoder
        cap = max(rounds_total, 1) * ops.STREAM_OPEN
        emit = {m: torch.zeros((K, S, cap, ops.STREAM_EMIT_WORDS), dtype=torch.int32, device=self.dev) for m in dec.fusion}
        emit_count = {m: torch.zeros((K, S), dtype=torch.int32, device=self.dev) for m in dec.fusion}
        n_tags = max(rounds_total, 1)                   # one [S, C] block of tags per round
        tags = torch.zeros((n_tags, S, dec.C), dtype=torch.int64, device=self.dev) if self._rd.at else None
        body(emit, emit_count, tags)
        ring = self._host
        if ring is None or ring['cap'] < cap or ring['tags'] < n_tags:
            pin = lambda n, dt: torch.empty(n, dtype=dt).pin_memory()
            ring = self._host = {'cap': cap, 'tags': n_tags, 'k': 0, 'event': [None] * 2, 'serial': [-1] * 2,
                                 'emit': [{m: pin(emit[m].numel(), torch.int32) for m in dec.fusion} for _ in range(2)],
                                 'small': [{m: pin(2 * K * S, torch.int32) for m in dec.fusion} for _ in range(2)],
                                 'tagbuf': [pin(n_tags * S * dec.C, torch.int64) for _ in range(2)]}
        k = ring['k']
        ring['k'] = (k + 1) % 2
        if ring['event'][k] is not None:
            ring['event'][k].synchronize()
        for m in dec.fusion:
            ring['emit'][k][m][:emit[m].numel()].copy_(emit[m].reshape(-1), non_blocking=True)
            ring['small'][k][m][:K * S].copy_(emit_count[m].reshape(-1), non_blocking=True)
            ring['small'][k][m][K * S:].copy_(self.state[m][1].reshape(-1), non_blocking=True)
        if tags is not None and tag_rows:
            ring['tagbuf'][k][:tags.numel()].copy_(tags.reshape(-1), non_blocking=True)
        ring['event'][k] = torch.cuda.Event()
        ring['event'][k].record()
        self._serial += 1
        ring['serial'][k] = self._serial
        return PendingStream(self, ring, k, self._serial, cap, tag_rows, tags is not None)

    def push(self, chunks, streams=None):
        idx = self._indices(streams)
        chunks = list(chunks)
        if len(chunks) != len(idx):
            raise ValueError(f'StreamDetector.push: {len(chunks)} chunks for {len(idx)} streams')
        if any(getattr(c, 'ndim', 1) != 1 for c in chunks):
            raise ValueError('StreamDetector.push: mono chunks expected, every one 1-D')
        lengths = [int(c.shape[0]) for c in chunks]
        phases, received, done = self.schedule(idx, lengths)
        sr = float(self.mel.sr)
        all_rounds = [rnd for _, rounds in phases for rnd in rounds]

        def body(emit, emit_count, tags):
            flat, _, _, host = self._stage(chunks) if phases else (None, None, None, None)
            r = 0
            for jobs, rounds in phases:
                h = np.asarray(jobs, np.int32).reshape(-1, 4)
                ops.stream_append(flat, h, self._rd._up('stream_append', h), self.ring)
                for rnd in rounds:
                    cut = [(s, start % self.ring_samples, self.window) for s, start, _ in rnd]
                    rows = {s: (ADD, start / sr, (start + self.window) / sr, w) for s, start, w in rnd}
                    self._round(cut, rows, emit, emit_count, tags, r)
                    r += 1
            self._keep = (flat, host)                  # the staged chunks live until the copies behind them have run
        # the tags of a round are kept per round [S, C]: a window's are those of (round, stream)
        tag_rows = [(r, s, start / sr) for r, rnd in enumerate(all_rounds) for s, start, _ in rnd] if self._rd.at else []
        handle = self._run(len(all_rounds), body, tag_rows)
        self.received, self.done = received, done
        return handle

    def finish(self, streams=None):
        idx = self._indices(streams)
        sr = float(self.mel.sr)
        closing = {s: stream_finish(self.received[s], self.window, self.hop, self.mel.min_samples) for s in idx}     # may refuse
        cut, rows = [], {}
        for s in idx:
            n = int(self.received[s])
            if closing[s] is None:
                rows[s] = (FLUSH, 0.0, 0.0, 0)
            else:
                start, length = closing[s]
                cut.append((s, start % self.ring_samples, length))
                rows[s] = (ADD_FLUSH, start / sr, n / sr, int(self.done[s]))
        which = np.zeros(self.S, np.int32)
        which[idx] = 1

        def body(emit, emit_count, tags):
            if not cut and not hasattr(self, '_last'):
                return                                  # nothing was ever detected: nothing is open
            self._round(cut, rows, emit, emit_count, tags, 0)
        handle = self._run(1, body, [(0, s, closing[s][0] / sr) for s, _, _ in cut] if self._rd.at else [])
        d_which = self._rd._up('stream_which', which)
        for m in self.decoder.fusion:
            ops.stream_reset(self.state[m][0], self.state[m][1], d_which)
        self.received[idx] = 0
        self.done[idx] = 0
        return handle


class PendingStream(object):
    """the results of one push / finish on their way to the host"""

    def __init__(self, det, ring, slot, serial, cap, tag_rows, has_tags):
        self._det, self._ring, self._slot, self._serial = det, ring, slot, serial
        self.cap, self.tag_rows, self.has_tags = cap, tag_rows, has_tags

    def result(self):
        """wait for the copies, then {at_m: StreamEvents}: copies, the ring slot is free afterwards"""
        r, k, det = self._ring, self._slot, self._det
        dec, K, S = det.decoder, det.decoder.K, det.S
        if r['serial'][k] != self._serial:
            raise RuntimeError('StreamDetector: this call\'s host buffers were reused by a later push(); ask for result() within two '
                               'calls')
        r['event'][k].synchronize()
        det._keep = None
        tags = None
        if self.has_tags:
            n_rounds = 1 + max((t[0] for t in self.tag_rows), default=-1)
            per_round = r['tagbuf'][k].numpy()[:n_rounds * S * dec.C].reshape(n_rounds, S, dec.C)
            tags = np.stack([per_round[rr, s] for rr, s, _ in self.tag_rows]) if self.tag_rows else np.zeros((0, dec.C), np.int64)
        out = {}
        for m in dec.fusion:
            emit = r['emit'][k][m].numpy()[:K * S * self.cap * ops.STREAM_EMIT_WORDS].reshape(K, S, self.cap, ops.STREAM_EMIT_WORDS)
            small = r['small'][k][m].numpy()
            out[m] = StreamEvents(dec.labels, dec.threshold_values, det.names, emit.copy(), small[:K * S].reshape(K, S).copy(),
                                  small[K * S:].reshape(K, S).copy(), tags, [s for _, s, _ in self.tag_rows],
                                  [t for _, _, t in self.tag_rows])
        return out
