"""Sound events in recordings of any length.  The reference scores 10 s dataset clips only; here a recording is cut into overlapping
windows of the clip length the model was trained on, every window goes through the target-free predict step
(engine.GraphedDetectStep: forward, audio tags, PostProcess, ops.decode_events), and the windows' event records are stitched on
the device into one event list per recording (ops.stitch_events, csrc/stitch.hip): an event a window boundary cut in two, or one
that two overlapping windows both report, becomes one event.  DESIGN.md section 4 ("Recordings of any length") holds the definition.

    detector = RecordingDetector(model, postprocessor, decoder, mel, transform, window_seconds=10.0, hop_seconds=5.0)
    predictions, tags = detector([wave], ['street.wav'])           # {at_m: RecordingPredictions}, WindowTags
    predictions[1].write_tsv('street.tsv')                         # event_label, onset, offset, score, filename

``window_plan`` and ``open_depth`` are the host half and need no GPU."""
import numpy as np
import torch

from .. import ops
from .predictions import COLUMNS, operating_point
from .scoring import Uploads

MAX_OUTPUT_BYTES = 1 << 30        # the stitched event buffer of one fusion strategy
DEFAULT_CAP = 4096


def window_plan(n_samples, window_samples, hop_samples, min_samples=1):
    """the start samples (int64, ascending) of the windows a recording of ``n_samples`` is cut into, 1 <= hop <= window.
    n <= window: one window at 0 (n samples long; PadOrTrunc pads it as it pads a short dataset clip).  Otherwise
    1 + ceil((n - window) / hop) full windows at min(w * hop, n - window): the last one is pulled back to end at the last sample.
    A recording shorter than ``min_samples`` (the mel front end's n_fft/2 + 1) is refused."""
    n, win, hop = int(n_samples), int(window_samples), int(hop_samples)
    if not 1 <= hop <= win:
        raise ValueError(f'window_plan: hop {hop} outside 1 .. window {win}')
    if n < max(int(min_samples), 1):
        raise ValueError(f'window_plan: a recording of {n} samples is shorter than the {max(int(min_samples), 1)} the front end needs')
    if n <= win:
        return np.zeros(1, np.int64)
    count = 1 + -(-(n - win) // hop)
    return np.minimum(np.arange(count, dtype=np.int64) * hop, n - win)


def open_depth(win_start, window_seconds, merge_gap=0.0):
    """D of a recording's plan: the largest number of earlier windows w' with t_w' + window + merge_gap >= t_w over its windows w -
    the windows whose events may still be open when window w is reached (``win_start`` ascending, seconds)"""
    t = np.asarray(win_start, np.float64)
    reach = t + float(window_seconds) + float(merge_gap)
    return max([int(np.count_nonzero(reach[:w] >= t[w])) for w in range(len(t))], default=0)


def check_depth(win_start, window_seconds, merge_gap=0.0, what='the plan'):
    d = open_depth(win_start, window_seconds, merge_gap)
    if d > ops.STITCH_MAX_DEPTH:
        raise ValueError(f'{what}: {d} earlier windows can still hold open events when a window starts, the stitch kernel keeps '
                         f'{ops.STITCH_MAX_DEPTH}: use a longer hop (window / {ops.STITCH_MAX_DEPTH} at the least) or a smaller merge_gap')
    return d


def check_output_bytes(K, R, C, cap):
    """the bytes of one fusion strategy's stitched event buffer [K, R, C, cap, 8 words]; more than 1 GiB is refused"""
    nbytes = int(K) * int(R) * int(C) * int(cap) * ops.STITCH_WORDS * 4
    if nbytes > MAX_OUTPUT_BYTES:
        raise ValueError(f'the stitched event buffer of {K} thresholds x {R} recordings x {C} classes x cap {cap} takes {nbytes} bytes '
                         f'(> {MAX_OUTPUT_BYTES}): pass a smaller cap, fewer thresholds or fewer recordings per call')
    return nbytes


def stage_resampled(waves, sample_rates, resampler, dev):
    """stage_recordings for recordings at their own sample rates, 1-D or interleaved (frames, channels); ``resampler``: rate -> the
    DeviceResampler from that rate to the model's (kept by the caller).  Grouped by rate, every group ONE
    sedt_resample launch that down-mixes, converts to mel.sr and writes straight into the flat vector at the recordings'
    offsets (a recording already at mel.sr goes through the identity plan).  Lengths and offsets are the resampled ones."""
    rates = [int(sample_rates)] * len(waves) if np.ndim(sample_rates) == 0 else [int(r) for r in sample_rates]
    if len(rates) != len(waves):
        raise ValueError('sample_rates: one rate, or one per recording')
    groups = {}
    for i, r in enumerate(rates):
        groups.setdefault(r, []).append(i)
    staged, ns = {}, [0] * len(waves)
    for r, idx in groups.items():
        rs = resampler(r)
        clips, pins = rs.stage([waves[i] for i in idx])
        staged[r] = (rs, clips, pins)
        for i, (_, n, _) in zip(idx, clips):
            ns[i] = rs.n_out(n)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    flat = torch.empty(max(int(off[-1]), 1), dtype=torch.float32, device=dev)
    for r, idx in groups.items():
        rs, clips, _ = staged[r]
        rs.launch(clips, flat, [int(off[i]) for i in idx], [ns[i] for i in idx])
    return flat, off, ns, [(clips, pins) for _, clips, pins in staged.values()]     # the raw input lives as long as the flat vector


def stage_recordings(waves, dev):
    """the recordings as ONE float32 device vector (every recording 4-byte aligned by construction) and their sample offsets.
    Host waveforms go through one pinned buffer; int16 PCM is widened as the mel kernel widens it (x / 32768, exact).
    Returns (flat, offsets int64 [R + 1], samples per recording, what must stay alive until the copies have run).
    Shared by RecordingDetector and recording_clips.RecordingClips."""
    ns = [int(w.shape[0]) for w in waves]
    if any(getattr(w, 'ndim', 1) != 1 for w in waves):
        raise ValueError('mono waveforms expected: every recording 1-D (pass sample_rates= to down-mix and resample on the device)')
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    flat = torch.empty(max(int(off[-1]), 1), dtype=torch.float32, device=dev)
    host = None
    if any(not (torch.is_tensor(w) and w.is_cuda) for w in waves):
        host = torch.empty(max(int(off[-1]), 1), dtype=torch.float32).pin_memory()
    for i, w in enumerate(waves):
        dst = slice(int(off[i]), int(off[i + 1]))
        if torch.is_tensor(w) and w.is_cuda:
            flat[dst] = w.float() * (1.0 / 32768.0) if w.dtype == torch.int16 else w.float()
        else:
            a = w.numpy() if torch.is_tensor(w) else np.asarray(w)
            if a.dtype == np.int16:
                a = a.astype(np.float32) * np.float32(1.0 / 32768.0)
            elif a.dtype != np.float32:
                raise ValueError(f'waveforms are float32 or int16, got {a.dtype}')
            host.numpy()[dst] = a
    if host is not None:
        for i, w in enumerate(waves):
            if not (torch.is_tensor(w) and w.is_cuda):
                dst = slice(int(off[i]), int(off[i + 1]))
                flat[dst].copy_(host[dst], non_blocking=True)
    return flat, off, ns, host


class WindowTags(object):
    """the audio tags of every window of a call with the window table: ``tags`` (W, C) 0/1 (None without audio tagging),
    ``recording`` (W,) index into ``filenames``, ``start`` (W,) float64 seconds"""

    def __init__(self, tags, recording, start, filenames, labels):
        self.tags, self.recording, self.start = tags, recording, start
        self.filenames, self.labels = list(filenames), list(labels)

    def __len__(self):
        return len(self.start)

    def to_rows(self):
        """[(event_label, filename, window start)] for every tag that is 1, windows in order, classes ascending"""
        if self.tags is None:
            return []
        w, c = np.nonzero(self.tags == 1)
        return [(self.labels[j], self.filenames[self.recording[i]], float(self.start[i])) for i, j in zip(w.tolist(), c.tolist())]


class RecordingPredictions(object):
    """one fusion strategy's events over the recordings of a call, per threshold of the decoder's grid: the column arrays of the
    reference's prediction frame (event_label, onset, offset, score, filename) plus n_merged, window and query.  onset / offset are
    float64 seconds from the start of the recording, score float32.  Rows: recordings in order, then (onset, class).
    Built from the host copies of ops.stitch_events' outputs; a list that overflowed ``cap`` or a raised status is an error here."""

    def __init__(self, labels, thresholds, filenames, count, out, status, cap):
        self.labels = np.asarray(list(labels), dtype=object)
        self.thresholds = [operating_point(t) for t in thresholds]
        self.filenames = np.asarray(list(filenames), dtype=object)
        count, status = np.asarray(count), np.asarray(status)
        K, R, C = count.shape
        bad = np.argwhere(status != 0)
        if len(bad):
            k, r = bad[0]
            why = {1: 'its window starts are not ascending', 2: 'more events were open at once than the stitch kernel holds: use a '
                   'longer hop or a smaller merge_gap', 4: 'a window record holds an event with a negative onset: decode with a finite '
                   'max_len', 8: 'its window range is not inside the window table'}.get(int(status[k, r]), 'unknown')
            raise RuntimeError(f'stitch_events: recording {self.filenames[r]!r} at threshold {self.thresholds[k]}: status '
                               f'{int(status[k, r])} ({why})')
        over = np.argwhere(count > cap)
        if len(over):
            k, r, c = over[0]
            raise RuntimeError(f'stitch_events: recording {self.filenames[r]!r}, class {self.labels[c]!r}, threshold {self.thresholds[k]}: '
                               f'{int(count[k, r, c])} merged events, the output holds cap = {cap}: pass cap >= {int(count.max())}')
        times, score, n_merged, window, query = ops.stitch_events_views(np.asarray(out))
        self._tables = []
        for k in range(K):
            live = np.arange(cap)[None, None, :] < count[k][:, :, None]                 # [R, C, cap]
            r, c, _ = np.nonzero(live)
            on, off = times[k][..., 0][live], times[k][..., 1][live]
            order = np.lexsort((c, on, r))                                              # recording, then (onset, class)
            self._tables.append({'event_label': self.labels[c[order]], 'onset': on[order].copy(), 'offset': off[order].copy(),
                                 'score': score[k][live][order], 'filename': self.filenames[r[order]],
                                 'n_merged': n_merged[k][live][order], 'window': window[k][live][order],
                                 'query': query[k][live][order], 'cls': c[order].astype(np.int32), 'recording': r[order]})

    def __len__(self):
        return len(self.thresholds)

    def at(self, k=0):
        """the column arrays at threshold k (a dict: COLUMNS, n_merged, window, query, cls, recording)"""
        return self._tables[k]

    def to_rows(self, k=0):
        """[(event_label, onset, offset, score, filename)] with Python floats"""
        t = self._tables[k]
        return list(zip(*[t[c].tolist() for c in COLUMNS]))

    def to_dataframe(self, k=0):
        import pandas as pd
        t = self._tables[k]
        return pd.DataFrame({c: t[c] for c in COLUMNS + ('n_merged',)}, columns=list(COLUMNS + ('n_merged',)))

    def write_tsv(self, path, k=0):
        """the rows at threshold k with the reference's columns, tab-separated (floats in their shortest round-trip form)"""
        t = self._tables[k]
        with open(path, 'w') as f:
            f.write('\t'.join(COLUMNS) + '\n')
            for lab, on, off, sc, name in zip(*[t[c] for c in COLUMNS]):
                f.write(f'{lab}\t{repr(float(on))}\t{repr(float(off))}\t{str(sc)}\t{name}\n')


class RecordingDetector(object):
    """model, postprocessor (PostProcess), decoder (predictions.EventDecoder with max_len_seconds = window_seconds), mel
    (DeviceMelSpectrogram), transform (DeviceBoxTransform without augmentation, its frames = the model's clip length).
    ``window_seconds`` is the decoder's max_len and the orig_size of every window; ``hop_seconds`` the distance of window starts;
    ``batch_windows`` the windows per replay; ``merge_gap`` seconds: events of a class this close are one event; ``cap`` the events
    per (threshold, recording, class) the output holds (default min(4096, windows * Q)).

    A call takes a list of 1-D float32 / int16 waveforms (host or device) at mel.sr - or, with ``sample_rates``, recordings at any rate,
    mono or interleaved (frames, channels), resampled on the device at ``resample_quality`` - and their names and returns ({at_m: RecordingPredictions},
    WindowTags).  Per batch of windows: one strided copy launch cuts the windows out of the recordings (ops.copy2d: src stride = hop,
    dst stride = window), mel + box transform write the graph's static input, one GraphedDetectStep replay, one more copy2d launch
    per fusion strategy appends the batch's valid rows to the call's record buffer - nothing is read back between batches.  Then one
    ops.stitch_events launch per fusion strategy and one asynchronous copy of counts, lists, status and tags into a ring of pinned
    host buffers (``submit`` returns the handle, a call is ``submit(...).result()``)."""

    def __init__(self, model, postprocessor, decoder, mel, transform, window_seconds, hop_seconds, batch_windows=8, merge_gap=0.0, cap=None,
                 at=True, threshold=0.5, graphed=True, resample_quality='kaiser_best'):
        if float(window_seconds) != decoder.max_len:
            raise ValueError(f'RecordingDetector: window_seconds {window_seconds} is not the decoder\'s max_len_seconds {decoder.max_len}: '
                             'the events of a window are clipped to the window')
        if any((transform.time_mask, transform.freq_mask, transform.freq_shift)):
            raise ValueError('RecordingDetector: the transform augments; build DeviceBoxTransform without time_mask / freq_mask / freq_shift')
        self.model, self.post, self.decoder, self.mel, self.transform = model, postprocessor, decoder, mel, transform
        self.window_seconds, self.hop_seconds = float(window_seconds), float(hop_seconds)
        self.window = int(round(self.window_seconds * mel.sr))
        self.hop = int(round(self.hop_seconds * mel.sr))
        if not 1 <= self.hop <= self.window:
            raise ValueError(f'RecordingDetector: hop_seconds {hop_seconds} outside (0, window_seconds {window_seconds}]')
        self.merge_gap = float(merge_gap)
        if not (0.0 <= self.merge_gap < float('inf')):
            raise ValueError(f'RecordingDetector: merge_gap {merge_gap} is not a finite number >= 0')
        self.B, self.cap, self.at, self.threshold, self.graphed = int(batch_windows), cap, at, threshold, graphed
        self.dev = decoder.device
        # the plan of a long recording decides D; a short one has fewer windows and no more
        check_depth(np.arange(ops.STITCH_MAX_DEPTH + 2) * (self.hop / mel.sr), self.window_seconds, self.merge_gap, 'RecordingDetector')
        self.wave = torch.zeros((self.B, self.window), dtype=torch.float32, device=self.dev)
        self.amp = torch.zeros((self.B, 1 + self.window // mel.hop, mel.F), dtype=torch.float32, device=self.dev)
        self.sizes = torch.full((self.B,), self.window_seconds, dtype=torch.float32, device=self.dev)
        self.step = None
        self._up, self._host, self._serial, self._keep = Uploads(self.dev), None, 0, None
        self.resample_quality, self._resamplers = resample_quality, {}

    # ------------------------------------------------------------------ pieces
    def plan(self, lengths):
        """(win_off [R + 1] int32, start samples [W] int64, win_start [W] float64 seconds, rec_dur [R] float64 seconds)"""
        starts = [window_plan(n, self.window, self.hop, self.mel.min_samples) for n in lengths]
        off = np.concatenate([[0], np.cumsum([len(s) for s in starts])]).astype(np.int32)
        start = np.concatenate(starts) if starts else np.zeros(0, np.int64)
        t = start.astype(np.float64) / float(self.mel.sr)
        for r in range(len(lengths)):
            check_depth(t[off[r]:off[r + 1]], self.window_seconds, self.merge_gap, f'recording {r}')
        return off, start, t, np.asarray(lengths, np.float64) / float(self.mel.sr)

    def resampler(self, rate):
        """the DeviceResampler from ``rate`` to mel.sr, made at first use and kept (its table stays on the device)"""
        rs = self._resamplers.get(int(rate))
        if rs is None:
            from .resample import DeviceResampler
            rs = self._resamplers[int(rate)] = DeviceResampler(int(rate), self.mel.sr, self.resample_quality, device=self.dev)
        return rs

    def _stage_resampled(self, waves, sample_rates):
        """_stage for recordings at their own sample rates: stage_resampled with this detector's resamplers"""
        return stage_resampled(waves, sample_rates, self.resampler, self.dev)

    def _stage(self, waves, sample_rates=None):
        """the recordings as ONE float32 device vector and their sample offsets (stage_recordings; with ``sample_rates``:
        _stage_resampled)"""
        if sample_rates is not None:
            return self._stage_resampled(waves, sample_rates)
        return stage_recordings(waves, self.dev)

    def _cut_jobs(self, flat, rec_off, ns, win_off, start, lo, hi):
        """the copy2d jobs that fill rows 0 .. hi - lo - 1 of self.wave with windows lo .. hi - 1: runs of windows of one recording a
        hop apart are one job (src stride = hop, dst stride = window)"""
        jobs, w = [], lo
        rec = np.searchsorted(win_off, np.arange(lo, hi), side='right') - 1
        while w < hi:
            r, e = rec[w - lo], w + 1
            while e < hi and rec[e - lo] == r and start[e] - start[e - 1] == self.hop:
                e += 1
            src = flat.data_ptr() + 4 * (int(rec_off[r]) + int(start[w]))
            dst = self.wave.data_ptr() + 4 * (w - lo) * self.window
            jobs.append((src, dst, e - w, 4 * min(self.window, ns[r]), 4 * self.hop, 4 * self.window))
            w = e
        return jobs

    def _detect(self, x):
        from .. import engine
        if not self.graphed:
            return engine.detect_step(self.model, self.post, x, self.sizes, self.decoder.fusion, self.at, self.threshold, self.decoder)
        if self.step is None:
            self.step = engine.GraphedDetectStep(self.model, self.post, x, self.sizes, self.decoder.fusion, self.at, self.threshold,
                                                 self.decoder)
            self.x = self.step.static_x
            return self.step(None)                      # the warm-up ran on this batch; the replay fills the outputs from it
        return self.step(None if x is self.step.static_x else x)

    # ------------------------------------------------------------------ the call
    def records(self, waves, sample_rates=None):
        """windows -> the per-window event records: ({at_m: int32 [K, W, 1 + 5 Q] on the device}, tags (W, C) int64 on the device or
        None, plan) - what ``stitch`` takes.  sample_rates: see submit()"""
        flat, rec_off, ns, _host = self._stage(waves, sample_rates)
        plan = self.plan(ns)
        win_off, start, _, _ = plan
        W, K, fusion = len(start), self.decoder.K, self.decoder.fusion
        rec, tags, x = None, None, getattr(self, 'x', None)
        for lo in range(0, W, self.B):
            hi = min(lo + self.B, W)
            nv = hi - lo
            if nv < self.B:
                self.wave[nv:].zero_()                  # a short last batch: zero windows behind the valid ones
            ops.copy2d(self._cut_jobs(flat, rec_off, ns, win_off, start, lo, hi))
            rcd = np.searchsorted(win_off, np.arange(lo, hi), side='right') - 1
            lengths = [min(self.window, ns[r]) for r in rcd] + [self.window] * (self.B - nv)
            amp, nframes = self.mel(self.wave, lengths=lengths, out=self.amp)
            x = self.transform(amp, nframes=nframes, out=x)
            t, _, dec = self._detect(x)
            x = getattr(self, 'x', x)
            dev_rec, dev_tags = dec
            Q = dev_rec['Q']
            if rec is None:
                row = 1 + 5 * Q
                rec = {m: torch.empty((K, W, row), dtype=torch.int32, device=self.dev) for m in fusion}
                tags = torch.empty((W, self.decoder.C), dtype=torch.int64, device=self.dev) if dev_tags is not None else None
            jobs = [(dev_rec['dev'][m].data_ptr(), rec[m].data_ptr() + 4 * lo * row, K, 4 * nv * row, 4 * self.B * row, 4 * W * row)
                    for m in fusion]
            if tags is not None:
                jobs.append((dev_tags.data_ptr(), tags.data_ptr() + 8 * lo * self.decoder.C, 1, 8 * nv * self.decoder.C, 0, 0))
            ops.copy2d(jobs)
        self._keep = (flat, _host)                      # the staged recordings stay alive until the work queued on them has run
        return rec, tags, plan

    def stitch(self, rec, plan):
        """one launch per fusion strategy: {at_m: (count, out, status) on the device} and cap"""
        win_off, start, t, dur = plan
        R, W = len(dur), len(start)
        Q = (next(iter(rec.values())).shape[2] - 1) // 5
        cap = int(self.cap) if self.cap is not None else min(DEFAULT_CAP, max(int(np.diff(win_off).max(initial=1)), 1) * Q)
        check_output_bytes(self.decoder.K, R, self.decoder.C, cap)
        d_off = self._up('off', win_off)
        d_t = self._up('t', t)
        d_dur = self._up('dur', dur)
        res = {m: ops.stitch_events(rec[m], d_off, d_t, d_dur, self.decoder.C, self.merge_gap, cap, n_windows=W) for m in rec}
        return res, cap

    def submit(self, waves, filenames, sample_rates=None, metrics=None):
        """everything of a call enqueued on the current stream, the copies of counts, lists, status and tags into the next slot of a ring
        of pinned host buffers included (as EventDecoder.fetch: a slot is reused only after its copies have finished).  Returns the
        handle whose ``result()`` waits for them: submit the next call before asking for this one's result and the host formatting
        runs beside the device.  ``sample_rates`` (one int, or one per recording): the recordings are at these rates and may be
        interleaved (frames, channels); they are down-mixed and resampled to mel.sr on the device (utilities/resample.py, one launch
        per distinct rate), and window plan, durations and event times follow from the resampled lengths.  None: the recordings
        are mono and at mel.sr already.  ``metrics`` (a utilities.recording_metrics.RecordingMetrics with its reference set): the
        stitched lists are scored against the annotations where they lie - ``metrics.update`` is enqueued right after the stitch
        launches, on the same stream, and reads nothing back."""
        waves, filenames = list(waves), list(filenames)
        if len(waves) != len(filenames) or not waves:
            raise ValueError('RecordingDetector: one name per recording, at least one recording')
        rec, tags, plan = self.records(waves, sample_rates)
        res, cap = self.stitch(rec, plan)
        if metrics is not None:
            metrics.update(res, cap, filenames, durations=plan[3])
        key = (len(filenames), len(plan[1]), cap, tags is not None)
        ring = self._host if self._host is not None and self._host['key'] == key else None
        if ring is None:                                # another shape: a new ring (a handle still out keeps its own alive)
            pin = lambda t: torch.empty(t.shape, dtype=t.dtype).pin_memory()
            ring = self._host = {'key': key, 'k': 0, 'event': [None] * 2, 'serial': [-1] * 2,
                                 'res': [{m: tuple(pin(t) for t in res[m]) for m in res} for _ in range(2)],
                                 'tags': [None if tags is None else pin(tags) for _ in range(2)]}
        k = ring['k']
        ring['k'] = (k + 1) % 2
        if ring['event'][k] is not None:
            ring['event'][k].synchronize()
        for m in res:
            for dst, src in zip(ring['res'][k][m], res[m]):
                dst.copy_(src, non_blocking=True)
        if tags is not None:
            ring['tags'][k].copy_(tags, non_blocking=True)
        ring['event'][k] = torch.cuda.Event()
        ring['event'][k].record()
        self._serial += 1
        ring['serial'][k] = self._serial
        keep, self._keep = self._keep, None             # the staged recordings live until the copies behind them have run
        return PendingDetection(self, ring, k, self._serial, plan, filenames, cap, keep)

    def __call__(self, waves, filenames, sample_rates=None, metrics=None):
        return self.submit(waves, filenames, sample_rates, metrics).result()


class PendingDetection(object):
    """the results of one RecordingDetector call on their way to the host"""

    def __init__(self, det, ring, slot, serial, plan, filenames, cap, keep):
        self._det, self._ring, self._slot, self._serial, self._keep = det, ring, slot, serial, keep
        self.plan, self.filenames, self.cap = plan, filenames, cap

    def result(self):
        """wait for the copies, then ({at_m: RecordingPredictions}, WindowTags): copies, the ring slot is free afterwards"""
        r, k, dec = self._ring, self._slot, self._det.decoder
        if r['serial'][k] != self._serial:
            raise RuntimeError('RecordingDetector: this call\'s host buffers were reused by a later submit(); ask for result() within two '
                               'submits')
        r['event'][k].synchronize()
        self._keep = None
        win_off, _, t, _ = self.plan
        preds = {m: RecordingPredictions(dec.labels, dec.threshold_values, self.filenames, c.numpy(), o.numpy(), s.numpy(), self.cap)
                 for m, (c, o, s) in r['res'][k].items()}
        tags = None if r['tags'][k] is None else r['tags'][k].numpy().copy()
        recording = np.repeat(np.arange(len(self.filenames)), np.diff(win_off))
        return preds, WindowTags(tags, recording, t, self.filenames, dec.labels)
