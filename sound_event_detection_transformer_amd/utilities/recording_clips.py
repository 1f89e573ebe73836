"""Training on annotated recordings of any length.  The reference trains on 10 s dataset clips that the host cut, with strong labels that
the host encoded (data_utils/DataLoad.py, utilities/BoxEncoder.py encode_strong_df).  Here the recordings and their annotations are
staged on the device ONCE; every training batch is then a set of random windows cut from them by ONE launch (sedt_cut_clips,
csrc/clips.hip), and the same launch builds the windows' target tables in the layout the matching kernel reads
(sedt.TargetTables).  DESIGN.md section 4 ("Training on recordings") holds the definition; tests/recording_clips_ref.py restates it.

    clips = RecordingClips(mel, labels, window_seconds=10.0).add(waves, names, {'street.wav': [('Speech', 1.5, 4.25), ...]})
    x, targets = clips.batch(transform, clips.draw(64))          # (B, 1, frames, n_mels), DeviceTargets - nothing synchronises
    step(x, targets)                                             # engine.GraphedTrainStep: one device copy fills its tables
    engine.train_on_recordings(step, clips, transform, steps)    # the plain loop

Recordings come in three kinds (``add(..., kind=)``): 'strong' (annotated events), 'weak' (tags only) and 'unlabelled'.  A batch of
several kinds is laid out as the steppers expect it - strong clips, then weak ones, then unlabelled ones - and carries its static split:

    picks = clips.draw_split(16, 16)                             # C3: 16 strong + 16 weak clips
    x, targets = clips.batch(transform, picks, split=(16, 32))   # targets.ns == 16, targets.n_lab == 32
    (x_t, x_s), targets = clips.batch(view_transform, clips.draw_split(2, 1, 2), split=(2, 3))
    engine.semi_train_on_recordings(step, clips, view_transform, steps, split=(2, 1, 2))      # the mean-teacher loop

A mixing stepper takes such targets as they are: sedt.TargetTables.load_mixed plans mix-up on the device (sedt_mixup_plan, csrc/mixplan.hip).

Definition of a clip's targets.  Float64, plain subtract / multiply / divide / compare.  W = window / sr, t0 = start / sr, t1 = t0 + W.
For every annotated event (class c, on, end) of the recording, in table order (sorted by (onset, offset, input order)):
a = max(on, t0) - t0, z = min(end, t1) - t0; the event is kept iff z - a > 0 and z - a >= min_event_seconds, and becomes label c and
box (float32(((a + z) * 0.5) / W), float32((z - a) / W)).  Events of one class that overlap are kept as annotated.  More than
``max_targets`` survivors raise the clip's status (the first ``max_targets`` are written): the count is never cut silently.

``clip_event_table``, ``draw_picks`` and ``blob_layout`` are the host half and need no GPU."""
import math

import numpy as np
import torch

from .. import lib as L
from .recording import stage_recordings, stage_resampled
from .recording_psds import prefix_max
from .transforms import PinnedRing

KINDS = ('strong', 'weak', 'unlabelled')
STATUS_REASONS = {1: 'more events survive in the clip than max_targets holds: build RecordingClips with a larger max_targets',
                  2: 'the pick is not inside the table of staged recordings'}


def clip_event_table(reference, labels):
    """{filename: [(label, onset, offset), ...]} -> the per-recording event table sedt_cut_clips reads, as host arrays: {'names' (the
    filenames in the dict's order), 'index' {filename: r}, 'off' int32 [R + 1], 'on' / 'end' float64 [E], 'cls' int32 [E], 'pmax'
    float64 [E]}.  Per recording the events of ALL classes are sorted by (onset, offset, input order); pmax is the running maximum of
    'end' inside the recording (no event before the first j with pmax[j] > t ends after t).  label: a class name or index.  Unknown
    labels, non-finite times and end < onset are refused; a recording annotated with [] is valid (silence)."""
    labels = list(labels)
    index, C = {l: i for i, l in enumerate(labels)}, len(labels)
    names, off, on, end, cls = [], [0], [], [], []
    for name, events in reference.items():
        rows = []
        for n, (label, onset, offset) in enumerate(events):
            if label in index:
                c = index[label]
            elif isinstance(label, (int, np.integer)) and not isinstance(label, bool) and 0 <= int(label) < C:
                c = int(label)
            else:
                raise ValueError(f'clip_event_table: recording {name!r}: class {label!r} is not one of the {C} labels')
            onset, offset = float(onset), float(offset)
            if not (math.isfinite(onset) and math.isfinite(offset)):
                raise ValueError(f'clip_event_table: recording {name!r}: non-finite event time ({onset}, {offset})')
            if offset < onset:
                raise ValueError(f'clip_event_table: recording {name!r}: an event ends before it starts ({onset}, {offset})')
            rows.append((onset, offset, n, c))
        rows.sort(key=lambda e: e[:3])
        on += [e[0] for e in rows]
        end += [e[1] for e in rows]
        cls += [e[3] for e in rows]
        off.append(len(on))
        names.append(name)
    if len(on) > 2 ** 31 - 1:
        raise ValueError(f'clip_event_table: {len(on)} events exceed int32 indexing')
    off, end = np.asarray(off, np.int32), np.asarray(end, np.float64)
    return {'names': names, 'index': {n: i for i, n in enumerate(names)}, 'off': off, 'on': np.asarray(on, np.float64), 'end': end,
            'cls': np.asarray(cls, np.int32), 'pmax': prefix_max(end, off)}


def weak_events(tags, labels, seconds, name='?'):
    """a weakly labelled recording's tags [label, ...] (class names or indices) -> the events [(class index, 0.0, seconds), ...] staged
    for it: one per tag, de-duplicated in input order; unknown labels are refused"""
    labels = list(labels)
    index, C = {l: i for i, l in enumerate(labels)}, len(labels)
    seen = []
    for label in tags:
        if label in index:
            c = index[label]
        elif isinstance(label, (int, np.integer)) and not isinstance(label, bool) and 0 <= int(label) < C:
            c = int(label)
        else:
            raise ValueError(f'weak_events: recording {name!r}: class {label!r} is not one of the {C} labels')
        if c not in seen:
            seen.append(c)
    return [(c, 0.0, float(seconds)) for c in seen]


def draw_split_picks(ns, kinds, window, counts):
    """picks (rec int32, start int64) for counts = (n_strong, n_weak, n_unlabelled) clips, kind by kind, strong first: every kind is one
    draw_picks over that kind's recordings (``kinds``: the kind of each staged recording), so np.random is consumed in that order"""
    ns, rec, start = np.asarray(ns, np.int64), [], []
    for kind, n in zip(KINDS, counts):
        if int(n) < 0:
            raise ValueError(f'draw_split: {n} {kind} clips')
        if int(n) == 0:
            continue
        own = np.asarray([r for r, k in enumerate(kinds) if k == kind], np.int32)
        if not len(own):
            raise ValueError(f'draw_split: {n} {kind} clips asked for, no {kind} recording is staged')
        r, s_ = draw_picks(ns[own], window, n)
        rec.append(own[r])
        start.append(s_)
    if not rec:
        raise ValueError('draw_split: no clips asked for')
    return np.concatenate(rec).astype(np.int32), np.concatenate(start).astype(np.int64)


def blob_layout(B, max_targets):
    """(offset words, byte offset of lab_cat, of box_cat, total bytes) of the target blob of B clips: the layout of
    sedt.TargetTables(batch=B, ns=B, n_lab=B, max_targets=max_targets, with_ratio=False)"""
    n_off = 2 * B + 4
    o_lab = (4 * n_off + 7) // 8 * 8
    o_box = o_lab + 8 * B * max_targets
    return n_off, o_lab, o_box, o_box + 8 * B * max_targets


class DeviceTargets(object):
    """the targets of one cut batch where sedt_cut_clips wrote them: ``blob`` (uint8, the TargetTables layout of B strong clips),
    ``status`` int32 [B], both on the device and both OVERWRITTEN by the next cut into the same buffers.  ``names``: the recording every
    clip was cut from.  ``ns`` / ``n_lab`` (keywords, default B and B): the static split the blob is READ under - clips from ``ns`` on
    are weak (their boxes are ignored), clips from ``n_lab`` on unlabelled.  ``TargetTables.load`` takes it with a few device copies,
    ``TargetTables.load_mixed`` plans mix-up from it on the device; ``to_list`` is the list-of-dicts form."""

    def __init__(self, blob, status, B, max_targets, names, orig_size, *, ns=None, n_lab=None):
        self.blob, self.status, self.B, self.max_targets = blob, status, int(B), int(max_targets)
        self.names, self.orig_size = list(names), float(orig_size)
        self.ns = self.B if ns is None else int(ns)
        self.n_lab = self.B if n_lab is None else int(n_lab)
        if not 0 <= self.ns <= self.n_lab <= self.B:
            raise ValueError(f'DeviceTargets: split {self.ns} | {self.n_lab} outside 0..{self.B}')

    def __len__(self):
        return self.B

    def check(self):
        """synchronises; raises on a clip whose status is not 0, naming its recording"""
        err = status_error(self.status.cpu().numpy(), self.names)
        if err is not None:
            raise err
        return self

    def to_list(self):
        """synchronises; [{'labels' int64 (n,), 'boxes' float32 (n, 2), 'orig_size'}] on the host, one dict per clip - for a stepper's
        example targets, the eager paths and tests; clips from ``ns`` on have empty boxes, clips from ``n_lab`` on empty labels.  Raises
        on a non-zero status."""
        self.check()
        n_off, o_lab, o_box, total = blob_layout(self.B, self.max_targets)
        raw = self.blob[:total].cpu().numpy()
        off = raw[:4 * (self.B + 1)].view(np.int32)
        lab = raw[o_lab:o_box].view(np.int64)
        box = raw[o_box:total].view(np.float32).reshape(-1, 2)
        return [{'labels': torch.from_numpy(lab[off[b]:off[b + 1] if b < self.n_lab else off[b]].copy()),
                 'boxes': torch.from_numpy(box[off[b]:off[b + 1] if b < self.ns else off[b]].copy()),
                 'orig_size': torch.tensor(self.orig_size)} for b in range(self.B)]


def status_error(status, names, what='cut_clips', reasons=None):
    """None, or the RuntimeError for the first non-zero entry of a status vector [B] (or [steps, B] with names [steps][B]);
    ``reasons``: what the status values mean (default: sedt_cut_clips')"""
    status = np.asarray(status)
    bad = np.argwhere(status != 0)
    if not len(bad):
        return None
    at = tuple(int(v) for v in bad[0])
    s = int(status[at])
    name = names[at[0]] if len(at) == 1 else names[at[0]][at[1]]
    where = f'clip {at[0]}' if len(at) == 1 else f'step {at[0]}, clip {at[1]}'
    return RuntimeError(f'{what}: {where} of recording {name!r}: status {s} ({(STATUS_REASONS if reasons is None else reasons).get(s, "unknown")})')


def draw_picks(ns, window, B):
    """B picks (rec int32 [B], start int64 [B]) from recordings of ``ns`` samples, consuming np.random per clip in order:
    r = np.random.choice(R, p=w) with w proportional to max(n_r - window, 0) + 1 (the number of start positions), then
    start = np.random.randint(0, max(n_r - window, 0) + 1).  A recording shorter than the window always starts at 0."""
    room = np.maximum(np.asarray(ns, np.int64) - int(window), 0) + 1
    w = room / room.sum()
    rec, start = np.zeros(int(B), np.int32), np.zeros(int(B), np.int64)
    for b in range(int(B)):
        rec[b] = np.random.choice(len(room), p=w)
        start[b] = np.random.randint(0, room[rec[b]])
    return rec, start


class RecordingClips(object):
    """mel: the DeviceMelSpectrogram of the model (its sample rate is the recordings' after staging); labels: the class names;
    window_seconds: the clip length; max_targets: the events a clip's tables hold (1 .. 63, the stepper's TargetTables must be built
    with the same value); min_event_seconds: events clipped shorter than this are dropped.  See the module docstring."""

    def __init__(self, mel, labels, window_seconds, max_targets=32, min_event_seconds=0.0, device='cuda', resample_quality='kaiser_best'):
        self.mel, self.labels = mel, list(labels)
        self.window_seconds = float(window_seconds)
        self.window = int(round(self.window_seconds * mel.sr))
        self.max_targets, self.min_event_seconds = int(max_targets), float(min_event_seconds)
        if not 1 <= self.max_targets <= 63:
            raise ValueError('max_targets must be in 1..63 (the target tables\' own limit)')
        if self.window < mel.min_samples:
            raise ValueError(f'RecordingClips: a window of {self.window} samples is shorter than the {mel.min_samples} the front end needs')
        if math.isnan(self.min_event_seconds):
            raise ValueError('RecordingClips: min_event_seconds is NaN')
        self.dev = torch.device(device)
        self.resample_quality, self._resamplers = resample_quality, {}
        self.names, self.ns, self.reference, self.kinds = [], [], {}, []
        self.flat, self.host, self.table = None, None, None
        self.rec_off = None
        self._ring, self._buf, self._amp, self._keep = None, {}, {}, []

    # ------------------------------------------------------------------ staging
    def resampler(self, rate):
        """the DeviceResampler from ``rate`` to mel.sr, made at first use and kept"""
        rs = self._resamplers.get(int(rate))
        if rs is None:
            from .resample import DeviceResampler
            rs = self._resamplers[int(rate)] = DeviceResampler(int(rate), self.mel.sr, self.resample_quality, device=self.dev)
        return rs

    def add(self, waves, filenames, reference, sample_rates=None, kind='strong'):
        """stage recordings and their annotations on the device, where they stay: ``waves`` 1-D float32 / int16 at mel.sr (host or
        device) or, with ``sample_rates`` (one int or one per recording), at any rate and interleaved (frames, channels) - down-mixed
        and resampled on the device as RecordingDetector does.  May be called again to add more.  Returns self.
        kind='strong': ``reference`` {filename: [(label, onset, offset), ...]} with an entry for every recording ([]: silence).
        kind='weak': ``reference`` {filename: [label, ...]}, the recording's tags (de-duplicated in input order).  Every tag is staged as
        an event from 0 to max(duration, window_seconds), so EVERY window of the recording carries all its tags: exact for recordings
        no longer than the window (DCASE's weak clips); for longer ones it is the multiple-instance assumption - a tag may be absent
        from a given window - and the caller's choice.  The boxes of such clips are never read.
        kind='unlabelled': ``reference`` may be None; no events are staged."""
        waves, filenames = list(waves), list(filenames)
        if kind not in KINDS:
            raise ValueError(f'RecordingClips.add: kind {kind!r} is not one of {KINDS}')
        if len(waves) != len(filenames) or not waves:
            raise ValueError('RecordingClips.add: one name per recording, at least one recording')
        reference = {} if reference is None else reference
        for f in filenames:
            if kind != 'unlabelled' and f not in reference:
                raise ValueError(f'RecordingClips.add: recording {f!r} has no entry in the reference (annotate silence with [])')
            if f in self.reference or filenames.count(f) > 1:
                raise ValueError(f'RecordingClips.add: recording {f!r} is staged twice')
        merged = dict(self.reference)
        if kind == 'strong':
            merged.update({f: list(reference[f]) for f in filenames})
        elif kind == 'weak':                                         # (the durations are known once the recordings are staged)
            merged.update({f: weak_events(reference[f], self.labels, self.window_seconds, f) for f in filenames})
        else:
            merged.update({f: [] for f in filenames})
        host = clip_event_table(merged, self.labels)                 # refusals before anything is staged
        if sample_rates is not None:
            flat, _, ns, keep = stage_resampled(waves, sample_rates, self.resampler, self.dev)
        else:
            flat, _, ns, keep = stage_recordings(waves, self.dev)
        for f, n in zip(filenames, ns):
            if n < self.mel.min_samples:
                raise ValueError(f'RecordingClips.add: recording {f!r} of {n} samples is shorter than the {self.mel.min_samples} the front '
                                 'end needs')
        if kind == 'weak':
            for f, n in zip(filenames, ns):
                merged[f] = weak_events(reference[f], self.labels, max(int(n) / self.mel.sr, self.window_seconds), f)
            host = clip_event_table(merged, self.labels)
        self._keep.append(keep)                                      # the raw input lives until the copies behind it have run
        self.flat = flat if self.flat is None else torch.cat([self.flat[:sum(self.ns)], flat])
        self.names, self.ns, self.reference, self.host = self.names + filenames, self.ns + [int(n) for n in ns], merged, host
        self.kinds = self.kinds + [kind] * len(filenames)
        off = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        self.rec_off = off
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.table = {'rec_off': up(off[:-1]), 'rec_len': up(np.asarray(self.ns, np.int64)), 'off': up(host['off']),
                      'on': up(pad(host['on'])), 'end': up(pad(host['end'])), 'cls': up(pad(host['cls'])), 'pmax': up(pad(host['pmax'])),
                      'n_events': int(host['on'].size)}
        return self

    def __len__(self):
        return len(self.names)

    def wave(self, name):
        """the device view of one staged recording (1-D float32 at mel.sr): RecordingDetector takes it as it is"""
        r = self.names.index(name)
        return self.flat[int(self.rec_off[r]):int(self.rec_off[r + 1])]

    # ------------------------------------------------------------------ batches
    def draw(self, B):
        """B picks (rec int32 [B], start int64 [B]) over the staged recordings: draw_picks.  Strong recordings only: with weak or
        unlabelled ones staged a batch has a layout, draw_split"""
        if not self.names:
            raise RuntimeError('RecordingClips.draw: add() recordings first')
        if any(k != 'strong' for k in self.kinds):
            raise RuntimeError('RecordingClips.draw: weak or unlabelled recordings are staged: draw_split(n_strong, n_weak, n_unlabelled)')
        return draw_picks(self.ns, self.window, B)

    def draw_split(self, n_strong, n_weak=0, n_unlabelled=0):
        """picks for a batch of n_strong strong, then n_weak weak, then n_unlabelled unlabelled clips: draw_split_picks"""
        if not self.names:
            raise RuntimeError('RecordingClips.draw_split: add() recordings first')
        return draw_split_picks(self.ns, self.kinds, self.window, (n_strong, n_weak, n_unlabelled))

    def check_split(self, rec, split):
        """(ns, n_lab) of a batch of picks; raises unless the picked recordings are strong | weak | unlabelled in that layout"""
        B = len(rec)
        ns, n_lab = (B, B) if split is None else (int(split[0]), int(split[1]))
        if not 0 <= ns <= n_lab <= B:
            raise ValueError(f'RecordingClips.cut: split {ns} | {n_lab} outside 0..{B}')
        for b, r in enumerate(rec):
            want = KINDS[0] if b < ns else (KINDS[1] if b < n_lab else KINDS[2])
            if self.kinds[int(r)] != want:
                raise ValueError(f'RecordingClips.cut: clip {b} is cut from the {self.kinds[int(r)]} recording {self.names[int(r)]!r}, the '
                                 f'split {ns} | {n_lab} of {B} wants a {want} one there')
        return ns, n_lab

    def buffers(self, B):
        """(wave (B, window) f32, blob uint8, status int32 [B]) of batch size B, owned by this object and reused by every cut"""
        buf = self._buf.get(int(B))
        if buf is None:
            buf = self._buf[int(B)] = (torch.zeros((B, self.window), dtype=torch.float32, device=self.dev),
                                       torch.zeros(blob_layout(B, self.max_targets)[3], dtype=torch.uint8, device=self.dev),
                                       torch.zeros(B, dtype=torch.int32, device=self.dev))
        return buf

    def cut(self, rec, start, status=None, split=None):
        """ONE sedt_cut_clips launch on the current stream into this object's buffers: (wave (B, window) f32 on the device, samples per
        clip min(window, n_r - start) as a host list, DeviceTargets).  The picks travel through a ring of pinned buffers; nothing
        synchronises.  ``status``: an int32 [B] device tensor to raise the statuses in instead of the buffer's own (a row of a log,
        engine.train_on_recordings).  ``split`` = (ns, n_lab): the batch is strong | weak | unlabelled clips in that layout (default:
        every clip strong); picks whose recordings are of another kind are refused."""
        if self.table is None:
            raise RuntimeError('RecordingClips.cut: add() recordings first')
        rec, start = np.ascontiguousarray(rec, np.int32), np.ascontiguousarray(start, np.int64)
        B = int(rec.shape[0])
        if rec.shape != (B,) or start.shape != (B,) or not 1 <= B <= L.CLIPS_MAXB:
            raise ValueError(f'RecordingClips.cut: one (rec, start) pair per clip, 1 .. {L.CLIPS_MAXB} clips')
        ns = np.asarray(self.ns, np.int64)
        if rec.min() < 0 or rec.max() >= len(ns) or start.min() < 0 or bool((start >= ns[rec]).any()):
            raise ValueError('RecordingClips.cut: a pick outside its recording (0 <= rec < recordings, 0 <= start < samples)')
        n_strong, n_lab = self.check_split(rec, split)
        if self._ring is None:
            self._ring = PinnedRing(self.dev)
        raw = self._ring.upload(np.concatenate([start.view(np.uint8), rec.view(np.uint8)]))
        d_start, d_rec = raw[:8 * B].view(torch.int64), raw[8 * B:12 * B].view(torch.int32)
        wave, blob, own = self.buffers(B)
        status = own if status is None else status
        if status.shape != (B,) or status.dtype != torch.int32 or not status.is_contiguous() or status.device != wave.device:
            raise ValueError('RecordingClips.cut: status is a contiguous int32 [B] tensor on the device')
        t = self.table
        L.check(L.load().sedt_cut_clips(L.p(self.flat), int(self.rec_off[-1]), L.p(t['rec_off']), L.p(t['rec_len']), len(self.names),
                                        L.p(d_rec), L.p(d_start), B, self.window, self.mel.sr, L.p(t['off']), L.p(t['on']), L.p(t['end']),
                                        L.p(t['cls']), L.p(t['pmax']), t['n_events'], self.max_targets, self.min_event_seconds,
                                        L.p(wave), L.p(blob), L.p(status), L.stream_ptr()), 'cut_clips')
        lengths = np.minimum(self.window, ns[rec] - start).tolist()
        return wave, lengths, DeviceTargets(blob, status, B, self.max_targets, [self.names[r] for r in rec], self.window_seconds,
                                            ns=n_strong, n_lab=n_lab)

    def batch(self, transform, picks=None, B=None, status=None, split=None):
        """cut -> mel -> transform: (x (B, 1, frames, n_mels), DeviceTargets).  ``picks``: (rec, start), else draw(B).  The transform
        (a DeviceBoxTransform) may augment; a DeviceViewTransform makes both views of the mean-teacher recipe and the result is
        ((x_teacher, x_student), DeviceTargets).  ``split``: as in cut."""
        if picks is None:
            if B is None:
                raise ValueError('RecordingClips.batch: picks=(rec, start) or B=')
            picks = self.draw(B)
        wave, lengths, targets = self.cut(picks[0], picks[1], status=status, split=split)
        amp = self._amp.get(wave.shape[0])
        if amp is None:
            amp = self._amp[wave.shape[0]] = torch.zeros((wave.shape[0], 1 + self.window // self.mel.hop, self.mel.F), dtype=torch.float32,
                                                         device=self.dev)
        amp, nframes = self.mel(wave, lengths=lengths, out=amp)
        return transform(amp, nframes=nframes), targets
