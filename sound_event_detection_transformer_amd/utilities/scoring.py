"""What the five scorers share (EventMetrics, SweepEventMetrics, PsdsMetrics at clip level; RecordingMetrics, RecordingPsds on
recordings).  A scorer is a holder of device counters plus ONE reference; several scorers may hold the same one, which is then built,
uploaded and checked once.  The format of a reference changes here and nowhere else: ``ClipReference`` (the per-clip CSR table),
``RecordingReference`` (``reference_table`` on the device), the scorers' bases ``Scorer`` / ``ClipScorer`` / ``RecordingScorer``,
``Uploads`` (small per-call arrays to the device) and ``read_back`` (counters and statuses to the host in ONE copy)."""
import itertools
import math
import weakref

import numpy as np
import torch

from .transforms import PinnedRing

MAX_REF_EVENTS = 64        # reference events of one clip the clip-level kernels hold (csrc/event_records.h: SEDT_MAX_REF_EVENTS)
STATUS_REASONS = {1: 'its stitched lists are not complete (a stitch status was raised, or a class holds more events than cap)',
                  2: 'more than 64 reference events or 64 estimates of one class lie in one block of onsets chained within t_collar',
                  4: 'an event list is not ascending by onset or holds a non-finite time'}
GENERATION = itertools.count(1)    # one sequence for every table and scorer: a generation taken from it was never seen before


# ------------------------------------------------------------------------------------------------------------------ clip level
class ClipReference(object):
    """the reference events of one validation set, per clip (``labels``: the class names in the model's order).  ``table``: the device
    arrays present / off / cls / on / end / dur the clip-level launches read, ``host`` the same as numpy; ``generation`` changes when
    ``set`` changes what a captured launch baked in: a table pointer, n_clips or max_ref; n_gt / gt_dur / total_dur: PSDS' n_c, T_c, T."""

    def __init__(self, labels, device=None):
        self.labels = list(labels)
        self.index = {l: i for i, l in enumerate(self.labels)}
        self.C = len(self.labels)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.table, self.host, self.n_clips, self.n_events, self.max_ref, self.generation = None, None, 0, 0, 0, 0
        self.n_gt, self.gt_dur, self.total_dur = None, None, 0.0          # PSDS' n_c [C], T_c [C] and T
        self.holders = weakref.WeakSet()          # the scorers that hold this reference (Scorer._bind)

    def set(self, events, durations=None, default_duration=10.0):
        """ClipScorer's list and durations (None: ``default_duration`` each), checked - by the holders too (``_accepts``); a refusal
        leaves everything as it was - and uploaded: in place when every array fits (a captured step stays valid)."""
        events = list(events)
        if durations is None:
            durations = [default_duration] * len(events)
        durations = [float(d) for d in durations]
        if len(durations) != len(events):
            raise ValueError(f'set_reference: {len(durations)} durations for {len(events)} clips')
        off, cls, on, end, present = [0], [], [], [], []
        n_gt, gt_dur, total = np.zeros(self.C, np.int64), np.zeros(self.C, np.float64), 0.0
        for k, ev in enumerate(events):
            present.append(ev is not None)
            if not (math.isfinite(durations[k]) and durations[k] >= 0):
                raise ValueError(f'set_reference: clip {k}: duration {durations[k]!r} is not a finite non-negative number of seconds')
            if ev is not None:
                total += durations[k]
            for label, onset, offset in (ev or ()):
                c = self.index[label] if label in self.index else int(label)
                if not 0 <= c < self.C:
                    raise ValueError(f'set_reference: clip {k}: class {label!r} is not one of the {self.C} labels')
                if not (math.isfinite(onset) and math.isfinite(offset)):
                    raise ValueError(f'set_reference: clip {k}: non-finite event time')
                cls.append(c), on.append(float(onset)), end.append(float(offset))
                if end[-1] - on[-1] > 0:                               # a zero-length event takes part in nothing
                    n_gt[c] += 1
                    gt_dur[c] += end[-1] - on[-1]
            if len(cls) - off[-1] > MAX_REF_EVENTS:
                raise ValueError(f'set_reference: clip {k} has {len(cls) - off[-1]} reference events (at most {MAX_REF_EVENTS})')
            off.append(len(cls))
        host = {'present': np.asarray(present or [0], np.int32), 'off': np.asarray(off, np.int32), 'cls': np.asarray(cls or [0], np.int32),
                'on': np.asarray(on or [0.0], np.float64), 'end': np.asarray(end or [0.0], np.float64),
                'dur': np.asarray(durations or [0.0], np.float64)}
        for h in list(self.holders):
            h._accepts(host, len(cls))
        t, shape = self.table, (len(events), int(np.diff(off).max()) if events else 0)
        if t is not None and all(t[k].numel() >= host[k].size for k in host):
            for k in host:
                t[k][:host[k].size].copy_(torch.from_numpy(host[k]))
        else:
            self.table = {k: torch.from_numpy(v).to(self.device, copy=True) for k, v in host.items()}
            self.generation = next(GENERATION)
        if shape != (self.n_clips, self.max_ref):
            self.generation = next(GENERATION)
        self.host, self.n_events, (self.n_clips, self.max_ref) = host, len(cls), shape
        self.n_gt, self.gt_dur, self.total_dur = n_gt, gt_dur, total
        for h in list(self.holders):
            h._adopted()
        return self

    def host_clip_index(self, idx, who='ClipReference'):
        """the batch's clip indices as a host int32 tensor, checked against the table (-1 = a clip outside it, not evaluated)"""
        h = torch.as_tensor(np.asarray(idx, dtype=np.int64)).reshape(-1)
        bad = (h < -1) | (h >= self.n_clips)
        if bool(bad.any()):
            raise ValueError(f'{who}: clip index {int(h[bad][0])} outside -1 .. {self.n_clips - 1}')
        return h.to(torch.int32)

    def clip_index(self, idx, who='ClipReference'):
        """the same on the device (a device tensor is taken as it is: the kernels skip indices outside the table)"""
        if torch.is_tensor(idx) and idx.is_cuda:
            return idx.to(torch.int32).contiguous()
        return self.host_clip_index(idx, who).to(self.device)


class Scorer(object):
    """base of the five scorers: device counters (``counters()``) plus ``reference`` - the scorer's own, filled by
    ``set_reference(list or dict)``, or one handed to ``set_reference`` that other scorers hold too (a list or dict handed to one of
    them later sets it for all).  A reference asks its holders before it changes (``_accepts``) and tells them after (``_adopted``)."""

    table = property(lambda self: self.reference.table)

    def _bind(self, reference):
        """make ``reference`` (a new one, or one handed to set_reference) this scorer's, if the scorer accepts what it holds"""
        if reference.labels != list(self.labels):
            raise ValueError(f'set_reference: the reference holds labels {reference.labels}, {type(self).__name__} {list(self.labels)}')
        if reference.host is not None:
            self._accepts(reference.host, reference.n_events)
        if getattr(self, 'reference', None) is not None:
            self.reference.holders.discard(self)
        reference.holders.add(self)
        self.reference, self._generation = reference, next(GENERATION)
        self._adopted()

    def _accepts(self, host, n_events):
        pass

    def _adopted(self):
        pass

    def reset(self):
        """zero the counters (start of a validation set or of another grid), in place: a captured graph keeps adding to them"""
        for t in self.counters():
            t.zero_()
        return self


class ClipScorer(Scorer):
    """base of the clip-level scorers.  ``generation`` changes when what a launch captured does: table pointers or shape, the reference"""

    n_clips = property(lambda self: self.reference.n_clips)
    max_ref = property(lambda self: self.reference.max_ref)
    generation = property(lambda self: max(self.reference.generation, self._generation) if self.table is not None else 0)

    def _set_reference(self, events, durations=None):
        """events: per clip (the index ``update`` receives) a list of (label, onset, offset) - label a class name or index, times in
        seconds - or None for a clip without a row in the reference; durations: per clip its seconds (None: max_len each).  Or a
        ClipReference already set, whose durations hold.  Uploads the table once; the counters are not touched."""
        if not isinstance(events, ClipReference):
            self.reference.set(events, durations, default_duration=self.max_len)
        elif durations is not None:
            raise ValueError('set_reference: a ClipReference carries its own durations')
        elif events.table is None:
            raise RuntimeError('set_reference: the reference is empty: call its set() first')
        else:
            self._bind(events)
        return self

    def set_reference(self, events):
        return self._set_reference(events)

    def host_clip_index(self, idx):
        return self.reference.host_clip_index(idx, type(self).__name__)

    def clip_index(self, idx):
        return self.reference.clip_index(idx, type(self).__name__)

    def _records(self, decoded, clip_idx):
        """of what ``EventDecoder.decode`` returned, per fusion strategy: (row i, its device records, the device clip indices)"""
        who = type(self).__name__
        if self.table is None:
            raise RuntimeError(f'{who}.update: set_reference() first')
        idx = self.clip_index(clip_idx)
        for i, m in enumerate(self.fusion):
            records = decoded[0]['dev'][m]
            if records.shape[0] != self.K:
                raise ValueError(f'{who}.update: records of {records.shape[0]} thresholds, the counters hold {self.K}')
            yield i, records, idx


# ------------------------------------------------------------------------------------------------------------------ recordings
def reference_table(reference, labels, segments=False):
    """{filename: [(label, onset, offset), ...]} -> the CSR table over (reference recording, class) the kernels read, as host arrays:
    {'names' (the filenames in the dict's order), 'index' {filename: i}, 'off' int32 [N * C + 1], 'on' / 'end' float64 [E] (per
    (recording, class) sorted by (onset, offset, input order)), 'max_end' float64 [N] (0 for an empty list)}.  label: a class name or
    index.  Unknown labels and non-finite times are refused, with ``segments`` negative times too."""
    labels = list(labels)
    index, C = {l: i for i, l in enumerate(labels)}, len(labels)
    names, off, on, end, max_end = [], [0], [], [], []
    for name, events in reference.items():
        per = [[] for _ in range(C)]
        for n, (label, onset, offset) in enumerate(events):
            if label in index:
                c = index[label]
            elif isinstance(label, (int, np.integer)) and 0 <= int(label) < C:
                c = int(label)
            else:
                raise ValueError(f'set_reference: recording {name!r}: class {label!r} is not one of the {C} labels')
            onset, offset = float(onset), float(offset)
            if not (math.isfinite(onset) and math.isfinite(offset)):
                raise ValueError(f'set_reference: recording {name!r}: non-finite event time ({onset}, {offset})')
            if segments and (onset < 0 or offset < 0):
                raise ValueError(f'set_reference: recording {name!r}: negative event time ({onset}, {offset}) in a segment-based '
                                 'evaluation')
            per[c].append((onset, offset, n))
        for c in range(C):
            per[c].sort()
            on += [e[0] for e in per[c]]
            end += [e[1] for e in per[c]]
            off.append(len(on))
        names.append(name)
        max_end.append(max([e[1] for p in per for e in p], default=0.0))
    if len(on) > 2 ** 31 - 1:
        raise ValueError(f'set_reference: {len(on)} reference events exceed int32 indexing')
    return {'names': names, 'index': {n: i for i, n in enumerate(names)}, 'off': np.asarray(off, np.int32),
            'on': np.asarray(on, np.float64), 'end': np.asarray(end, np.float64), 'max_end': np.asarray(max_end, np.float64)}


def prefix_max(end, off):
    """per (recording, class) list of the CSR table (``off`` [N * C + 1], ``end`` [E]) the running maximum of ``end``: float64 [E].
    No reference before the first j of a list with prefix_max[j] > t ends after t."""
    out = np.array(end, np.float64)
    for a, b in zip(off[:-1], off[1:]):
        if b > a:
            out[a:b] = np.maximum.accumulate(out[a:b])
    return out


def reference_constants(host, n_classes):
    """per reference recording of the table: (n [N, C] int64 the number, t [N, C] float64 the summed duration) of every class's
    reference events, zero-length ones left out"""
    N = len(host['names'])
    n, t = np.zeros((N, n_classes), np.int64), np.zeros((N, n_classes), np.float64)
    dur = host['end'] - host['on']
    for i in range(N):
        for c in range(n_classes):
            d = dur[host['off'][i * n_classes + c]:host['off'][i * n_classes + c + 1]]
            d = d[d > 0]
            n[i, c], t[i, c] = d.size, d.sum()
    return n, t


class RecordingReference(object):
    """the annotations of a set of recordings: ``host`` is ``reference_table``'s result, ``table`` the device dict the recording-level
    launches read (off / on / end, the host ints n_rec and n_events; 'pmax' once ``with_pmax`` was asked for)."""

    def __init__(self, labels, device=None):
        self.labels = list(labels)
        self.C = len(self.labels)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.host, self.table, self.n_events, self._constants = None, None, 0, None
        self.holders = weakref.WeakSet()          # the scorers that hold this reference (Scorer._bind)

    def set(self, reference, segments=False):
        """RecordingScorer's dict as the CSR table, uploaded once if every holder accepts it; ``segments``: no negative times"""
        h = reference_table(reference, self.labels, segments=segments)
        for holder in list(self.holders):
            holder._accepts(h, h['on'].size)
        self.host, self.n_events, self._constants = h, int(h['on'].size), None
        self.table = {'off': self._up(h['off']), 'on': self._up(h['on']), 'end': self._up(h['end']), 'n_rec': len(h['names']),
                      'n_events': self.n_events}
        return self

    def _up(self, a):
        return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(self.device)

    def with_pmax(self):
        """``table`` with 'pmax', the running maximum of the ends per (recording, class) list (``prefix_max``)"""
        if 'pmax' not in self.table:
            self.table['pmax'] = self._up(prefix_max(self.host['end'], self.host['off']))
        return self.table

    def constants(self):
        """``reference_constants`` of the table: per recording (n [N, C], t [N, C]), PSDS' n_c and T_c"""
        if self._constants is None:
            self._constants = reference_constants(self.host, self.C)
        return self._constants

    def recording_index(self, filenames):
        """the recordings' indices in the reference table as host int32 [R] (-1: not in the reference, not evaluated)"""
        return np.asarray([self.host['index'].get(f, -1) for f in filenames], np.int32)


class RecordingScorer(Scorer):
    """base of the recording-level scorers; ``_status``: the launches' status tensors since reset(), as ``read_back`` takes them"""

    host = property(lambda self: self.reference.host)

    def _accepts(self, host, n_events):
        """a scorer with ``time_resolution`` takes no negative time, whoever sets the reference it holds"""
        if getattr(self, 'time_resolution', None) is not None and ((host['on'] < 0).any() or (host['end'] < 0).any()):
            raise ValueError('set_reference: a negative event time in a segment-based evaluation')

    def set_reference(self, reference):
        """reference: {filename: [(label, onset, offset), ...]} - label a class name or index, seconds from the recording's start; a
        filename that is absent is not evaluated, one with an empty list is.  Or a RecordingReference already set.  Builds and
        uploads the CSR table once; the counters are not touched.  A scorer with ``time_resolution`` refuses negative times."""
        if not isinstance(reference, RecordingReference):
            self.reference.set(reference, segments=getattr(self, 'time_resolution', None) is not None)
        elif reference.table is None:
            raise RuntimeError('set_reference: the reference is empty: call its set() first')
        else:
            self._bind(reference)
        return self

    def recording_index(self, filenames):
        return self.reference.recording_index(filenames)

    def _check_counts(self, stitched, n):
        for m in self.fusion:
            shape = tuple(stitched[m][0].shape)
            if shape != (self.K, n, self.C):
                raise ValueError(f'{type(self).__name__}.update: counts {shape} for {self.K} thresholds x {n} recordings x {self.C} classes')

    def _checked(self):
        """every counter as numpy int64, in the order of counters(); raises on a status"""
        return read_back(self.counters(), self._status)

    def reset(self):
        """zero the counters and forget the statuses (start of an evaluation)"""
        self._status = []
        return Scorer.reset(self)


# ------------------------------------------------------------------------------------------------------------------ to and from the device
class Uploads(object):
    """small per-call host arrays (int32 / float64) to the device, every name through its own transforms.PinnedRing"""

    DTYPES = {np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64}

    def __init__(self, device):
        self.device, self.rings = device, {}

    def __call__(self, name, host):
        ring = self.rings.get(name)
        if ring is None:
            ring = self.rings[name] = PinnedRing(self.device)
        host = np.ascontiguousarray(host)
        return ring.upload(host.view(np.uint8).reshape(-1))[:host.nbytes].view(self.DTYPES[host.dtype])


def status_error(status, filenames, thresholds, what):
    """None, or the RuntimeError for the first non-zero entry of a launch's status [K, R]"""
    bad = np.argwhere(np.asarray(status) != 0)
    if not len(bad):
        return None
    k, r = (int(v) for v in bad[0])
    s = int(status[k][r])
    return RuntimeError(f'{what}: recording {filenames[r]!r} at threshold {thresholds[k]}: status {s} ({STATUS_REASONS.get(s, "unknown")})')


def read_back(counters, statuses=()):
    """the int64 device tensors ``counters`` as numpy arrays, in their order, from ONE device->host copy that also carries ``statuses``:
    per launch (status int32 [K, R] on the device, filenames, thresholds, what).  Raises ``status_error`` of the first that reported one."""
    ts = list(counters) + [s[0].to(torch.int64) for s in statuses]
    h = torch.cat([t.reshape(-1) for t in ts]).cpu().numpy()
    got, o = [], 0
    for t in ts:
        got.append(h[o:o + t.numel()].reshape(t.shape))
        o += t.numel()
    for st, (_, filenames, thresholds, what) in zip(got[len(counters):], statuses):
        err = status_error(st, filenames, thresholds, what)
        if err is not None:
            raise err
    return got[:len(counters)]
