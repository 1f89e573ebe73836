"""The predictions of the reference's engine.get_sedt_predictions (engine.py:218-297) decoded on the device: per fusion strategy the
(event_label, onset, offset, score, filename) rows BoxEncoder.decode_strong + the clip to [0, max_len_seconds] give, at one threshold
or at a whole grid of them (one prediction table per operating point, what compute_psds_from_operating_points takes), and the
audio-tag rows (event_label, filename, onset = offset = 0) of BoxEncoder.decode_weak.

``EventDecoder`` owns the device side: the threshold vector, one packed buffer per fusion strategy that ops.decode_events
(csrc/decode.hip) fills with one launch - inside the captured graph of engine.GraphedPredictStep(decoder=...) - and a ring of pinned
host buffers the records are copied into asynchronously.  ``fetch()`` returns a handle; ``rows()`` on it waits for the copy and
unpacks with numpy, which a validation loop does for batch i - 1 while the device runs batch i (engine.get_sedt_predictions).
``PredictionSet`` collects the rows of one fusion strategy over a validation pass.

Times and scores stay the float32 values the device computed (the reference's rows hold the same float32 scalars); a TSV writes
them in float32's shortest round-trip form."""
import numpy as np
import torch

from .. import ops

COLUMNS = ('event_label', 'onset', 'offset', 'score', 'filename')      # the reference's prediction frame (engine.py:285-288)
TAG_COLUMNS = ('event_label', 'filename', 'onset', 'offset')           # its audio-tag frame (engine.py:269-272)


def operating_point(t):
    """the threshold of one operating point as it is reported: a float, or with class-wise thresholds (one row of an EventDecoder's
    [K, C] grid) a tuple of C floats"""
    t = np.asarray(t)
    return float(t) if t.ndim == 0 else tuple(float(v) for v in t.reshape(-1))


def unpack(packed, Q):
    """a packed decode buffer [K, B, 1 + 5 Q] (numpy int32, include/sedt_hip.h: sedt_decode_events) -> per threshold a dict of
    copied arrays {clip int64 [n], cls int32 [n], onset / offset / score float32 [n], query int32 [n]}: clips in order, the events
    of a clip in decode order"""
    packed = np.asarray(packed)
    assert packed.dtype == np.int32 and packed.ndim == 3 and packed.shape[2] == 1 + 5 * Q, (packed.dtype, packed.shape, Q)
    count, cls, times, score, query = ops.decode_events_views(packed, Q)
    if count.size and (count.min() < 0 or count.max() > Q):
        raise ValueError(f'unpack: event count outside 0 .. {Q}: not a decode_events buffer')
    out = []
    for k in range(packed.shape[0]):
        live = np.arange(Q)[None, :] < count[k][:, None]               # [B, Q], row-major = clip order, then slot order
        out.append({'clip': np.nonzero(live)[0], 'cls': cls[k][live], 'onset': times[k][..., 0][live], 'offset': times[k][..., 1][live],
                    'score': score[k][live], 'query': query[k][live]})
    return out


class PredictionTable(object):
    """the prediction rows at one threshold (a float, or a tuple of one per class) as column arrays: event_label (names), onset, offset,
    score (float32), filename"""

    def __init__(self, threshold, event_label, onset, offset, score, filename):
        self.threshold = threshold
        self.event_label, self.onset, self.offset, self.score, self.filename = event_label, onset, offset, score, filename

    def __len__(self):
        return len(self.event_label)

    def to_rows(self):
        """[(event_label, onset, offset, score, filename)] with Python floats"""
        return list(zip(self.event_label.tolist(), self.onset.tolist(), self.offset.tolist(), self.score.tolist(),
                        self.filename.tolist()))

    def to_dataframe(self):
        import pandas as pd
        return pd.DataFrame({c: getattr(self, c) for c in COLUMNS}, columns=list(COLUMNS))

    def write_tsv(self, path):
        with open(path, 'w') as f:
            f.write('\t'.join(COLUMNS) + '\n')
            for lab, on, off, sc, name in zip(self.event_label, self.onset, self.offset, self.score, self.filename):
                f.write(f'{lab}\t{str(on)}\t{str(off)}\t{str(sc)}\t{name}\n')      # str(np.float32): shortest round trip


class PredictionSet(object):
    """one fusion strategy's predictions over a validation pass, per threshold of the decoder's grid (``thresholds``: per operating
    point a float, or for a class-wise decoder the C thresholds of its classes, kept as a tuple).  Order is the reference's: batches in
    order, clips in order, events in decode order."""

    def __init__(self, labels, thresholds):
        self.labels = np.asarray(list(labels), dtype=object)
        self.thresholds = [operating_point(t) for t in thresholds]
        self._parts = [[] for _ in self.thresholds]
        self._tables = None

    def __len__(self):
        return len(self.thresholds)

    def add(self, events, filenames):
        """one batch: ``events`` as ``unpack`` returns them, ``filenames`` the batch's clips' names"""
        assert len(events) == len(self.thresholds), (len(events), len(self.thresholds))
        names = np.asarray(list(filenames), dtype=object)
        for k, e in enumerate(events):
            self._parts[k].append((self.labels[e['cls']], e['onset'], e['offset'], e['score'], names[e['clip']]))
        self._tables = None
        return self

    def at(self, k):
        """the PredictionTable of threshold k"""
        if self._tables is None:
            self._tables = [None] * len(self.thresholds)
        if self._tables[k] is None:
            empty = (np.zeros(0, object), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, object))
            cols = [np.concatenate(c) for c in zip(*self._parts[k])] if self._parts[k] else empty
            self._tables[k] = PredictionTable(self.thresholds[k], *cols)
        return self._tables[k]

    def __iter__(self):
        return (self.at(k) for k in range(len(self.thresholds)))

    def to_rows(self, k=0):
        return self.at(k).to_rows()

    def to_dataframe(self, k=0):
        return self.at(k).to_dataframe()

    def write_tsv(self, path, k=0):
        """the rows at threshold k with the reference's columns, tab-separated"""
        self.at(k).write_tsv(path)


class TagTable(object):
    """the audio-tag rows of a validation pass (engine.py:266-273): event_label, filename, onset = offset = 0"""

    def __init__(self):
        self._parts = []

    def add(self, names, filenames):
        self._parts.append((np.asarray(names, dtype=object), np.asarray(filenames, dtype=object)))
        return self

    @property
    def event_label(self):
        return np.concatenate([p[0] for p in self._parts]) if self._parts else np.zeros(0, object)

    @property
    def filename(self):
        return np.concatenate([p[1] for p in self._parts]) if self._parts else np.zeros(0, object)

    def __len__(self):
        return sum(len(p[0]) for p in self._parts)

    @property
    def empty(self):
        return len(self) == 0

    def to_rows(self):
        return [(l, f, 0, 0) for l, f in zip(self.event_label.tolist(), self.filename.tolist())]

    def to_dataframe(self):
        import pandas as pd
        n = len(self)
        return pd.DataFrame({'event_label': self.event_label, 'filename': self.filename, 'onset': np.zeros(n, np.int64),
                             'offset': np.zeros(n, np.int64)}, columns=list(TAG_COLUMNS))


class Fetched(object):
    """the records of one batch on their way to the host (EventDecoder.fetch)"""

    def __init__(self, decoder, ring, slot, serial, has_tags, thresholds):
        self._dec, self._ring, self._slot, self._serial, self._has_tags = decoder, ring, slot, serial, has_tags
        self.thresholds = thresholds

    def rows(self):
        """wait for the copies, then (tags [B, C] numpy 0/1 or None, {at_m: unpack(...)}): copies, the ring slot is free afterwards"""
        r = self._ring
        if r['serial'][self._slot] != self._serial:
            raise RuntimeError('EventDecoder: this batch\'s host buffer was reused by a later fetch(); call rows() within '
                               f'{len(r["event"])} fetches')
        r['event'][self._slot].synchronize()
        tags = r['tags'][self._slot].numpy().copy() if self._has_tags else None
        return tags, {m: unpack(p[self._slot].numpy(), r['Q']) for m, p in r['packed'].items()}


class EventDecoder(object):
    """decode_strong(threshold, del_overlap) + the clip to [0, max_len_seconds] at every threshold of a grid, on the device.
    ``labels``: the class names in the model's class order (decoder.labels); ``max_len_seconds``: a value float32 holds exactly
    (the drivers' 10), inf for no clip; ``thresholds``: the grid (K values, compared as float32 like the reference's torch scalars);
    ``fusion_strategy``: the PostProcess fusion modes the predict step runs, in its order.

    ``class_wise=True``: every operating point holds one threshold per class - the device grid and ``threshold_values`` are [K, C], a
    query is compared with the threshold of its label, ``thresholds`` / ``set_thresholds`` take [K] (each value for every class) or
    [K, C], and an operating point's threshold is reported as a tuple of C floats (``operating_points()``).  Decode is class by class:
    class c's events at point k are those of a uniform threshold threshold_values[k, c]."""

    def __init__(self, labels, max_len_seconds, thresholds=(0.5,), min_duration=0.2, del_overlap=True, fusion_strategy=(1,), device=None,
                 slots=2, class_wise=False):
        self.labels = list(labels)
        self.C = len(self.labels)
        assert 1 <= self.C <= 63, 'EventDecoder: 1..63 classes'
        self.max_len = float(max_len_seconds)
        if not (self.max_len >= 0 and float(np.float32(self.max_len)) == self.max_len):
            raise ValueError(f'EventDecoder: max_len_seconds {max_len_seconds!r} is not a non-negative value float32 represents exactly')
        self.min_duration, self.del_overlap = float(min_duration), bool(del_overlap)
        self.fusion = tuple(fusion_strategy)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.class_wise = bool(class_wise)
        host = self._grid(thresholds)
        if not 1 <= host.shape[0] <= ops.DECODE_MAX_THRESHOLDS:
            raise ValueError(f'EventDecoder: {host.shape[0]} thresholds (1 .. {ops.DECODE_MAX_THRESHOLDS})')
        self.threshold_values = host
        self.thresholds = torch.from_numpy(host.copy()).to(self.device)
        assert slots >= 2
        self._slots = slots
        self._rings = {}              # (B, Q) -> the static device buffers and the pinned ring of that batch shape
        self._last = None
        self._serial = 0

    def _grid(self, values):
        host = np.asarray(list(values), dtype=np.float64)
        if not self.class_wise:
            host = host.reshape(-1)
        elif host.ndim <= 1:
            host = np.repeat(host.reshape(-1, 1), self.C, axis=1)          # [K]: each value for every class
        elif host.ndim != 2 or host.shape[1] != self.C:
            raise ValueError(f'EventDecoder: class-wise thresholds {host.shape} are neither [K] nor [K, {self.C}]')
        host = np.ascontiguousarray(host.astype(np.float32))
        if np.isnan(host).any():
            raise ValueError('EventDecoder: a threshold is NaN')
        return host

    @property
    def K(self):
        return self.threshold_values.shape[0]

    def operating_points(self):
        """the grid as it is reported: per operating point a float, or with class_wise a tuple of C floats"""
        return [operating_point(t) for t in self.threshold_values]

    def set_thresholds(self, values):
        """another grid of the same K ([K], or with class_wise [K] or [K, C]), in place: a captured graph reads it at its next replay"""
        host = self._grid(values)
        if host.shape[0] != self.K:
            raise ValueError(f'set_thresholds: {host.shape[0]} thresholds, the decoder was built with {self.K}')
        self.threshold_values = host
        self.thresholds.copy_(torch.from_numpy(host.copy()))
        return self

    def _ring(self, B, Q):
        r = self._rings.get((B, Q))
        if r is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'EventDecoder: no buffers for batches of {B} x {Q} yet; decode one batch before capturing')
            shape = (self.K, B, 1 + 5 * Q)
            r = {'Q': Q, 'k': 0,
                 'dev': {m: torch.zeros(shape, dtype=torch.int32, device=self.device) for m in self.fusion},
                 'packed': {m: [torch.zeros(shape, dtype=torch.int32).pin_memory() for _ in range(self._slots)] for m in self.fusion},
                 'tags': [torch.zeros((B, self.C), dtype=torch.int64).pin_memory() for _ in range(self._slots)],
                 'event': [None] * self._slots, 'serial': [-1] * self._slots}
            self._rings[(B, Q)] = r
        return r

    def decode(self, results, audio_tags):
        """one batch: results {at_m: (scores [B,Q], labels [B,Q] int64, boxes [B,Q,2] seconds)} as predict_step returns them,
        audio_tags [B,C] (0/1) or None.  One launch per fusion strategy into this batch shape's static buffers; nothing is read
        back (``fetch`` does that).  Returns what ``fetch`` takes: the buffers of this batch shape and the tags tensor (a captured
        graph keeps filling the same ones on every replay)."""
        B, Q = results[self.fusion[0]][0].shape
        r = self._ring(B, Q)
        for m in self.fusion:
            scores, labels, boxes = results[m]
            ops.decode_events(scores.contiguous(), labels.contiguous(), boxes.contiguous(), self.thresholds, self.C,
                              min_duration=self.min_duration, max_len=self.max_len, del_overlap=self.del_overlap, out=r['dev'][m])
        if audio_tags is not None:
            assert tuple(audio_tags.shape) == (B, self.C) and audio_tags.dtype == torch.int64, (audio_tags.shape, audio_tags.dtype)
        self._last = (r, audio_tags)
        return self._last

    def fetch(self, decoded=None):
        """enqueue the device -> host copies of the last decoded batch (or of ``decoded``, a value ``decode`` returned) on the
        current stream (one per fusion strategy, one for the tags) into the next ring slot; returns the handle whose ``rows()``
        waits for them"""
        if decoded is None:
            decoded = self._last
        if decoded is None:
            raise RuntimeError('EventDecoder.fetch: decode() first')
        r, tags = decoded
        k = r['k']
        r['k'] = (k + 1) % self._slots
        if r['event'][k] is not None:
            r['event'][k].synchronize()
        for m in self.fusion:
            r['packed'][m][k].copy_(r['dev'][m], non_blocking=True)
        if tags is not None:
            r['tags'][k].copy_(tags, non_blocking=True)
        r['event'][k] = torch.cuda.Event()
        r['event'][k].record()
        self._serial += 1
        r['serial'][k] = self._serial
        return Fetched(self, r, k, self._serial, tags is not None, self.threshold_values.copy())

    def decode_weak(self, tags):
        """BoxEncoder.decode_weak (utilities/BoxEncoder.py:163-177): the names of the classes whose tag is 1"""
        return [self.labels[i] for i, v in enumerate(np.asarray(tags).reshape(-1)) if v == 1]

    def prediction_sets(self, thresholds=None):
        """an empty PredictionSet per fusion strategy at this decoder's grid"""
        t = self.threshold_values if thresholds is None else thresholds
        return {m: PredictionSet(self.labels, t) for m in self.fusion}


def collect(fetched, filenames, tag_table, sets, labels):
    """the host half of one batch: wait for ``fetched``, add its audio-tag rows to ``tag_table`` and its events to ``sets`` {at_m:
    PredictionSet}; filenames: the batch's clips' names"""
    tags, events = fetched.rows()
    names = np.asarray(list(filenames), dtype=object)
    if tags is not None:
        b, c = np.nonzero(tags == 1)                                   # clip by clip, classes ascending: decode_weak's order
        tag_table.add(np.asarray(list(labels), dtype=object)[c], names[b])
    for m, ev in events.items():
        sets[m].add(ev, names)
