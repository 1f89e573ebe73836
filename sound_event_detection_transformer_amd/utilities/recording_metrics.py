"""Recordings of any length scored against their annotations, on the device.  ``utilities.recording.RecordingDetector`` leaves one
stitched event list per (threshold, recording, class) on the device; ``RecordingMetrics`` is one more consumer of those lists: lists
in, counts out (ops.recording_event_counts / ops.recording_segment_counts, csrc/recmetrics.hip), at every threshold of the decoder's
grid, without per-clip records, without a criterion and without the per-clip limits of EventMetrics (64 reference events, 1024
segments).  DESIGN.md section 4 ("Scoring recordings") holds the definition:

Scope: per fusion strategy, threshold k, recording r, class c.  Float64, plain subtract / multiply / divide / compare.
  * estimates: the first count[k][r][c] slots of the stitch output, as stitch wrote them (no second clip, no duration filter),
    ascending by onset and disjoint.  References: the recording's annotated events of class c, sorted here by (onset, offset, input
    order); any number of them, and those of one class may overlap.
  * evaluated recordings: only those with an entry in the reference; a filename that is absent adds nothing anywhere (deliberately
    simpler than the clip-level outer merge of EventMetrics).  A recording annotated with an empty list is evaluated: its estimates
    count as n_sys, as false positives and as I.
  * event-based {tp, n_ref, n_sys}: sed_eval's hit test (|on_r - on_e| <= t_collar, |off_r - off_e| <= max(t_collar, pct * (off_r -
    on_r))); tp = the size of a maximum-cardinality matching of the hit graph of class c over the WHOLE recording; ``optimal=False``
    selects sed_eval's greedy pass (references in table order, each takes the first estimate in onset order still free that it
    hits).  No limit on events: the two lists are merged by onset and cut into blocks wherever two consecutive onsets differ by more
    than t_collar (no hit crosses such a cut, so the matching is the sum over the blocks); a block of more than 64 references or 64
    estimates raises a status, it is never silently mis-counted.
  * recording-level presence {tp, fp, fn} per class: "count[k][r][c] > 0" against "class c has a reference event in r".
  * with ``time_resolution`` = rho, segment-based {tp, n_ref, n_sys} and {S, D, I} as EventMetrics documents them (an event is active
    in floor(on / rho) <= s < ceil(off / rho), float64 divisions), over ceil(max(recording duration, largest reference offset) /
    rho) segments - any number of them.  Negative reference times are refused.
  * status per (threshold, recording) and launch: 1 the lists are not complete (a stitch status, or more events than ``cap``), 4 a list
    is not ascending by onset or holds a non-finite time, 2 a block over capacity.  ``compute()`` raises and names the recording,
    the threshold and the reason.

    metrics = RecordingMetrics(decoder, time_resolution=1.0).set_reference({'street.wav': [('Speech', 1.5, 4.25), ...]})
    scores = engine.evaluate_recordings(detector, metrics, [([wave], ['street.wav'])])      # {at_m: [per threshold: finalize's dict]}
    best = metrics.class_wise_thresholds(1)                                                  # one threshold per class, no criterion

``reference_table``, ``finish`` and ``status_error`` are the host half and need no GPU."""
import math

import numpy as np
import torch

from .. import ops
from .metrics import finalize
from .operating_points import select_class_wise
from .predictions import operating_point
from .scoring import STATUS_REASONS, RecordingReference, RecordingScorer, Uploads, reference_table, status_error    # noqa: F401

MAX_WORDS = (1 << 25) - 1          # 64-segment words of one recording (csrc/recmetrics.hip: SEDT_RM_MAXWORDS)


def segment_words(rec_dur, max_end, time_resolution):
    """the 64-segment words a recording spans: ceil(ceil(max(rec_dur, largest reference offset) / rho) / 64) (float64 division)"""
    n = math.ceil(max(float(rec_dur), float(max_end), 0.0) / float(time_resolution))
    words = -(-n // 64)
    if words > MAX_WORDS:
        raise ValueError(f'{max(float(rec_dur), float(max_end))} s at time_resolution {time_resolution} s are {n} segments: more than '
                         f'int32 indexing holds ({MAX_WORDS * 64})')
    return words


def finish(ev, tag, labels, fusion, seg=None, sdi=None):
    """counter arrays ev / tag [n_fusion, K, C, 3] (and seg [n_fusion, K, C, 3], sdi [n_fusion, K, 3]) -> {at_m: [per threshold what
    utilities.metrics.finalize returns for that threshold's slices]}: the recording-level presence scores under its 'clip' key"""
    K = ev.shape[1]
    per_k = [finalize(ev[:, k], tag[:, k], labels, fusion, at_counted=False,
                      **({} if seg is None else dict(seg=seg[:, k], sdi=sdi[:, k]))) for k in range(K)]
    return {m: [per_k[k][m] for k in range(K)] for m in fusion}


class RecordingMetrics(RecordingScorer):
    """event-based, recording-level and (with ``time_resolution``) segment-based counts of a RecordingDetector's stitched lists against
    annotations, at every threshold of ``event_decoder`` (a utilities.predictions.EventDecoder: its labels, its K thresholds, its
    fusion strategies).  int64 counters on the device: ev / tag [n_fusion, K, C, 3], seg [n_fusion, K, C, 3], sdi [n_fusion, K, 3].
    See the module docstring."""

    def __init__(self, event_decoder, t_collar=0.2, percentage_of_length=0.2, optimal=True, time_resolution=None, device=None):
        self.decoder = event_decoder
        self.labels, self.C, self.K, self.fusion = list(event_decoder.labels), event_decoder.C, event_decoder.K, tuple(event_decoder.fusion)
        self.device = event_decoder.device if device is None else torch.device(device)
        self.t_collar, self.pct, self.optimal = float(t_collar), float(percentage_of_length), bool(optimal)
        if not (0.0 <= self.t_collar < float('inf')) or math.isnan(self.pct):
            raise ValueError(f'RecordingMetrics: t_collar {t_collar!r} is not a finite number >= 0 (or percentage_of_length is NaN)')
        self.time_resolution = None if time_resolution is None else float(time_resolution)
        if self.time_resolution is not None and not (math.isfinite(self.time_resolution) and self.time_resolution > 0):
            raise ValueError(f'RecordingMetrics: time_resolution {time_resolution!r} is not a positive number of seconds')
        shape = (len(self.fusion), self.K, self.C, 3)
        self.ev = torch.zeros(shape, dtype=torch.int64, device=self.device)
        self.tag = torch.zeros(shape, dtype=torch.int64, device=self.device)
        self.seg = self.sdi = None
        if self.time_resolution is not None:
            self.seg = torch.zeros(shape, dtype=torch.int64, device=self.device)
            self.sdi = torch.zeros((len(self.fusion), self.K, 3), dtype=torch.int64, device=self.device)
        self._status, self._up = [], Uploads(self.device)
        self._bind(RecordingReference(self.labels, self.device))

    # ------------------------------------------------------------------------------------------------------------------------
    def counters(self):
        """every device counter tensor: [ev, tag] (+ [seg, sdi] with segment-based scores)"""
        return [t for t in (self.ev, self.tag, self.seg, self.sdi) if t is not None]

    def update(self, stitched, cap, filenames, durations=None):
        """one detector call: ``stitched`` {at_m: (count, out, status)} and ``cap`` as ``RecordingDetector.stitch`` returns them,
        ``filenames`` the recordings' names, ``durations`` their lengths in seconds (needed with ``time_resolution``: the plan's
        rec_dur).  One launch per fusion strategy, one more each with segments, on the current stream; nothing is read back - the
        small status tensors stay on the device until compute()."""
        if self.table is None:
            raise RuntimeError('RecordingMetrics.update: set_reference() first')
        filenames = list(filenames)
        idx = self.recording_index(filenames)
        words = None
        if self.seg is not None:
            if durations is None or len(durations) != len(filenames):
                raise ValueError('RecordingMetrics.update: segment-based counts need the recordings\' durations, one per recording')
            words = [segment_words(d, self.host['max_end'][i] if i >= 0 else 0.0, self.time_resolution) for d, i in zip(durations, idx)]
        self._check_counts(stitched, len(filenames))
        if not filenames:
            return
        d_idx = self._up('idx', idx)
        d_words = None if words is None else self._up('words', np.asarray(words, np.int32))
        thresholds = [operating_point(t) for t in self.decoder.threshold_values]
        for i, m in enumerate(self.fusion):
            count, out, st = stitched[m]
            s = ops.recording_event_counts(count, out, st, cap, d_idx, self.table, self.ev, self.tag, i, t_collar=self.t_collar,
                                           pct=self.pct, optimal=self.optimal)
            self._status.append((s, filenames, thresholds, f'recording_event_counts (fusion {m})'))
            if self.seg is not None:
                s = ops.recording_segment_counts(count, out, st, cap, d_idx, self.table, d_words, self.seg, self.sdi, i,
                                                 time_resolution=self.time_resolution)
                self._status.append((s, filenames, thresholds, f'recording_segment_counts (fusion {m})'))

    def counts(self):
        """(ev [n_fusion, K, C, 3] {tp, n_ref, n_sys}, tag [n_fusion, K, C, 3] {tp, fp, fn}) as numpy int64; one device->host copy;
        raises on a status"""
        return tuple(self._checked()[:2])

    def segment_counts(self):
        """(seg [n_fusion, K, C, 3] {tp, n_ref, n_sys}, sdi [n_fusion, K, 3] {S, D, I}) as numpy int64, None without time_resolution"""
        if self.seg is None:
            return None
        return tuple(self._checked()[2:])

    def compute(self):
        """{at_m: [per threshold {'f1', 'precision', 'recall', 'class_wise', 'clip': {...}[, 'segment': {...}]}]}: what
        utilities.metrics.finalize returns for every threshold's slices of the counters, the recording-level presence scores under
        'clip'.  One device->host copy of counters and statuses; raises on a status, naming recording, threshold and reason."""
        got = self._checked()
        seg = {} if self.seg is None else dict(seg=got[2], sdi=got[3])
        return finish(got[0], got[1], self.labels, self.fusion, **seg)

    def class_wise_thresholds(self, m, default=0.5):
        """operating_points.select_class_wise on fusion strategy ``m``'s event-based counts and the decoder's grid: one threshold per
        class tuned on recordings, without a criterion"""
        ev = self.counts()[0][self.fusion.index(m)]
        return select_class_wise(ev, self.decoder.threshold_values.copy(), default)


class MetricGroup(object):
    """several consumers of one detector pass's stitched lists behind the interface ``RecordingDetector.submit(..., metrics=)`` and
    ``engine.evaluate_recordings`` call - a RecordingMetrics and a utilities.recording_psds.RecordingPsds, say, each with its reference
    set: ``reset`` and ``update`` go to every member in order, ``compute`` returns the tuple of the members' results."""

    def __init__(self, *metrics):
        if not metrics:
            raise ValueError('MetricGroup: no members')
        self.metrics = tuple(metrics)

    def reset(self):
        for m in self.metrics:
            m.reset()
        return self

    def update(self, stitched, cap, filenames, durations=None):
        for m in self.metrics:
            m.update(stitched, cap, filenames, durations=durations)

    def compute(self):
        return tuple(m.compute() for m in self.metrics)
