"""The operating point of a validation set, found on the device: the event-based and clip-level counts of utilities.metrics.EventMetrics
at EVERY threshold of an EventDecoder's grid from one validation pass, the F1-versus-threshold curve of every class they give, and the
choice of one decision threshold per class from it - what the reference leaves to a re-run per grid point (its decode is fixed at
0.5; its own get_pseudo_labels / adjust_threshold / get_f_measure_by_class take one threshold per class).

``SweepEventMetrics`` is bound to a utilities.predictions.EventDecoder.  It holds the reference events of one validation set (uploaded
once) and int64 counters ev / tag [n_fusion, K, C, 3] on the device.  Every batch adds to them with one launch per fusion strategy
(ops.event_sweep_update, csrc/sweep.hip) that reads the packed records the decoder's launch just wrote - inside the captured graph of
engine.GraphedPredictStep(decoder=..., sweep=...) - and ``compute()`` reads them back once and finishes on the host.

What is counted is EventMetrics' event-based and clip-level part (see utilities/metrics.py), at threshold k on the events the decoder
wrote at k: ev[k] and tag[k] equal the counters of an EventMetrics(threshold=grid[k]) fed the same batches.  Scores follow
utilities.metrics.finalize: F = 2 tp / (n_ref + n_sys), 0 on a zero denominator, the macro average at k over the classes that occur in
the reference or in the estimates at k.

Choosing thresholds (``select_class_wise``, a pure host function of the counts): decode and matching are both class by class, so the
counts of class c under class-wise thresholds tau equal the counts of class c under the uniform threshold tau_c.  Per class the point
with the best class F1 is taken; the macro F1 promised is exactly the one a class-wise decoder set to the chosen thresholds
(EventDecoder(class_wise=True)) delivers on the same set."""
import numpy as np
import torch

from .. import ops
from .metrics import _class_scores, _macro, _ratio, _tag_scores
from .predictions import operating_point
from .scoring import ClipReference, ClipScorer, read_back


def _grid_2d(threshold_values, K, C):
    """the candidates of every class as [K, C] float64: a [K] grid holds the same ones for every class"""
    t = np.asarray(threshold_values, dtype=np.float64)
    if t.ndim == 1:
        t = np.repeat(t.reshape(-1, 1), C, axis=1)
    if t.shape != (K, C):
        raise ValueError(f'operating points: thresholds {t.shape} for counts of {K} points x {C} classes')
    return t


def class_f1(ev):
    """ev [K, C, 3] {tp, n_ref, n_sys} -> the event-based F1 of every class at every point [K, C] (0 on a zero denominator)"""
    ev = np.asarray(ev)
    return np.array([[_ratio(2 * int(tp), int(nr) + int(ns)) for tp, nr, ns in row] for row in ev], dtype=np.float64).reshape(ev.shape[:2])


def select_class_wise(ev, threshold_values, default=0.5):
    """one threshold per class from the event-based counts ev [K, C, 3] {tp, n_ref, n_sys} of K operating points; threshold_values
    [K] (every class has the same candidates) or [K, C] (class c's candidates are threshold_values[:, c]).  Pure numpy.
    Per class with a reference event: the point with the largest class F1; ties go to the tied point whose threshold for that class
    is nearest ``default``, then to the lower threshold, then to the lower index.  A class with no reference event in the set keeps
    ``default`` and index -1.
    Returns {'index' [C] int64, 'thresholds' [C] float64, 'class_f1' [C], 'f1'}: 'f1' is the macro average of class_f1 over the
    classes that occur in the reference, or in any estimate at their chosen point - for a class without reference events that point is
    the grid point whose threshold for it equals ``default`` as float32, and the class is left out when the grid holds no such point
    (nothing was decoded at ``default``).  n_ref does not depend on the point; row 0 is read."""
    ev = np.asarray(ev)
    if ev.ndim != 3 or ev.shape[2] != 3 or ev.shape[0] < 1:
        raise ValueError(f'operating points: counts {ev.shape} are not [K >= 1, C, 3]')
    K, C = ev.shape[:2]
    t = _grid_2d(threshold_values, K, C)
    default = float(default)
    f = class_f1(ev)
    index, chosen, best, counted = np.full(C, -1, np.int64), np.full(C, default, np.float64), np.zeros(C, np.float64), []
    for c in range(C):
        if ev[0, c, 1] > 0:
            tied = np.nonzero(f[:, c] == f[:, c].max())[0]
            k = min(tied.tolist(), key=lambda i: (abs(t[i, c] - default), t[i, c], i))
            index[c], chosen[c], best[c] = k, t[k, c], f[k, c]
            counted.append(c)
        else:
            at = np.nonzero(t[:, c].astype(np.float32) == np.float32(default))[0]
            if at.size and ev[at[0], c, 2] > 0:                          # estimates of a class the reference does not hold: F1 0
                counted.append(c)
    return {'index': index, 'thresholds': chosen, 'class_f1': best, 'f1': float(np.mean(best[counted])) if counted else 0.0}


class SweepResult(object):
    """one fusion strategy's scores at every operating point: ``thresholds`` [K] (floats, or tuples of C floats of a class-wise
    decoder) and ``threshold_values`` ([K] or [K, C] float32), ``class_f1`` / ``class_precision`` / ``class_recall`` [K, C], the macro
    ``f1`` / ``precision`` / ``recall`` [K], the clip-level macro ``clip_f1`` [K], and the counts ``ev`` / ``tag`` [K, C, 3]"""

    def __init__(self, ev, tag, threshold_values, labels):
        self.ev, self.tag = np.asarray(ev), np.asarray(tag)
        K, C = self.ev.shape[:2]
        self.threshold_values = np.asarray(threshold_values, dtype=np.float32)
        _grid_2d(self.threshold_values, K, C)
        self.thresholds = [operating_point(t) for t in self.threshold_values]
        self.labels = list(labels)
        self.class_f1, self.class_precision, self.class_recall = (np.zeros((K, C)) for _ in range(3))
        self.f1, self.precision, self.recall, self.clip_f1 = (np.zeros(K) for _ in range(4))
        every = np.ones(C, dtype=bool)
        for k in range(K):
            cw = _class_scores(self.ev[k], every, self.labels)
            for c, l in enumerate(self.labels):
                self.class_f1[k, c], self.class_precision[k, c], self.class_recall[k, c] = (cw[l][s] for s in ('f1', 'precision', 'recall'))
            present = (self.ev[k, :, 1] > 0) | (self.tag[k, :, 0] + self.tag[k, :, 1] > 0)    # in a reference, or decoded in any clip
            m = _macro({l: cw[l] for c, l in enumerate(self.labels) if present[c]})
            self.f1[k], self.precision[k], self.recall[k] = m['f1'], m['precision'], m['recall']
            self.clip_f1[k] = _tag_scores(self.tag[k], self.labels)['f1']

    def best_uniform(self):
        """(k, threshold, f1): the operating point with the largest macro F1, ties to the lowest k"""
        k = int(np.argmax(self.f1))
        return k, self.thresholds[k], float(self.f1[k])

    def best_class_wise(self, default=0.5):
        """``select_class_wise`` on these counts and this grid"""
        return select_class_wise(self.ev, self.threshold_values, default)


class SweepEventMetrics(ClipScorer):
    """EventMetrics' event-based and clip-level counts at every operating point of ``decoder`` (a utilities.predictions.EventDecoder:
    its labels, its K thresholds, its fusion strategies), accumulated on the device from its event records.  ``t_collar``,
    ``percentage_of_length`` and ``optimal`` are EventMetrics'.  See the module docstring."""

    def __init__(self, decoder, t_collar=0.2, percentage_of_length=0.2, optimal=True):
        self.decoder = decoder
        self.labels, self.C, self.K, self.fusion, self.device = decoder.labels, decoder.C, decoder.K, decoder.fusion, decoder.device
        self.t_collar, self.pct, self.optimal = float(t_collar), float(percentage_of_length), bool(optimal)
        shape = (len(self.fusion), self.K, self.C, 3)
        self.ev = torch.zeros(shape, dtype=torch.int64, device=self.device)
        self.tag = torch.zeros(shape, dtype=torch.int64, device=self.device)
        self.max_len = decoder.max_len
        self._bind(ClipReference(self.labels, self.device))

    def counters(self):
        return [self.ev, self.tag]

    def update(self, decoded, clip_idx):
        """one batch: what ``EventDecoder.decode`` returned for it and clip_idx [B], the clips' indices in the reference (-1: none).
        One launch per fusion strategy on the records still on the device; nothing is read back."""
        for i, records, idx in self._records(decoded, clip_idx):
            ops.event_sweep_update(records, idx, self.table, self.n_clips, self.max_ref, self.C, self.ev, self.tag, i,
                                   t_collar=self.t_collar, pct=self.pct, optimal=self.optimal)

    def counts(self):
        """(ev [n_fusion, K, C, 3] {tp, n_ref, n_sys}, tag [n_fusion, K, C, 3] {tp, fp, fn}) as numpy int64: ONE device->host copy"""
        return tuple(read_back(self.counters()))

    def compute(self):
        """{at_m: SweepResult}: per fusion strategy the scores at every operating point of the decoder's grid as it stands; one
        device->host copy"""
        ev, tag = self.counts()
        return {m: SweepResult(ev[i], tag[i], self.decoder.threshold_values.copy(), self.labels) for i, m in enumerate(self.fusion)}
