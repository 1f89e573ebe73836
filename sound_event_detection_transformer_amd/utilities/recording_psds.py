"""PSDS (utilities/psds.py holds the score's definition) on recordings of any length, on the device.  ``RecordingPsds`` is one more
consumer of the stitched event lists a ``utilities.recording.RecordingDetector`` leaves on the device, beside
``utilities.recording_metrics.RecordingMetrics``: lists in, counts out (ops.recording_psds_counts, csrc/recpsds.hip), at every
threshold of the decoder's grid - one operating point each - without per-clip records, without a criterion and without the 64
reference events per clip of PsdsMetrics.  DESIGN.md section 4 ("PSDS on recordings") holds the definition:

Scope: per fusion strategy, threshold k, recording r in the reference (a filename that is absent adds nothing; one annotated with an
empty list is evaluated: its detections can only be false positives).  Float64, plain subtract / divide / compare, comparisons >=;
inter(d, g) = min(off_d, off_g) - max(on_d, on_g) counts only where it is > 0; every term is one division added to a running sum.
  * detections of class c: the first min(count, cap) slots of the stitch output, ascending by onset and disjoint; references of class
    c': the table's list (utilities.recording_metrics.reference_table: sorted by (onset, offset, input order)), any number of them,
    and they may overlap.  A detection or a reference whose duration is not > 0 takes part in nothing.
  * DTC: p_d = sum of inter(d, g) / dur_d over the references of d's class, in table order; d passes when p_d >= dtc_threshold.
  * GTC: v_g = sum of inter(d, g) / dur_g over the detections of g's class that passed, in onset order; v_g >= gtc_threshold:
    counts[c][c] += 1.
  * CTTC and false positives, for every d that failed the DTC: for each other class c' the sum of inter(d, g) / dur_d over the
    references of class c' >= cttc_threshold: counts[class(d)][c'] += 1; independently (min(off_d, duration of r) - max(on_d, 0)) /
    dur_d >= cttc_threshold: counts[class(d)][C] += 1, the world column.
  * no limit on events: only the items that can overlap are walked - a binary search on the running maximum of the references' ends
    (``prefix_max``), one on the disjoint detections - and the kept terms are added in the order above.
  * status per (threshold, recording) and launch: 1 the lists are not complete (a stitch status, or more events than ``cap``), 4 a list
    is not ascending by onset, holds a non-finite time, or estimates overlap.  ``compute()`` raises and names the recording, the
    threshold and the reason.

DATASET CONSTANTS.  n_c (the number of reference events of class c), T_c (their summed duration; zero-length references left out of
both) and T (the summed duration of the recordings) accumulate on the host inside ``update``, over the recordings of each call that
are in the reference, and ``reset()`` zeroes them.  This differs on purpose from PsdsMetrics, which fixes them at set_reference: a
recording's length is known only when it is submitted, and it matches RecordingMetrics, whose n_ref counts only what was submitted.  A
recording submitted twice counts twice, in the counters and in the constants alike.

    psds = RecordingPsds(decoder).set_reference({'street.wav': [('Speech', 1.5, 4.25), ...]})
    both = MetricGroup(RecordingMetrics(decoder).set_reference(reference), psds)
    f1, score = engine.evaluate_recordings(detector, both, [([wave], ['street.wav'])])       # score: {at_m: PsdsResult}

``prefix_max`` and ``reference_constants`` are the host half and need no GPU."""
import math

import numpy as np
import torch

from .. import ops
from .predictions import operating_point
from .psds import SETTINGS, finish
from .scoring import RecordingReference, RecordingScorer, Uploads, prefix_max, reference_constants    # noqa: F401 (importers)


class RecordingPsds(RecordingScorer):
    """PSDS of a RecordingDetector's stitched lists against annotations, accumulated on the device at every threshold of
    ``event_decoder`` (a utilities.predictions.EventDecoder: its labels, its K thresholds - one operating point each - and its fusion
    strategies).  int64 counters [n_fusion, K, C, C + 1] on the device, PsdsMetrics' layout.  The dataset constants n_c, T_c and T
    accumulate in ``update`` over the evaluated recordings of each call - see the module docstring."""

    def __init__(self, event_decoder, dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3, device=None):
        self.decoder = event_decoder
        self.labels, self.C, self.K, self.fusion = list(event_decoder.labels), event_decoder.C, event_decoder.K, tuple(event_decoder.fusion)
        self.device = event_decoder.device if device is None else torch.device(device)
        self.dtc, self.gtc, self.cttc = float(dtc_threshold), float(gtc_threshold), float(cttc_threshold)
        if any(math.isnan(t) for t in (self.dtc, self.gtc, self.cttc)):
            raise ValueError('RecordingPsds: a tolerance criterion is NaN')
        self.counts = torch.zeros((len(self.fusion), self.K, self.C, self.C + 1), dtype=torch.int64, device=self.device)
        self._status, self._up = [], Uploads(self.device)
        self._bind(RecordingReference(self.labels, self.device))
        self._pass = None
        self._zero_constants()

    # the launch also reads 'pmax', the running maximum of the ends: built when the table is first asked for
    table = property(lambda self: self.reference.table and self.reference.with_pmax())

    def _zero_constants(self):
        self.n_gt, self.gt_dur, self.total_dur = np.zeros(self.C, np.int64), np.zeros(self.C, np.float64), 0.0

    # ------------------------------------------------------------------------------------------------------------------------
    def counters(self):
        return [self.counts]

    def reset(self):
        """zero the counters and the dataset constants and forget the statuses (start of an evaluation)"""
        self._zero_constants()
        return RecordingScorer.reset(self)

    def _durations(self, filenames, durations):
        if self.table is None:
            raise RuntimeError('RecordingPsds.update: set_reference() first')
        if durations is None or len(durations) != len(filenames):
            raise ValueError('RecordingPsds.update: PSDS needs the recordings\' durations, one per recording')
        durations = np.asarray(durations, np.float64).reshape(-1)
        if not (np.isfinite(durations).all() and (durations >= 0).all()):
            raise ValueError('RecordingPsds.update: a duration is not a finite non-negative number of seconds')
        return durations

    def account(self, filenames, durations):
        """the host half of ``update``: checks the durations, adds the call's recordings that are in the reference to n_c, T_c and T,
        and returns (rec_idx int32 [R], durations float64 [R]) as the launch takes them"""
        durations = self._durations(filenames, durations)
        idx = self.recording_index(filenames)
        rec_n, rec_t = self.reference.constants()
        for i, d in zip(idx, durations):
            if i >= 0:
                self.n_gt += rec_n[i]
                self.gt_dur += rec_t[i]
                self.total_dur += float(d)
        return idx, durations

    def update(self, stitched, cap, filenames, durations=None):
        """one detector call: ``stitched`` {at_m: (count, out, status)} and ``cap`` as ``RecordingDetector.stitch`` returns them,
        ``filenames`` the recordings' names, ``durations`` their lengths in seconds (required: the world term and T need them).  One
        launch per fusion strategy on the current stream; nothing is read back - the small status tensors stay on the device until
        compute().  n_c, T_c and T grow by the call's recordings that are in the reference (``account``)."""
        filenames = list(filenames)
        self._durations(filenames, durations)
        self._check_counts(stitched, len(filenames))
        idx, durations = self.account(filenames, durations)
        if not filenames:
            return
        d_idx = self._up('idx', idx)
        d_dur = self._up('dur', durations)
        words = self.K * len(filenames) * self.C * ((int(cap) + 63) // 64)
        if self._pass is None or self._pass.numel() < words:
            self._pass = torch.empty(words, dtype=torch.int64, device=self.device)
        thresholds = [operating_point(t) for t in self.decoder.threshold_values]
        for i, m in enumerate(self.fusion):
            count, out, st = stitched[m]
            s = ops.recording_psds_counts(count, out, st, cap, d_idx, self.table, d_dur, self.counts, i, dtc=self.dtc, gtc=self.gtc,
                                          cttc=self.cttc, pass_words=self._pass)
            self._status.append((s, filenames, thresholds, f'recording_psds_counts (fusion {m})'))

    def counts_host(self):
        """counts [n_fusion, K, C, C + 1] as numpy int64, from ONE device->host copy of counters and statuses; raises on a status,
        naming recording, threshold and reason"""
        return self._checked()[0]

    def compute(self, settings=SETTINGS):
        """{at_m: PsdsResult}: per fusion strategy the PSD scores at ``settings`` ((alpha_ct, alpha_st, max_efpr) triples), the rates
        they come from and the decoder's thresholds - PsdsMetrics.compute's result, finished by the same function (psds.finish)
        from the constants accumulated since reset()"""
        if self.table is None:
            raise RuntimeError('RecordingPsds.compute: set_reference() first')
        counts = self.counts_host()
        return {m: finish(counts[i], self.n_gt, self.gt_dur, self.total_dur, settings, self.decoder.operating_points())
                for i, m in enumerate(self.fusion)}
