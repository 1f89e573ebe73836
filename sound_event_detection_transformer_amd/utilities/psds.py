"""The polyphonic sound detection score (PSDS, Bilen et al., "A framework for the robust evaluation of sound event detection", ICASSP
2020), the DCASE Task 4 ranking metric, scored on the device from the threshold sweep's event records: what the reference's
compute_psds_from_operating_points + psds_score (utilities/metrics.py:325-330, 120-145) print, without pulling K prediction tables to
the host and without psds_eval.

``PsdsMetrics`` is bound to a utilities.predictions.EventDecoder.  It holds the reference events and the clip durations of one
validation set (uploaded once) and int64 counters [n_fusion, K, C, C + 1] on the device.  Every batch adds to them with one launch per
fusion strategy (ops.psds_update, csrc/psds.hip) that reads the packed records the decoder's launch just wrote - inside the captured
graph of engine.GraphedPredictStep(decoder=..., psds=...) - and ``compute()`` reads them back once and finishes on the host
(``psds_from_counts``, numpy float64, usable without a GPU).

THIS SCORE IS A RESTATEMENT of psds_eval's PSDSEval from its published definition, not pinned by the package: psds_eval is not
installed where this project is built and tested.  The definition it commits to, to be held against psds_eval:

Inputs per validation set: per clip k its reference events (class, onset, offset) and its duration D_k in seconds (psds_eval's
``metadata``; default: the decoder's max_len_seconds for every clip).  Every detection also gets the interval [0, D_k], which stands
for psds_eval's injected "world" label.  Dataset constants, from the whole reference table on the host in float64: n_c = number of
reference events of class c, T_c = their summed duration, T = sum of D_k over the clips present in the reference.

Per operating point (threshold of the decoder's grid) and clip, in float64 on the records' float32 onsets / offsets widened;
inter(d, g) = min(off_d, off_g) - max(on_d, on_g) counts only where it is > 0:
  1. DTC (detection tolerance criterion): p_d = sum of inter(d, g) / dur_d over the clip's reference events g of d's class, in table
     order; d passes when p_d >= dtc_threshold.
  2. GTC (ground-truth intersection criterion): v_g = sum of inter(d, g) / dur_g over the detections d of g's class that passed the
     DTC, in record order; g is a true positive when v_g >= gtc_threshold: counts[c][c] += 1.
  3. CTTC (cross-trigger tolerance criterion) and false positives, for every detection d that FAILED the DTC: for each other class
     c', sum of inter(d, g) / dur_d over the clip's reference events of class c' >= cttc_threshold: counts[class(d)][c'] += 1;
     independently, (min(off_d, D_k) - max(on_d, 0)) / dur_d >= cttc_threshold: counts[class(d)][C] += 1, the world column - a
     false positive.
Comparisons are >=; every term is a plain division added to a running sum (no contraction), so a sum that lands exactly on a
threshold does so on the device and on the host alike.  A clip outside the table (index -1, an index >= n_clips, a clip given as None)
is skipped, the rule of utilities.metrics.EventMetrics; a clip present with an empty event list is scored: its detections can only be
false positives.

Finish over counts [K, C, C + 1] (``psds_from_counts``):
  tpr[k][c] = counts[k][c][c] / n_c;  fpr[k][c] = counts[k][c][C] / T * 3600;  ctr[k][c][c'] = counts[k][c][c'] / T_c' * 3600;
  efpr[k][c] = fpr[k][c] + alpha_ct * mean over {c' != c, n_c' > 0} of ctr[k][c][c'] (an empty mean is 0).
  Per class, the K points (efpr, tpr) sorted by x, equal x keeping the largest y, y replaced by its running maximum: a step function,
  0 left of the first point, the last y held to the right.  Common axis: the sorted union of all classes' x values.
  etpr(x) = max(0, mean_c f_c(x) - alpha_st * std_c f_c(x)) (population std);  PSDS = 1 / max_efpr * integral of etpr over
  [0, max_efpr], integrated as the step function it is: points past max_efpr are dropped, the last value is held up to max_efpr.

Where this may differ from psds_eval:
  * arithmetic: float64 on the device's float32 onsets / offsets widened (psds_eval reads the decimal text of a TSV or the float32
    column of a frame as float64: the same values when the frame holds the float32 scalars, not when they were rounded to text);
  * classes without reference events (n_c = 0) are LEFT OUT of every mean here - the cross-trigger mean of efpr, the mean and std of
    etpr - instead of entering them as NaN or 0; they still own a row of ``counts`` and of the returned rates (tpr 0);
  * zero-length events: a detection or a reference event whose duration is <= 0 (an event clipped to the clip's end, a reference row
    with onset = offset) takes part in nothing - no overlap, no count, and such a reference event is not counted in n_c either;
    psds_eval divides by the duration;
  * the curve is integrated exactly as the step function defined above; psds_eval interpolates onto its own axis first, which gives
    the same area for the same points."""
import math

import numpy as np
import torch

from .. import ops
from .scoring import ClipReference, ClipScorer, read_back

SETTINGS = ((0, 0, 100), (1, 0, 100), (0, 1, 100))         # (alpha_ct, alpha_st, max_efpr) of the reference's psds_score


def _rates(counts, n_gt, gt_dur, total_dur):
    """counts [K, C, C + 1] -> (tpr [K, C], fpr [K, C], ctr [K, C, C], valid [C]): the rates of the module docstring; a class without
    reference events has tpr 0 and a zero ctr column, the diagonal of ctr is 0"""
    counts = np.asarray(counts)
    n_gt, gt_dur = np.asarray(n_gt, dtype=np.float64).reshape(-1), np.asarray(gt_dur, dtype=np.float64).reshape(-1)
    C = n_gt.size
    if counts.ndim != 3 or counts.shape[1:] != (C, C + 1) or gt_dur.size != C or counts.shape[0] < 1:
        raise ValueError(f'psds: counts {counts.shape} is not [K >= 1, C, C + 1] for the {C} classes of n_gt / {gt_dur.size} of gt_dur')
    valid = n_gt > 0
    if not valid.any():
        raise ValueError('psds: no class has a reference event (n_c = 0 for every class)')
    if (gt_dur[valid] <= 0).any() or not np.isfinite(gt_dur[valid]).all():
        raise ValueError('psds: a class with reference events has no positive finite reference duration T_c')
    if not (math.isfinite(total_dur) and total_dur > 0):
        raise ValueError(f'psds: the total duration T = {total_dur!r} is not a positive number of seconds')
    cnt = counts.astype(np.float64)
    k = np.arange(C)
    tpr = np.zeros(cnt.shape[:2])
    tpr[:, valid] = cnt[:, k, k][:, valid] / n_gt[valid]
    fpr = cnt[:, :, C] / float(total_dur) * 3600.0
    ctr = np.zeros((cnt.shape[0], C, C))
    ctr[:, :, valid] = cnt[:, :, :C][:, :, valid] / gt_dur[valid] * 3600.0
    ctr[:, k, k] = 0.0
    return tpr, fpr, ctr, valid


def _curve(tpr, fpr, ctr, valid, alpha_ct, alpha_st, max_efpr):
    """(psds, efpr axis, etpr on it) of the module docstring's finish; the axis is not cut at max_efpr"""
    if not (math.isfinite(max_efpr) and max_efpr > 0):
        raise ValueError(f'psds: max_efpr {max_efpr!r} is not a positive number of false positives per hour')
    classes = np.nonzero(valid)[0]
    curves = []
    for c in classes:
        others = [o for o in classes if o != c]
        cross = ctr[:, c, others].mean(axis=1) if others else 0.0
        x, y = fpr[:, c] + alpha_ct * cross, tpr[:, c]
        order = np.lexsort((y, x))                                     # by x, then y: the last of equal x holds the largest y
        x, y = x[order], y[order]
        last = np.append(x[1:] != x[:-1], True)
        curves.append((x[last], np.maximum.accumulate(y[last])))
    axis = np.unique(np.concatenate([x for x, _ in curves]))
    f = np.zeros((len(curves), axis.size))
    for i, (x, y) in enumerate(curves):
        at = np.searchsorted(x, axis, side='right') - 1               # the last point at or left of each axis value
        f[i] = np.where(at >= 0, y[np.maximum(at, 0)], 0.0)
    etpr = np.maximum(0.0, f.mean(axis=0) - alpha_st * f.std(axis=0))
    inside = axis <= max_efpr
    edges = np.append(axis[inside], float(max_efpr))
    return float((etpr[inside] * np.diff(edges)).sum() / float(max_efpr)), axis, etpr


def psds_from_counts(counts, n_gt, gt_dur, total_dur, alpha_ct=0, alpha_st=0, max_efpr=100):
    """the PSD score of the confusion counts [K, C, C + 1] of K operating points (module docstring, "Finish"): n_gt [C] the number
    n_c and gt_dur [C] the summed duration T_c (seconds) of every class's reference events, total_dur the summed clip duration T.
    Pure numpy float64.  Refuses a dataset in which no class has a reference event, and max_efpr <= 0."""
    return _curve(*_rates(counts, n_gt, gt_dur, total_dur), alpha_ct, alpha_st, max_efpr)[0]


class PsdsResult(dict):
    """one fusion strategy's scores: {'psds': {(alpha_ct, alpha_st, max_efpr): value}, 'tpr' [K, C], 'fpr' [K, C] (per hour),
    'ctr' [K, C, C] (per hour), 'thresholds' [K] (of a class-wise decoder: a tuple of C floats each)}; ``curve(setting)`` gives the
    PSD-ROC of a setting"""

    def curve(self, setting=SETTINGS[0]):
        """(efpr, etpr): the common axis (per hour, not cut at max_efpr) and the effective true positive rate on it, a step function
        holding each value up to the next axis point"""
        alpha_ct, alpha_st, max_efpr = setting
        return _curve(self['tpr'], self['fpr'], self['ctr'], self._valid, alpha_ct, alpha_st, max_efpr)[1:]


def finish(counts, n_gt, gt_dur, total_dur, settings, thresholds):
    """one fusion strategy's PsdsResult from its counts [K, C, C + 1] and the dataset constants: the PSD scores at ``settings``
    ((alpha_ct, alpha_st, max_efpr) triples), the rates they come from and the decoder's ``thresholds``"""
    tpr, fpr, ctr, valid = _rates(counts, n_gt, gt_dur, total_dur)
    r = PsdsResult(psds={tuple(s): _curve(tpr, fpr, ctr, valid, *s)[0] for s in settings}, tpr=tpr, fpr=fpr, ctr=ctr,
                   thresholds=thresholds)
    r._valid = valid
    return r


class PsdsMetrics(ClipScorer):
    """PSDS accumulated on the device from ``decoder``'s event records (a utilities.predictions.EventDecoder: its labels, its K
    thresholds - one operating point each - and its fusion strategies).  See the module docstring for what is counted."""

    def __init__(self, decoder, dtc_threshold=0.5, gtc_threshold=0.5, cttc_threshold=0.3):
        self.decoder = decoder
        self.labels, self.C, self.K, self.fusion, self.device = decoder.labels, decoder.C, decoder.K, decoder.fusion, decoder.device
        self.dtc, self.gtc, self.cttc = float(dtc_threshold), float(gtc_threshold), float(cttc_threshold)
        if any(math.isnan(t) for t in (self.dtc, self.gtc, self.cttc)):
            raise ValueError('PsdsMetrics: a tolerance criterion is NaN')
        self.counts = torch.zeros((len(self.fusion), self.K, self.C, self.C + 1), dtype=torch.int64, device=self.device)
        self.max_len = decoder.max_len
        self._bind(ClipReference(self.labels, self.device))

    n_gt = property(lambda self: self.reference.n_gt)               # PSDS' n_c, T_c and T: the reference's
    gt_dur = property(lambda self: self.reference.gt_dur)
    total_dur = property(lambda self: self.reference.total_dur)

    def set_reference(self, events, durations=None):
        return self._set_reference(events, durations)

    def counters(self):
        return [self.counts]

    def update(self, decoded, clip_idx):
        """one batch: what ``EventDecoder.decode`` returned for it and clip_idx [B], the clips' indices in the reference (-1: none).
        One launch per fusion strategy on the records still on the device; nothing is read back."""
        for i, records, idx in self._records(decoded, clip_idx):
            ops.psds_update(records, idx, self.table, self.n_clips, self.max_ref, self.C, self.counts, i, dtc=self.dtc, gtc=self.gtc,
                            cttc=self.cttc)

    def counts_host(self):
        """counts [n_fusion, K, C, C + 1] as numpy int64: ONE device->host copy"""
        return read_back(self.counters())[0]

    def compute(self, settings=SETTINGS):
        """{at_m: PsdsResult}: per fusion strategy the PSD scores at ``settings`` ((alpha_ct, alpha_st, max_efpr) triples; the default
        is the reference's three), the rates they come from and the decoder's thresholds; one device->host copy"""
        if self.n_gt is None:
            raise RuntimeError('PsdsMetrics.compute: set_reference() first')
        counts = self.counts_host()
        return {m: finish(counts[i], self.n_gt, self.gt_dur, self.total_dur, settings, self.decoder.operating_points())
                for i, m in enumerate(self.fusion)}
