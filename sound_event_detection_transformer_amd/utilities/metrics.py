"""Validation scores on the device: event-based and clip-level macro F1 of the reference's engine.evaluate (engine.py:199-297,
utilities/metrics.py:43-80, 147-157, 281-322), and with ``time_resolution`` the segment-based scores of its final test
(``evaluate(..., cal_seg=True, cal_clip=True)``: metrics.py:83-116, 333-363), without the host decode (BoxEncoder.decode_strong, pandas,
sed_eval).

``EventMetrics`` holds the reference events of one validation set (uploaded once) and int64 counters on the device.  Every batch adds to
the counters with one launch per fusion strategy (ops.event_metrics_update, csrc/metrics.hip) - inside the captured graph of
engine.GraphedPredictStep(metrics=...) - and ``compute()`` reads them back once and finalizes on the host.

What is counted, as the reference does it:
  * decode_strong(threshold=0.5, del_overlap) on PostProcess's outputs, events shorter than min_duration dropped, onsets / offsets
    clipped to [0, max_len_seconds];
  * sed_eval EventBasedMetrics(t_collar=0.2, percentage_of_length=0.2), onset and offset evaluated, class-wise tp from a
    maximum-cardinality matching (sed_eval's default event_matching_type='optimal'; ``optimal=False`` selects its greedy pass).
    Only clips that have a row in the reference are evaluated (metrics.py:58): a clip given as ``None`` in ``set_reference`` adds
    nothing here, not even its false positives.  A clip given with an empty event list (a reference row without a label) is
    evaluated and its estimates count as false positives;
  * clip level (audio_tagging_results through format_df): per clip and class "present among the decoded events" against "present
    among the reference events", over the outer merge of the two file lists - so here every clip counts, and a clip without a
    reference row contributes its false positives;
  * the audio-tag head (engine.py:203-206): the same clip-level counts with the thresholded ``at`` tags;
  * with ``time_resolution=r`` (the reference's final test uses 1.0; ``None``, the default, counts no segments): sed_eval
    SegmentBasedMetrics(time_resolution=r) on the same evaluated clips, decoded and clipped estimates and reference events.  An
    event (c, on, off) makes class c active in the segments floor(on / r) <= k < ceil(off / r), both quotients float64 divisions as
    in sed_eval's event roll (0.3 / 0.1 = 2.9999999999999996: floor 2); events of one class OR together, an empty range sets
    nothing.  Class-wise: tp / n_ref / n_sys = segments where the class is active in both / the reference / the estimates.  Per
    segment over the classes: S += min(Nref, Nsys) - Ntp, D += max(0, Nref - Nsys), I += max(0, Nsys - Nref).  A clip holds at most
    MAX_SEGMENTS segments: ``set_reference`` refuses ceil(max(max_len_seconds, largest reference offset) / r) above that, and
    negative reference times (sed_eval's roll would wrap them around the clip).

Macro averages run over the classes the reference's tables contain: those occurring in the references or in the estimates
(metrics.py:60-63, 97-100, 283-287), not over all C classes.  F = 2 tp / (n_ref + n_sys) (event, segment) or 2 tp / (2 tp + fp + fn)
(clip), 0 when the denominator is 0; precision and recall likewise 0 on a zero denominator, and so are the segment-based overall
scores and error rates (sed_eval guards its denominators with machine epsilon, which moves a value by a few ulps; pandas gives NaN
for the clip-level precision / recall of such a class)."""
import math

import numpy as np
import torch

from .. import ops
from .scoring import GENERATION, MAX_REF_EVENTS, ClipReference, ClipScorer, read_back    # noqa: F401 (MAX_REF_EVENTS: importers)

MAX_SEGMENTS = 1024        # segments of one clip the segment-based counts hold (csrc/metrics.hip: SEDT_EM_MAXSEG)
SUMMARY_COLUMNS = ('Eb_F1', 'Eb_P', 'Eb_R', 'Sb_F', 'Sb_P', 'Sb_R', 'At_F1')      # the reference's "All Metrics" row


def reference_events(rows, filenames):
    """the reference TSV rows (filename, onset, offset, event_label) -> the list ``set_reference`` takes, aligned with ``filenames``
    (the dataset's clip order): per clip the [(label, onset, offset)] of its rows, [] for a file whose only row has no label
    (metrics.py:33-34), None for a file absent from the rows (not evaluated)."""
    per = {}
    for fname, onset, offset, label in rows:
        ev = per.setdefault(fname, [])
        if label is None or (isinstance(label, float) and math.isnan(label)):
            continue
        ev.append((label, float(onset), float(offset)))
    return [per.get(f) for f in filenames]


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


class EventMetrics(ClipScorer):
    """engine.evaluate's scores accumulated on the device.  ``labels``: the class names in the model's class order (decoder.labels);
    ``fusion_strategy``: the PostProcess fusion modes the predict step runs, in its order (results are keyed by them);
    ``time_resolution``: seconds per segment of the segment-based scores, None for none."""

    def __init__(self, labels, max_len_seconds, t_collar=0.2, percentage_of_length=0.2, threshold=0.5, min_duration=0.2,
                 del_overlap=True, fusion_strategy=(1,), optimal=True, device=None, time_resolution=None):
        self.labels = list(labels)
        self.C = len(self.labels)
        assert 1 <= self.C <= 63, 'EventMetrics: 1..63 classes'
        self.max_len = float(max_len_seconds)
        self.t_collar, self.pct = float(t_collar), float(percentage_of_length)
        self.threshold, self.min_duration = float(threshold), float(min_duration)
        self.del_overlap, self.optimal = bool(del_overlap), bool(optimal)
        self.fusion = tuple(fusion_strategy)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        nf = len(self.fusion)
        self.ev = torch.zeros((nf, self.C, 3), dtype=torch.int64, device=self.device)
        self.tag = torch.zeros((nf + 1, self.C, 3), dtype=torch.int64, device=self.device)
        self.time_resolution = None if time_resolution is None else float(time_resolution)
        self.seg = self.sdi = None
        if self.time_resolution is not None:
            self.seg = torch.zeros((nf, self.C, 3), dtype=torch.int64, device=self.device)
            self.sdi = torch.zeros((nf, 3), dtype=torch.int64, device=self.device)
        self.n_seg_words, self.at_counted = 0, False
        self._bind(ClipReference(self.labels, self.device))

    # ------------------------------------------------------------------------------------------------------------------------
    def _segment_words(self, host, n_events):
        """this scorer's own checks on a reference's host arrays: the 64-segment words of a clip, 0 without time_resolution"""
        if self.time_resolution is None:
            return 0
        if not (math.isfinite(self.time_resolution) and self.time_resolution > 0):
            raise ValueError(f'set_reference: time_resolution {self.time_resolution!r} is not a positive number of seconds')
        on, end = host['on'][:n_events], host['end'][:n_events]
        bad = np.nonzero((on < 0) | (end < 0))[0]
        if bad.size:
            j = int(bad[0])
            k = int(np.searchsorted(host['off'], j, side='right')) - 1
            raise ValueError(f'set_reference: clip {k}: negative event time ({on[j]}, {end[j]}) in a segment-based evaluation')
        longest = max([self.max_len] + end.tolist())
        q = longest * 1 / self.time_resolution                              # the longest event roll, as sed_eval sizes it
        if not q <= MAX_SEGMENTS:
            raise ValueError(f'set_reference: {longest} s at time_resolution {self.time_resolution} s is more '
                             f'than {MAX_SEGMENTS} segments per clip')
        return max(1, -(-math.ceil(q) // 64))

    _accepts = _segment_words         # asked before the reference changes, whoever sets it: a refusal leaves the table as it was

    def _adopted(self):
        """the table was set, or the scorer holds another: the segment words follow it, and with them the generation"""
        ref = self.reference
        words = 0 if ref.host is None else self._segment_words(ref.host, ref.n_events)
        if words != self.n_seg_words:
            self.n_seg_words, self._generation = words, next(GENERATION)

    def counters(self):
        """every device counter tensor: [ev, tag] (+ [seg, sdi] with segment-based scores)"""
        return [t for t in (self.ev, self.tag, self.seg, self.sdi) if t is not None]

    def _read(self):
        """every counter as numpy int64, in the order of counters(): ONE device->host copy (scoring.read_back)"""
        return read_back(self.counters())

    def update(self, results, audio_tags, clip_idx):
        """one batch: results {at_m: (scores [B,Q], labels [B,Q] int64, boxes [B,Q,2] seconds)} as predict_step returns them,
        audio_tags [B,C] (0/1, or None), clip_idx [B] (the clips' indices in the reference, -1 = no reference row).  One launch per
        fusion strategy; nothing is read back."""
        if self.table is None:
            raise RuntimeError('EventMetrics.update: set_reference() first')
        idx = self.clip_index(clip_idx)
        tags = None if audio_tags is None else audio_tags.to(torch.int64).contiguous()
        self.at_counted = self.at_counted or tags is not None
        seg = {} if self.seg is None else dict(seg_counts=self.seg, sdi_counts=self.sdi, time_resolution=self.time_resolution,
                                               n_seg_words=self.n_seg_words)
        for i, m in enumerate(self.fusion):
            scores, labels, boxes = results[m]
            ops.event_metrics_update(scores.contiguous(), labels.contiguous(), boxes.contiguous(), tags if i == 0 else None, idx,
                                     self.table, self.n_clips, self.max_ref, self.ev, self.tag, i, threshold=self.threshold,
                                     min_duration=self.min_duration, max_len=self.max_len, t_collar=self.t_collar, pct=self.pct,
                                     del_overlap=self.del_overlap, optimal=self.optimal, **seg)

    def counts(self):
        """(ev [n_fusion, C, 3] {tp, n_ref, n_sys}, tag [n_fusion + 1, C, 3] {tp, fp, fn}) as numpy int64: ONE device->host copy"""
        return tuple(self._read()[:2])

    def segment_counts(self):
        """(seg [n_fusion, C, 3] {tp, n_ref, n_sys}, sdi [n_fusion, 3] {S, D, I}) as numpy int64, None without time_resolution"""
        if self.seg is None:
            return None
        return tuple(self._read()[2:])

    def compute(self):
        """{at_m: {'f1', 'precision', 'recall', 'class_wise', 'clip': {...}[, 'segment': {...}]}, 'at': {...}}: event-based macro
        scores per fusion strategy (what engine.evaluate returns as metrics[at_m] is ['f1']), the clip-level scores of its decoded
        events, the segment-based scores (with time_resolution) and the clip-level scores of the audio-tag head (when tags were
        counted); one device->host copy"""
        got = self._read()
        seg = {} if self.seg is None else dict(seg=got[2], sdi=got[3])
        return finalize(got[0], got[1], self.labels, self.fusion, self.at_counted, **seg)

    def summary(self, res=None):
        """the reference's "All Metrics" row per fusion strategy (see ``summary``) of ``res`` or of compute()"""
        return summary(self.compute() if res is None else res)


def _class_scores(t, present, labels):
    """class-wise {f1, precision, recall, tp, n_ref, n_sys} of counts t [C, 3] {tp, n_ref, n_sys} over the classes ``present``"""
    cw = {}
    for c in np.nonzero(present)[0]:
        tp, nr, ns = (int(v) for v in t[c])
        cw[labels[c]] = {'f1': _ratio(2 * tp, nr + ns), 'precision': _ratio(tp, ns), 'recall': _ratio(tp, nr),
                         'tp': tp, 'n_ref': nr, 'n_sys': ns}
    return cw


def _tag_scores(t, labels):
    cw = {}
    for c in np.nonzero(t.sum(1) > 0)[0]:                 # classes in the references or the estimates
        tp, fp, fn = (int(v) for v in t[c])
        cw[labels[c]] = {'f1': _ratio(2 * tp, 2 * tp + fp + fn), 'precision': _ratio(tp, tp + fp), 'recall': _ratio(tp, tp + fn),
                         'tp': tp, 'fp': fp, 'fn': fn}
    return _macro(cw)


def _macro(cw):
    out = {k: float(np.mean([v[k] for v in cw.values()])) if cw else 0.0 for k in ('f1', 'precision', 'recall')}
    out['class_wise'] = cw
    return out


def _segment_scores(seg, sdi, present, labels):
    """SegmentBasedMetrics' class-wise average (the 'f1' / 'precision' / 'recall' the reference reports as Sb_F / Sb_P / Sb_R) and
    overall scores of one fusion strategy's counters"""
    out = _macro(_class_scores(seg, present, labels))
    ntp, nref, nsys = (int(v) for v in seg.sum(0))
    s, d, i = (int(v) for v in sdi)
    out['overall'] = {'f1': _ratio(2 * ntp, nref + nsys), 'precision': _ratio(ntp, nsys), 'recall': _ratio(ntp, nref),
                      'error_rate': _ratio(s + d + i, nref), 'substitution_rate': _ratio(s, nref), 'deletion_rate': _ratio(d, nref),
                      'insertion_rate': _ratio(i, nref), 'Ntp': ntp, 'Nref': nref, 'Nsys': nsys, 'S': s, 'D': d, 'I': i}
    return out


def finalize(ev, tag, labels, fusion, at_counted=True, seg=None, sdi=None):
    """the host side of EventMetrics.compute on counter arrays (see there); ``seg`` [n_fusion, C, 3] / ``sdi`` [n_fusion, 3] add the
    segment-based scores as [at_m]['segment']"""
    res = {}
    for i, m in enumerate(fusion):
        present = (ev[i, :, 1] > 0) | (tag[i, :, 0] + tag[i, :, 1] > 0)     # in a reference, or decoded in any clip
        res[m] = _macro(_class_scores(ev[i], present, labels))
        res[m]['clip'] = _tag_scores(tag[i], labels)
        if seg is not None:
            res[m]['segment'] = _segment_scores(seg[i], sdi[i], present, labels)
    if at_counted:
        res['at'] = _tag_scores(tag[len(fusion)], labels)
    return res


def summary(res):
    """the reference's "All Metrics" row (compute_metrics, metrics.py:350-363) per fusion strategy of a compute() / finalize()
    result with segment-based scores: {at_m: {'Eb_F1', 'Eb_P', 'Eb_R', 'Sb_F', 'Sb_P', 'Sb_R', 'At_F1'}} as fractions (the
    reference prints them as percentages); At_F1 is the clip-level macro F1 of the decoded events, res[at_m]['clip']['f1']"""
    out = {}
    for m, r in res.items():
        if m == 'at':
            continue
        if 'segment' not in r:
            raise ValueError('summary: no segment-based scores (EventMetrics(..., time_resolution=1.0))')
        s = r['segment']
        out[m] = dict(zip(SUMMARY_COLUMNS, (r['f1'], r['precision'], r['recall'], s['f1'], s['precision'], s['recall'],
                                            r['clip']['f1'])))
    return out
