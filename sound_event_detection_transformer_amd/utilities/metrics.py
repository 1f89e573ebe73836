"""Validation scores on the device: event-based and clip-level macro F1 of the reference's engine.evaluate (engine.py:199-297,
utilities/metrics.py:43-80, 147-157, 281-322), without the host decode (BoxEncoder.decode_strong, pandas, sed_eval).

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
  * the audio-tag head (engine.py:203-206): the same clip-level counts with the thresholded ``at`` tags.

Macro averages run over the classes the reference's tables contain: those occurring in the references or in the estimates
(metrics.py:60-63, 283-287), not over all C classes.  F = 2 tp / (n_ref + n_sys) (event) or 2 tp / (2 tp + fp + fn) (clip), 0 when
the denominator is 0; precision and recall likewise 0 on a zero denominator (sed_eval guards its denominators with machine epsilon,
which moves a value by a few ulps; pandas gives NaN for the clip-level precision / recall of such a class)."""
import math

import numpy as np
import torch

from .. import ops

MAX_REF_EVENTS = 64        # reference events of one clip the kernel holds (csrc/metrics.hip: SEDT_EM_MAXR)


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


class EventMetrics(object):
    """engine.evaluate's scores accumulated on the device.  ``labels``: the class names in the model's class order (decoder.labels);
    ``fusion_strategy``: the PostProcess fusion modes the predict step runs, in its order (results are keyed by them)."""

    def __init__(self, labels, max_len_seconds, t_collar=0.2, percentage_of_length=0.2, threshold=0.5, min_duration=0.2,
                 del_overlap=True, fusion_strategy=(1,), optimal=True, device=None):
        self.labels = list(labels)
        self.index = {l: i for i, l in enumerate(self.labels)}
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
        self.table, self.n_clips, self.max_ref = None, 0, 0
        self.generation = 0          # bumped when set_reference changes what a launch captured: table pointers, clip / event counts
        self.at_counted = False

    # ------------------------------------------------------------------------------------------------------------------------
    def set_reference(self, events):
        """events: per clip (the index ``update`` receives) a list of (label, onset, offset) - label a class name or index, times in
        seconds - or None for a clip that has no row in the reference.  Uploads the table once; the counters are not touched."""
        off, cls, on, end, present = [0], [], [], [], []
        for k, ev in enumerate(events):
            present.append(ev is not None)
            for label, onset, offset in (ev or ()):
                c = self.index[label] if label in self.index else int(label)
                if not 0 <= c < self.C:
                    raise ValueError(f'set_reference: clip {k}: class {label!r} is not one of the {self.C} labels')
                if not (math.isfinite(onset) and math.isfinite(offset)):
                    raise ValueError(f'set_reference: clip {k}: non-finite event time')
                cls.append(c), on.append(float(onset)), end.append(float(offset))
            if len(cls) - off[-1] > MAX_REF_EVENTS:
                raise ValueError(f'set_reference: clip {k} has {len(cls) - off[-1]} reference events (at most {MAX_REF_EVENTS})')
            off.append(len(cls))
        n = len(off) - 1
        max_ref = int(np.diff(off).max()) if n else 0
        host = {'present': torch.tensor(present or [0], dtype=torch.int32), 'off': torch.tensor(off, dtype=torch.int32),
                'cls': torch.tensor(cls or [0], dtype=torch.int32), 'on': torch.tensor(on or [0.0], dtype=torch.float64), 'end': torch.tensor(end or [0.0], dtype=torch.float64)}
        t = self.table
        if t is not None and all(t[k].numel() >= host[k].numel() for k in host):
            for k in host:
                t[k][:host[k].numel()].copy_(host[k])
        else:
            self.table = {k: v.to(self.device) for k, v in host.items()}
            self.generation += 1
        if (n, max_ref) != (self.n_clips, self.max_ref):
            self.generation += 1
        self.n_clips, self.max_ref = n, max_ref
        return self

    def host_clip_index(self, idx):
        """the batch's clip indices as a host int32 tensor, checked against the table (-1 = a clip outside it, not evaluated)"""
        h = torch.as_tensor(np.asarray(idx, dtype=np.int64)).reshape(-1)
        bad = (h < -1) | (h >= self.n_clips)
        if bool(bad.any()):
            raise ValueError(f'EventMetrics: clip index {int(h[bad][0])} outside -1 .. {self.n_clips - 1}')
        return h.to(torch.int32)

    def clip_index(self, idx):
        """the batch's clip indices as a device int32 tensor (a device tensor is taken as it is: the kernel skips indices outside
        the table)"""
        if torch.is_tensor(idx) and idx.is_cuda:
            return idx.to(torch.int32).contiguous()
        return self.host_clip_index(idx).to(self.device)

    def reset(self):
        """zero the counters (start of a validation set); in place, so a captured graph keeps accumulating into them"""
        self.ev.zero_()
        self.tag.zero_()
        return self

    def update(self, results, audio_tags, clip_idx):
        """one batch: results {at_m: (scores [B,Q], labels [B,Q] int64, boxes [B,Q,2] seconds)} as predict_step returns them,
        audio_tags [B,C] (0/1, or None), clip_idx [B] (the clips' indices in the reference, -1 = no reference row).  One launch per
        fusion strategy; nothing is read back."""
        if self.table is None:
            raise RuntimeError('EventMetrics.update: set_reference() first')
        idx = self.clip_index(clip_idx)
        tags = None if audio_tags is None else audio_tags.to(torch.int64).contiguous()
        self.at_counted = self.at_counted or tags is not None
        for i, m in enumerate(self.fusion):
            scores, labels, boxes = results[m]
            ops.event_metrics_update(scores.contiguous(), labels.contiguous(), boxes.contiguous(), tags if i == 0 else None, idx,
                                     self.table, self.n_clips, self.max_ref, self.ev, self.tag, i, threshold=self.threshold,
                                     min_duration=self.min_duration, max_len=self.max_len, t_collar=self.t_collar, pct=self.pct,
                                     del_overlap=self.del_overlap, optimal=self.optimal)

    def counts(self):
        """(ev [n_fusion, C, 3] {tp, n_ref, n_sys}, tag [n_fusion + 1, C, 3] {tp, fp, fn}) as numpy int64: ONE device->host copy"""
        h = torch.cat([self.ev.reshape(-1), self.tag.reshape(-1)]).cpu().numpy()
        n = self.ev.numel()
        return h[:n].reshape(self.ev.shape), h[n:].reshape(self.tag.shape)

    def compute(self):
        """{at_m: {'f1', 'precision', 'recall', 'class_wise', 'clip': {...}}, 'at': {...}}: event-based macro scores per fusion
        strategy (what engine.evaluate returns as metrics[at_m] is ['f1']), the clip-level scores of its decoded events, and the
        clip-level scores of the audio-tag head (when tags were counted)"""
        ev, tag = self.counts()
        return finalize(ev, tag, self.labels, self.fusion, self.at_counted)


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


def finalize(ev, tag, labels, fusion, at_counted=True):
    """the host side of EventMetrics.compute on counter arrays (see there)"""
    res = {}
    for i, m in enumerate(fusion):
        cw = {}
        present = (ev[i, :, 1] > 0) | (tag[i, :, 0] + tag[i, :, 1] > 0)     # in a reference, or decoded in any clip
        for c in np.nonzero(present)[0]:
            tp, nr, ns = (int(v) for v in ev[i, c])
            cw[labels[c]] = {'f1': _ratio(2 * tp, nr + ns), 'precision': _ratio(tp, ns), 'recall': _ratio(tp, nr),
                             'tp': tp, 'n_ref': nr, 'n_sys': ns}
        res[m] = _macro(cw)
        res[m]['clip'] = _tag_scores(tag[i], labels)
    if at_counted:
        res['at'] = _tag_scores(tag[len(fusion)], labels)
    return res
