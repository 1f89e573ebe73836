"""TEST INFRASTRUCTURE, not product code: the segment-based scores of the reference's final test restated on HOST numbers.

The product counts segments in the same HIP launch as the event-based scores (csrc/metrics.hip, sedt_event_segment_metrics_update) and
finalizes the int64 counters on the host (utilities/metrics.py).  This module restates, in plain Python / numpy and independently of
that code, sed_eval's SegmentBasedMetrics(time_resolution=r) as the reference's segment_based_evaluation_df feeds it (reference
utilities/metrics.py:83-116, 147-157, 350-363), on the decode of tests/event_metrics_ref.py (imported, not changed).

sed_eval is not installed where this suite runs, so this is RESTATED FROM ITS PUBLISHED CODE, NOT PINNED BY THE PACKAGE:
  * evaluated clips: the clips with a reference row (the loop over reference["filename"].unique()); a clip given as None or -1 adds
    nothing; a clip whose only row has no label is evaluated with an empty reference (sed_eval drops items without event_label), so
    its estimated segments count in n_sys and in I;
  * event roll at resolution r (event_list_to_event_roll): event (c, on, off) sets class c active in the segments
    floor(on * 1 / r) <= k < ceil(off * 1 / r), each quotient a float64 IEEE division, not a multiplication by 1 / r
    (0.3 / 0.1 = 2.9999999999999996, so the floor is 2, while 0.3 * (1 / 0.1) gives 3.0); an empty range sets nothing; overlapping
    events of one class OR together; the roll is ceil(max offset / r) long and the shorter of the two rolls is padded with zeros,
    which only adds true negatives (not reported);
  * estimates: the decoded survivors after the clip to [0, max_len]; an estimate clipped to zero length keeps its label in the class
    set and sets no segment when the clip point is a multiple of r (floor = ceil);
  * counts: class-wise over the clip's segments tp (active in both), n_ref, n_sys; per segment over the classes Ntp, Nref, Nsys and
    S += min(Nref, Nsys) - Ntp, D += max(0, Nref - Nsys), I += max(0, Nsys - Nref), so S + D = Nref - Ntp and S + I = Nsys - Ntp;
  * scores: class-wise F = 2 tp / (n_ref + n_sys), P = tp / n_sys, R = tp / n_ref, averaged over the classes of the reference and
    the estimate tables (results_class_wise_average_metrics, reported as Sb_F / Sb_P / Sb_R); overall P = Ntp / Nsys, R = Ntp / Nref,
    F = 2 Ntp / (Nref + Nsys), ER = (S + D + I) / Nref.  sed_eval guards these denominators with machine epsilon; here a zero
    denominator gives 0."""
import math

import numpy as np

import event_metrics_ref as R


def event_roll(events, n_classes, r):
    """sed_eval's event_list_to_event_roll on (class, onset, offset, ...) tuples: int64 [ceil(max offset / r), C] of 0 / 1"""
    n = int(math.ceil(max(e[2] for e in events) * 1 / r)) if events else 0
    roll = np.zeros((max(n, 0), n_classes), dtype=np.int64)
    for e in events:
        assert e[1] >= 0 and e[2] >= 0, 'a negative time would wrap around the roll (set_reference refuses it)'
        roll[int(math.floor(e[1] * 1 / r)):int(math.ceil(e[2] * 1 / r)), e[0]] = 1
    return roll


def clip_segment_counts(refs, ests, n_classes, r):
    """one evaluated clip: refs / ests lists of (class, onset, offset, ...) -> (int64 [C, 3] {tp, n_ref, n_sys}, int64 [3] {S, D, I})"""
    a, s = event_roll(refs, n_classes, r), event_roll(ests, n_classes, r)
    n = max(len(a), len(s))
    a = np.vstack([a, np.zeros((n - len(a), n_classes), np.int64)])
    s = np.vstack([s, np.zeros((n - len(s), n_classes), np.int64)])
    cw = np.stack([(a + s > 1).sum(0), a.sum(0), s.sum(0)], -1).astype(np.int64)
    ntp, nref, nsys = (a + s > 1).sum(1), a.sum(1), s.sum(1)          # per segment, over the classes
    sdi = np.array([(np.minimum(nref, nsys) - ntp).sum(), np.maximum(0, nref - nsys).sum(), np.maximum(0, nsys - nref).sum()],
                   dtype=np.int64)
    return cw, sdi


class HostSegmentMetrics(R.HostEventMetrics):
    """HostEventMetrics plus the segment counters of utilities/metrics.EventMetrics(time_resolution=r): seg [n_fusion, C, 3]
    {tp, n_ref, n_sys} and sdi [n_fusion, 3] {S, D, I}, from the clips that have a reference row"""

    def __init__(self, n_classes, reference, max_len, time_resolution, n_fusion=1, **kw):
        super().__init__(n_classes, reference, max_len, n_fusion=n_fusion, **kw)
        self.r = time_resolution
        self.seg = np.zeros((n_fusion, n_classes, 3), dtype=np.int64)
        self.sdi = np.zeros((n_fusion, 3), dtype=np.int64)

    def update(self, fusion, scores, labels, boxes, clip_idx, at_tags=None):
        super().update(fusion, scores, labels, boxes, clip_idx, at_tags=at_tags)
        for b, k in enumerate(clip_idx):
            k = int(k)
            refs = self.ref[k] if k >= 0 else None
            if refs is None:
                continue
            cw, sdi = clip_segment_counts(refs, R.decode_strong(scores[b], labels[b], boxes[b], max_len=self.max_len, **self.kw),
                                          self.C, self.r)
            self.seg[fusion] += cw
            self.sdi[fusion] += sdi


def segment_scores(reference, estimated, n_classes, r):
    """segment_based_evaluation_df + results_class_wise_average_metrics / results_overall_metrics straight from the event lists, with
    sets of active segments instead of rolls and counters: reference {file: [(class, on, off)]} (files with no event: empty list),
    estimated {file: [(class, on, off, ...)]} over any files.  Returns (macro f, macro p, macro r, overall dict)."""
    classes = {e[0] for v in reference.values() for e in v} | {e[0] for v in estimated.values() for e in v}
    tot = np.zeros((n_classes, 3), dtype=np.int64)
    S = D = I = 0
    for f, refs in reference.items():                     # evaluated files: those of the reference
        act = []
        for evs in (refs, estimated.get(f, [])):
            a = [set() for _ in range(n_classes)]
            for e in evs:
                a[e[0]].update(range(math.floor(e[1] / r), math.ceil(e[2] / r)))
            act.append(a)
        for c in range(n_classes):
            tot[c] += (len(act[0][c] & act[1][c]), len(act[0][c]), len(act[1][c]))
        for k in set().union(*act[0], *act[1]):
            nr = sum(k in x for x in act[0])
            ns = sum(k in x for x in act[1])
            nt = sum(k in x and k in y for x, y in zip(act[0], act[1]))
            S, D, I = S + min(nr, ns) - nt, D + max(0, nr - ns), I + max(0, ns - nr)
    fs, ps, rs = [], [], []
    for c in sorted(classes):
        tp, nr, ns = (int(v) for v in tot[c])
        fs.append(2 * tp / (nr + ns) if nr + ns else 0.0)
        ps.append(tp / ns if ns else 0.0)
        rs.append(tp / nr if nr else 0.0)
    ntp, nref, nsys = (int(v) for v in tot.sum(0))
    overall = {'f1': 2 * ntp / (nref + nsys) if nref + nsys else 0.0, 'precision': ntp / nsys if nsys else 0.0,
               'recall': ntp / nref if nref else 0.0, 'error_rate': (S + D + I) / nref if nref else 0.0, 'Ntp': ntp, 'Nref': nref,
               'Nsys': nsys, 'S': S, 'D': D, 'I': I}
    mean = (lambda v: float(np.mean(v)) if v else 0.0)
    return mean(fs), mean(ps), mean(rs), overall
