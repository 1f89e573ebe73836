"""TEST INFRASTRUCTURE, not product code: the counts of utilities/operating_points.SweepEventMetrics (csrc/sweep.hip) and the class-wise
decode (csrc/decode.hip: sedt_decode_events_classwise) restated on HOST numbers from tests/event_metrics_ref.py.

  * ``counts``: per operating point the event-based {tp, n_ref, n_sys} and clip-level {tp, fp, fn} counts of the rows
    utilities.predictions.unpack gives for a packed record buffer - the estimates of a clip are its rows in record order, compared as
    Python floats (the float32 times widened), against the clip's reference events; a clip outside the table counts at clip level only.
  * ``decode_strong``: BoxEncoder.decode_strong with one threshold per class: the queries that fail score >= tau[label] (> without
    del_overlap) or whose label is no class are dropped, event_metrics_ref.decode_strong decodes the rest with a threshold nothing
    fails, and the query indices are mapped back."""
import numpy as np

import event_metrics_ref as ER


def clip_reference(reference, k):
    """the reference events of clip index k, None for a clip outside the table (-1, past its end, or given as None)"""
    k = int(k)
    return reference[k] if 0 <= k < len(reference) else None


def counts(events, clip_idx, reference, n_classes, t_collar=0.2, pct=0.2, optimal=True):
    """events: predictions.unpack's list (per threshold {'clip' (position in the batch), 'cls', 'onset', 'offset', ...}); clip_idx [B]:
    the batch's clips in ``reference`` (per clip [(class index, onset, offset)] or None) -> (ev, tag) int64 [K, C, 3]"""
    K, C = len(events), n_classes
    ev, tag = np.zeros((K, C, 3), np.int64), np.zeros((K, C, 3), np.int64)
    for k, e in enumerate(events):
        for b, ci in enumerate(clip_idx):
            sel = np.nonzero(np.asarray(e['clip']) == b)[0]
            ests = [(int(e['cls'][i]), float(e['onset'][i]), float(e['offset'][i])) for i in sel]
            ests = [x for x in ests if 0 <= x[0] < C]
            refs = clip_reference(reference, ci)
            if refs is not None:
                ev[k] += ER.clip_event_counts(refs, ests, C, t_collar, pct, optimal)
            tag[k] += ER.clip_tag_counts({r[0] for r in (refs or [])}, {x[0] for x in ests}, C)
    return ev, tag


def decode_strong(scores, labels, boxes, tau, min_duration=0.2, del_overlap=True, max_len=None):
    """one clip, one operating point: tau [C] -> [(class, onset, offset, score, query)] in the reference's output order"""
    scores, boxes = np.asarray(scores, dtype=np.float32), np.asarray(boxes, dtype=np.float32)
    labels, tau = np.asarray(labels).astype(np.int64), np.asarray(tau, dtype=np.float32)
    keep = [q for q in range(len(scores)) if 0 <= labels[q] < len(tau)
            and (scores[q] >= tau[labels[q]] if del_overlap else scores[q] > tau[labels[q]])]
    out = ER.decode_strong(scores[keep], labels[keep], boxes[keep], threshold=-np.inf, min_duration=min_duration, del_overlap=del_overlap)
    res, used = [], set()
    for c, on, off, s in out:                                # the kept query this event is: same class, times and score, not yet used
        q = next(q for q in keep if q not in used and labels[q] == c and float(boxes[q][0]) == on and float(boxes[q][1]) == off
                 and float(scores[q]) == s)
        used.add(q)
        if max_len is not None:
            on, off = min(max(on, 0.0), float(max_len)), min(max(off, 0.0), float(max_len))
        res.append((c, on, off, s, q))
    return res


def f1_table(ev):
    """ev [K, C, 3] -> class F1 [K, C] as Python float divisions (0 on a zero denominator)"""
    return np.array([[2.0 * tp / (nr + ns) if nr + ns else 0.0 for tp, nr, ns in row] for row in np.asarray(ev).tolist()])
