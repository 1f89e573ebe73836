"""TEST INFRASTRUCTURE, not product code: the validation scores of the reference restated on HOST numbers.

The product decodes and counts in one HIP launch per fusion strategy (csrc/metrics.hip, sedt_event_metrics_update) and finalizes the
int64 counters on the host (utilities/metrics.py).  This module restates, in plain Python / numpy and independently of that code:

  * BoxEncoder.decode_strong (reference utilities/BoxEncoder.py:179-226) on one clip's PostProcess outputs, with the clip of
    onsets / offsets to [0, max_len_seconds] that engine.get_sedt_predictions applies afterwards (engine.py:287);
  * sed_eval's EventBasedMetrics as the reference calls it (utilities/metrics.py:43-80, 147-157: t_collar 0.2, percentage_of_length
    0.2, onset and offset evaluated, class-wise averages), with an exact maximum-cardinality bipartite matcher (depth-first
    augmenting paths) for sed_eval's default event_matching_type='optimal' and sed_eval's greedy pass behind a flag;
  * audio_tagging_results (metrics.py:281-322): per clip and class "present among the estimates" vs "present among the references",
    over the outer merge of the two file lists.

sed_eval, psds_eval and dcase_util are not installed where this suite runs, so the sed_eval part is RESTATED FROM ITS PUBLISHED
DEFINITION, NOT PINNED BY THE PACKAGE: a hit is an estimate of the reference's class with |on_r - on_e| <= t_collar and
|off_r - off_e| <= max(t_collar, percentage_of_length * (off_r - on_r)), compared on Python floats (float64); the class-wise
correct count is the size of a maximum matching of hits ('optimal', the documented default the reference does not override); the
class-wise F is 2 tp / (n_ref + n_sys) (sed_eval divides by denominators guarded with machine epsilon, which moves the value by a few
ulps and not at all when the denominator is 0).  decode_strong itself is pinned by tests/golden/g18_decode_strong.npz, made from the
reference's own function (tests/golden/make_golden_decode.py).

Numerics follow the reference's scalar types: the decode compares float32 values (torch / numpy float32 scalars against the Python
threshold, which torch rounds to float32), the matching compares float64.  Ties in onset between two kept events of one class are
ordered by query index here; the reference's np.argsort default (quicksort) leaves that order unspecified."""
import math

import numpy as np


def decode_strong(scores, labels, boxes, threshold=0.5, min_duration=0.2, del_overlap=True, max_len=None):
    """one clip: scores [Q], labels [Q], boxes [Q, 2] (seconds) -> [(class, onset, offset, score)] in the reference's output order
    (with del_overlap: classes in order of their first kept query, each class by onset); onsets / offsets as float64, clipped to
    [0, max_len] when max_len is given"""
    scores = np.asarray(scores, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    thr, mind = np.float32(threshold), np.float32(min_duration)
    out = []
    if not del_overlap:
        for i in range(len(scores)):
            on, off = boxes[i]
            if scores[i] > thr and np.float32(off - on) >= mind:
                out.append((int(labels[i]), on, off, scores[i]))
    else:
        groups = {}
        for i in range(len(scores)):
            on, off = boxes[i]
            if scores[i] >= thr and np.float32(off - on) >= mind:
                groups.setdefault(int(labels[i]), []).append((scores[i], on, off, i))
        for c, ev in groups.items():
            ev.sort(key=lambda e: (e[1], e[3]))             # onset, then query index
            i = 1
            while i < len(ev):                              # BoxEncoder.py:214-223, the same in-place deletions
                if ev[i][1] < ev[i - 1][2]:
                    if ev[i][0] > ev[i - 1][0]:
                        del ev[i - 1]
                    else:
                        del ev[i]
                    continue
                i += 1
            out += [(c, e[1], e[2], e[0]) for e in ev]
    res = []
    for c, on, off, s in out:
        on, off = float(on), float(off)
        if max_len is not None:
            on, off = min(max(on, 0.0), float(max_len)), min(max(off, 0.0), float(max_len))
        res.append((c, on, off, float(s)))
    return res


def hit(ref, est, t_collar=0.2, pct=0.2):
    """sed_eval validate_onset and validate_offset on (class, onset, offset, ...) tuples"""
    if ref[0] != est[0]:
        return False
    if not math.fabs(ref[1] - est[1]) <= t_collar:
        return False
    return math.fabs(ref[2] - est[2]) <= max(t_collar, pct * (ref[2] - ref[1]))


def max_matching(adj, n_est):
    """size of a maximum matching; adj[j] = estimates hit by reference j (Kuhn's depth-first augmenting paths)"""
    match = [-1] * n_est

    def augment(j, seen):
        for i in adj[j]:
            if not seen[i]:
                seen[i] = True
                if match[i] < 0 or augment(match[i], seen):
                    match[i] = j
                    return True
        return False
    return sum(augment(j, [False] * n_est) for j in range(len(adj)))


def greedy_matching(adj, n_est):
    """sed_eval's event_matching_type='greedy': references in order, each takes the first estimate (in order) not yet taken"""
    taken = [False] * n_est
    for row in adj:
        for i in sorted(row):
            if not taken[i]:
                taken[i] = True
                break
    return sum(taken)


def clip_event_counts(refs, ests, n_classes, t_collar=0.2, pct=0.2, optimal=True):
    """one clip: refs / ests lists of (class, onset, offset, ...) -> int64 [C, 3] of {tp, n_ref, n_sys}"""
    out = np.zeros((n_classes, 3), dtype=np.int64)
    for c in range(n_classes):
        r = [e for e in refs if e[0] == c]
        s = [e for e in ests if e[0] == c]
        adj = [[i for i, e in enumerate(s) if hit(x, e, t_collar, pct)] for x in r]
        out[c] = ((max_matching if optimal else greedy_matching)(adj, len(s)), len(r), len(s))
    return out


def clip_tag_counts(ref_classes, est_classes, n_classes):
    """one clip: sets of classes present -> int64 [C, 3] of {tp, fp, fn}"""
    out = np.zeros((n_classes, 3), dtype=np.int64)
    for c in range(n_classes):
        r, s = c in ref_classes, c in est_classes
        out[c] = (r and s, s and not r, r and not s)
    return out


class HostEventMetrics(object):
    """the counters of utilities/metrics.EventMetrics, accumulated clip by clip from the restatement above.
    reference: list over clips of [(class, onset, offset)] or None (no row in the reference: the clip is not evaluated)"""

    def __init__(self, n_classes, reference, max_len, n_fusion=1, threshold=0.5, min_duration=0.2, del_overlap=True, t_collar=0.2,
                 pct=0.2, optimal=True):
        self.C, self.ref, self.max_len = n_classes, reference, max_len
        self.kw = dict(threshold=threshold, min_duration=min_duration, del_overlap=del_overlap)
        self.t_collar, self.pct, self.optimal = t_collar, pct, optimal
        self.ev = np.zeros((n_fusion, n_classes, 3), dtype=np.int64)
        self.tag = np.zeros((n_fusion + 1, n_classes, 3), dtype=np.int64)

    def update(self, fusion, scores, labels, boxes, clip_idx, at_tags=None):
        """one fusion strategy's [B, Q] / [B, Q, 2] host arrays; at_tags [B, C] 0/1 or None"""
        for b, k in enumerate(clip_idx):
            k = int(k)
            refs = self.ref[k] if k >= 0 else None
            ests = decode_strong(scores[b], labels[b], boxes[b], max_len=self.max_len, **self.kw)
            if refs is not None:
                self.ev[fusion] += clip_event_counts(refs, ests, self.C, self.t_collar, self.pct, self.optimal)
            rc = {e[0] for e in (refs or [])}
            self.tag[fusion] += clip_tag_counts(rc, {e[0] for e in ests}, self.C)
            if at_tags is not None:
                self.tag[-1] += clip_tag_counts(rc, {c for c in range(self.C) if at_tags[b][c]}, self.C)


def macro_scores(reference, estimated, n_classes, t_collar=0.2, pct=0.2, optimal=True):
    """the reference's event_based_evaluation_df + results_class_wise_average_metrics and audio_tagging_results, straight from the
    event lists (no counters): reference {file: [(class, on, off)]} (files with no event: empty list), estimated {file: [(class,
    on, off, ...)]} over any files.  Returns (event macro f, event macro p, event macro r, clip macro f)."""
    classes = {e[0] for v in reference.values() for e in v} | {e[0] for v in estimated.values() for e in v}
    tot = np.zeros((n_classes, 3), dtype=np.int64)
    for f, refs in reference.items():                     # evaluated files: those of the reference (metrics.py:58)
        tot += clip_event_counts(refs, estimated.get(f, []), n_classes, t_collar, pct, optimal)
    fs, ps, rs = [], [], []
    for c in sorted(classes):
        tp, nr, ns = (int(v) for v in tot[c])
        fs.append(2 * tp / (nr + ns) if nr + ns else 0.0)
        ps.append(tp / ns if ns else 0.0)
        rs.append(tp / nr if nr else 0.0)
    tags = np.zeros((n_classes, 3), dtype=np.int64)
    for f in set(reference) | {f for f, v in estimated.items() if v}:        # outer merge of the weak tables
        tags += clip_tag_counts({e[0] for e in reference.get(f, [])}, {e[0] for e in estimated.get(f, [])}, n_classes)
    cf = []
    for c in sorted(classes):
        tp, fp, fn = (int(v) for v in tags[c])
        cf.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
    mean = (lambda v: float(np.mean(v)) if v else 0.0)
    return mean(fs), mean(ps), mean(rs), mean(cf)
