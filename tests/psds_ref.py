"""TEST INFRASTRUCTURE, not product code: the polyphonic sound detection score (Bilen et al., ICASSP 2020; psds_eval's PSDSEval)
restated on HOST numbers, in plain Python loops over prediction rows and reference rows.

The product counts in one HIP launch per fusion strategy on the packed event records (csrc/psds.hip) and finishes with numpy
(utilities/psds.py: psds_from_counts).  This module restates both halves independently of that code - it never reads a packed record
and imports nothing from the package - from the definition the product's module docstring writes down.  psds_eval is not installed
where this suite runs, so like the sed_eval part of tests/event_metrics_ref.py THIS IS A RESTATEMENT FROM THE PUBLISHED DEFINITION,
NOT PINNED BY THE PACKAGE.

  counts(...)     per operating point the confusion counts [C][C + 1]: DTC, GTC, CTTC and the world column, Python floats (float64)
  constants(...)  n_c, T_c and T of a reference
  score(...)      the PSD score of counts: every class curve f_c(x) = the largest tpr among the operating points whose efpr is <= x
                  (0 when there is none) - the sorted, de-duplicated, running-maximum step function of the definition - evaluated at
                  every breakpoint of every class"""
import math


def _overlap_sum(on, off, dur, refs):
    """sum over refs [(onset, offset)] in order of inter / dur, inter = min(off, off_g) - max(on, on_g) where > 0"""
    total = 0.0
    for g_on, g_off in refs:
        inter = min(off, g_off) - max(on, g_on)
        if inter > 0:
            total = total + inter / dur
    return total


def counts(tables_per_threshold, reference, durations, labels, dtc=0.5, gtc=0.5, cttc=0.3):
    """tables_per_threshold: per operating point the prediction rows [(clip index, class index, onset, offset)] in output order;
    reference: per clip [(class index or label, onset, offset)] or None (a clip outside the reference: skipped); durations: per clip
    seconds; labels: the class names.  Returns [K][C][C + 1] nested lists of ints."""
    C = len(labels)
    index = {l: i for i, l in enumerate(labels)}
    out = []
    for rows in tables_per_threshold:
        cnt = [[0] * (C + 1) for _ in range(C)]
        per_clip = {}
        for clip, c, on, off in rows:
            per_clip.setdefault(int(clip), []).append((int(c), float(on), float(off)))
        for clip, dets in per_clip.items():
            if clip < 0 or clip >= len(reference) or reference[clip] is None:
                continue
            refs = [(index[l] if l in index else int(l), float(on), float(off)) for l, on, off in reference[clip]]
            refs = [(c, on, off) for c, on, off in refs if off - on > 0]                  # a zero-length event takes part in nothing
            of_class = {}                                                                 # class -> its [(onset, offset)] in table order
            for g, g_on, g_off in refs:
                of_class.setdefault(g, []).append((g_on, g_off))
            dets = [(c, on, off) for c, on, off in dets if 0 <= c < C and off - on > 0]
            passed = []
            for c, on, off in dets:
                dur = off - on
                p = _overlap_sum(on, off, dur, of_class.get(c, []))
                if p >= dtc:
                    passed.append((c, on, off))
                    continue
                for other in range(C):
                    if other == c:
                        continue
                    if _overlap_sum(on, off, dur, of_class.get(other, [])) >= cttc:
                        cnt[c][other] += 1
                if (min(off, durations[clip]) - max(on, 0.0)) / dur >= cttc:
                    cnt[c][C] += 1
            for g, g_on, g_off in refs:
                g_dur = g_off - g_on
                v = 0.0
                for c, on, off in passed:
                    if c != g:
                        continue
                    inter = min(off, g_off) - max(on, g_on)
                    if inter > 0:
                        v = v + inter / g_dur
                if v >= gtc:
                    cnt[g][g] += 1
        out.append(cnt)
    return out


def constants(reference, durations, labels):
    """(n_c [C], T_c [C], T): the number and the summed duration of every class's reference events (zero-length ones left out) and the
    summed duration of the clips present in the reference"""
    C = len(labels)
    index = {l: i for i, l in enumerate(labels)}
    n, t, total = [0] * C, [0.0] * C, 0.0
    for clip, ev in enumerate(reference):
        if ev is None:
            continue
        total += float(durations[clip])
        for l, on, off in ev:
            c = index[l] if l in index else int(l)
            if float(off) - float(on) > 0:
                n[c] += 1
                t[c] += float(off) - float(on)
    return n, t, total


def score(cnt, n_gt, gt_dur, total_dur, alpha_ct=0, alpha_st=0, max_efpr=100):
    """the PSD score of cnt [K][C][C + 1] (see the module docstring)"""
    K, C = len(cnt), len(n_gt)
    classes = [c for c in range(C) if n_gt[c] > 0]
    assert classes and max_efpr > 0 and total_dur > 0
    points = {}                                            # class -> [(efpr, tpr)] over the operating points
    for c in classes:
        pts = []
        for k in range(K):
            tpr = cnt[k][c][c] / n_gt[c]
            fpr = cnt[k][c][C] / total_dur * 3600.0
            cross = [cnt[k][c][o] / gt_dur[o] * 3600.0 for o in classes if o != c]
            efpr = fpr + alpha_ct * (sum(cross) / len(cross) if cross else 0.0)
            pts.append((efpr, tpr))
        points[c] = pts
    breaks = sorted({x for pts in points.values() for x, _ in pts})

    def etpr(x):
        f = [max([y for px, y in points[c] if px <= x], default=0.0) for c in classes]
        mean = sum(f) / len(f)
        std = math.sqrt(sum((v - mean) ** 2 for v in f) / len(f))
        return max(0.0, mean - alpha_st * std)

    area = 0.0
    for i, x in enumerate(breaks):
        if x > max_efpr:
            break
        right = breaks[i + 1] if i + 1 < len(breaks) and breaks[i + 1] <= max_efpr else max_efpr
        area += etpr(x) * (right - x)
    return area / max_efpr
