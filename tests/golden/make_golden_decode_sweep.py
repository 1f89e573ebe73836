#!/usr/bin/env python3
"""Generate tests/golden/g23_decode_sweep.npz by running the REFERENCE's BoxEncoder.decode_strong (utilities/BoxEncoder.py:179-226) at
a grid of thresholds - the operating points of a threshold sweep - and at the edges of the decode kernel's envelope.

The module is imported the way make_golden_decode.py imports it (a stub dcase_util in ``sys.modules``; decode_strong executes none of
it).  Shapes (Q, C): (1, 1) and (21, 10) with 60 clips each, (64, 63) with 16 (every row repeats three float32 values per operating
point, and the file must stay no larger than g18_decode_strong.npz: 16 clips of 64 queries are what fits), both del_overlap values, thresholds THRESHOLDS passed as the
Python floats a caller writes.  Half of the scores are drawn from {float32(t), the float32 just above, the float32 just below} over
those thresholds, the rest uniform: the rounding of the threshold to float32 (float32(0.7) >= 0.7 holds in torch, not in float64) and
the >= (del_overlap) / > (no del_overlap) distinction decide rows.  Lengths lie around the 0.2 s minimum; labels come half the time
from 4 classes only (long same-class chains).  For Q <= 21 onsets lie on the 0.05 s grid and a clip where two events of one class kept
at the lowest threshold share an onset is redrawn (the reference's np.argsort leaves their order open); for Q = 64 onsets are
continuous uniform float32, so no ties arise and nothing is redrawn.

Arrays only: per shape ``q{Q}c{C}_scores`` f32 [N, Q], ``_labels`` int16 [N, Q], ``_boxes`` f32 [N, Q, 2], and per (del_overlap d,
threshold index i) ``q{Q}c{C}_del{d}_t{i}`` f32 [rows, 5] = (clip, class, onset, offset, score) in the reference's output order,
unclipped (every value is a float32 or a small integer: the generator asserts the float32 storage loses nothing); ``thresholds`` f64.

usage:  python tests/golden/make_golden_decode_sweep.py --reference <reference checkout>
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 23
SHAPES = ((1, 1, 60), (21, 10, 60), (64, 63, 16))       # (Q, C, clips)
THRESHOLDS = (0.1, 0.3, 0.5, 0.7, 0.9)


def draw_clip(rng, Q, C):
    t32 = np.array(THRESHOLDS, dtype=np.float32)
    edge = np.concatenate([t32, np.nextafter(t32, np.float32(2)), np.nextafter(t32, np.float32(-1))])
    scores = np.where(rng.random(Q) < 0.5, rng.choice(edge, Q), rng.uniform(0.0, 1.0, Q).astype(np.float32)).astype(np.float32)
    labels = rng.integers(0, min(C, 4) if rng.random() < 0.5 else C, Q)
    if Q <= 21:
        on = (np.round(rng.uniform(-0.5, 9.5, Q) / 0.05) * 0.05).astype(np.float32)
    else:
        on = rng.uniform(-0.5, 9.5, Q).astype(np.float32)
    length = rng.choice([0.1, 0.15, 0.2, 0.2, 0.25, 0.5, 1.0, 2.5], Q) + np.where(rng.random(Q) < 0.6, 0.0, rng.uniform(-0.05, 0.3, Q))
    boxes = np.stack([on, (on.astype(np.float64) + length).astype(np.float32)], -1)
    return scores, labels.astype(np.int64), boxes


def onset_ties(scores, labels, boxes):
    """two events of one class, kept at the lowest threshold (a superset of what any higher one keeps), on one onset"""
    keep = (scores >= np.float32(min(THRESHOLDS))) & ((boxes[:, 1] - boxes[:, 0]) >= np.float32(0.2))
    seen = set()
    for i in np.nonzero(keep)[0]:
        k = (int(labels[i]), float(boxes[i, 0]))
        if k in seen:
            return True
        seen.add(k)
    return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference repository')
    ref = ap.parse_args().reference
    dcase_util = types.ModuleType('dcase_util')
    data = types.ModuleType('dcase_util.data')
    data.DecisionEncoder = data.ProbabilityEncoder = object
    dcase_util.data = data
    sys.modules.update({'dcase_util': dcase_util, 'dcase_util.data': data})
    sys.path.insert(0, ref)
    from utilities.BoxEncoder import BoxEncoder
    rng = np.random.default_rng(SEED)
    out = {'thresholds': np.array(THRESHOLDS, dtype=np.float64)}
    for Q, C, N_CLIPS in SHAPES:
        enc = BoxEncoder([f'class_{c}' for c in range(C)], 10)
        S, L, X, drawn = [], [], [], 0
        while len(S) < N_CLIPS:
            s, l, x = draw_clip(rng, Q, C)
            drawn += 1
            if Q <= 21 and onset_ties(s, l, x):
                continue
            S.append(s), L.append(l), X.append(x)
        share = (drawn - N_CLIPS) / drawn
        print(f'Q {Q} C {C}: {drawn} clips drawn, {share:.1%} redrawn for an onset tie')
        assert share < 0.2, share
        if Q > 21:
            assert drawn == N_CLIPS and not any(onset_ties(s, l, x) for s, l, x in zip(S, L, X))
        key = f'q{Q}c{C}'
        out[f'{key}_scores'], out[f'{key}_labels'], out[f'{key}_boxes'] = np.stack(S), np.stack(L).astype(np.int16), np.stack(X)
        for d in (1, 0):
            for i, t in enumerate(THRESHOLDS):
                rows = []
                for b in range(N_CLIPS):
                    res = {'scores': torch.from_numpy(S[b]), 'labels': torch.from_numpy(L[b]), 'boxes': torch.from_numpy(X[b])}
                    for lab, on, off, sc in enc.decode_strong(res, threshold=t, del_overlap=bool(d)):
                        rows.append((b, int(lab.split('_')[1]), float(on), float(off), float(sc)))
                rows = np.array(rows, dtype=np.float64).reshape(-1, 5)
                assert np.array_equal(rows.astype(np.float32).astype(np.float64), rows)
                out[f'{key}_del{d}_t{i}'] = rows.astype(np.float32)
    path = os.path.join(HERE, 'g23_decode_sweep.npz')
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()})
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
