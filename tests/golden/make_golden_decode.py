#!/usr/bin/env python3
"""Generate tests/golden/g18_decode_strong.npz by running the REFERENCE's BoxEncoder.decode_strong (utilities/BoxEncoder.py:179-226).

The function body uses numpy only, but its module imports dcase_util, which is not installed where the fixtures are made: a stub
module with the two names the import line asks for (DecisionEncoder, ProbabilityEncoder) is placed in ``sys.modules`` first, the way
make_golden.py shims torchvision.  Nothing of the stub is executed by decode_strong.

Inputs are drawn from a seed (below) as PostProcess outputs of the URBAN-SED shape (Q = 10, C = 10 and Q = 20): scores on a grid
that hits the 0.5 threshold exactly, lengths around the 0.2 s minimum and runs of overlapping same-class events.  Each clip's
(scores, labels, boxes) is passed as CPU torch tensors, as engine.get_sedt_predictions passes them (engine.py:283-286).  Clips where two
kept events of one class share an onset are redrawn: the reference's default np.argsort leaves their order unspecified.

usage:  python tests/golden/make_golden_decode.py --reference <reference checkout>
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N_CLIPS, C = 18, 400, 10


def draw_clip(rng, Q):
    scores = rng.choice(np.array([0.3, 0.45, 0.5, 0.5, 0.55, 0.7, 0.9], dtype=np.float32), Q)
    scores = np.where(rng.random(Q) < 0.5, scores, rng.uniform(0.3, 1.0, Q).astype(np.float32)).astype(np.float32)
    labels = rng.integers(0, 4 if rng.random() < 0.5 else C, Q)      # few classes: long same-class chains
    on = np.round(rng.uniform(-0.5, 9.5, Q) / 0.05) * 0.05
    length = rng.choice([0.15, 0.2, 0.2, 0.25, 0.5, 1.0, 2.5], Q) + np.where(rng.random(Q) < 0.5, 0.0, rng.uniform(0, 1, Q))
    boxes = np.stack([on, on + length], -1).astype(np.float32)
    return scores, labels.astype(np.int64), boxes


def onset_ties(scores, labels, boxes):
    keep = (scores >= np.float32(0.5)) & ((boxes[:, 1] - boxes[:, 0]) >= np.float32(0.2))
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
    enc = BoxEncoder([f'class_{c}' for c in range(C)], 10)
    rng = np.random.default_rng(SEED)
    out = {}
    for Q in (10, 20):
        S, L, X = [], [], []
        while len(S) < N_CLIPS // 2:
            s, l, x = draw_clip(rng, Q)
            if not onset_ties(s, l, x):
                S.append(s), L.append(l), X.append(x)
        out[f'q{Q}_scores'], out[f'q{Q}_labels'], out[f'q{Q}_boxes'] = np.stack(S), np.stack(L), np.stack(X)
        for d in (1, 0):
            rows = []
            for b in range(len(S)):
                res = {'scores': torch.from_numpy(S[b]), 'labels': torch.from_numpy(L[b]), 'boxes': torch.from_numpy(X[b])}
                for lab, on, off, sc in enc.decode_strong(res, threshold=0.5, del_overlap=bool(d)):
                    rows.append((b, int(lab.split('_')[1]), float(on), float(off), float(sc)))
            out[f'q{Q}_del{d}'] = np.array(rows, dtype=np.float64).reshape(-1, 5)      # clip, class, onset, offset, score in output order
    np.savez_compressed(os.path.join(HERE, 'g18_decode_strong.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
