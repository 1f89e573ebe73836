#!/usr/bin/env python3
"""Generate tests/golden/g25_collapse.npz by running the REFERENCE's own ``data_utils.collapse_event.collapse`` - the function that merged
the overlapping annotations of one class when URBAN-SED's metadata was made - over designed event sets, one "file" each:

  0 nested      an event inside another of its class
  1 chained     a overlaps b, b overlaps c, a does not reach c: one event
  2 touching    end == onset of the next: merged (the reference compares with <=)
  3 disjoint    a gap of one sample: kept apart
  4 interleaved three classes whose events alternate in time; every class merges on its own
  5 single      one event
  6 empty       no event: the file has no row in the frame and none in the result

All times lie on the 16 kHz sample grid (k / 16000 in float64); collapse only compares and takes maxima, so the merged times are input
times and go back to the grid exactly.  The reference appends frames with DataFrame.append, which pandas 2 removed: it is supplied here
through pd.concat for the run.  Stored: data only - per event the file, class, onset and end in samples, before and after.

usage:  python tests/golden/make_golden_collapse.py --reference <reference checkout>
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 16000
FILES = [
    ('nested', [(1, 100, 900), (1, 300, 500), (1, 100, 200)]),
    ('chained', [(2, 0, 400), (2, 900, 1400), (2, 350, 1000), (2, 1400, 1401)]),
    ('touching', [(3, 1000, 2000), (3, 2000, 2500), (3, 500, 1000)]),
    ('disjoint', [(4, 0, 1000), (4, 1001, 2000), (4, 5000, 6000)]),
    ('interleaved', [(0, 0, 300), (5, 100, 400), (0, 250, 600), (9, 260, 270), (5, 500, 700), (0, 601, 800), (9, 265, 900), (5, 400, 450),
                     (9, 2000, 2100)]),
    ('single', [(7, 123, 45678)]),
    ('empty', []),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference repository')
    ref = ap.parse_args().reference
    import pandas as pd
    if not hasattr(pd.DataFrame, 'append'):
        pd.DataFrame.append = lambda self, other, ignore_index=False: pd.concat([self, other], ignore_index=ignore_index)
    sys.path.insert(0, ref)
    from data_utils.collapse_event import collapse

    rows = [(f'{name}.wav', f'c{c}', on / SR, end / SR) for name, events in FILES for c, on, end in events]
    got = collapse(pd.DataFrame(rows, columns=['filename', 'event_label', 'onset', 'offset']))
    index = {f'{name}.wav': i for i, (name, _) in enumerate(FILES)}
    grid = lambda t: np.asarray([int(round(float(v) * SR)) for v in t], np.int64)
    assert all(abs(float(v) * SR - round(float(v) * SR)) < 1e-6 for v in list(got.onset) + list(got.offset))
    res = {'sr': np.int64(SR), 'n_files': np.int64(len(FILES)), 'names': np.asarray([n for n, _ in FILES]),
           'in_file': np.asarray([i for i, (_, ev) in enumerate(FILES) for _ in ev], np.int64),
           'in_cls': np.asarray([c for _, ev in FILES for c, _, _ in ev], np.int64),
           'in_on': np.asarray([o for _, ev in FILES for _, o, _ in ev], np.int64),
           'in_end': np.asarray([e for _, ev in FILES for _, _, e in ev], np.int64),
           'out_file': np.asarray([index[f] for f in got.filename], np.int64),
           'out_cls': np.asarray([int(l[1:]) for l in got.event_label], np.int64),
           'out_on': grid(got.onset), 'out_end': grid(got.offset)}
    assert len(res['out_on']) < len(res['in_on']) and index['empty.wav'] not in set(res['out_file'].tolist())
    np.savez_compressed(os.path.join(HERE, 'g25_collapse.npz'), **res)
    print('G25 ok', os.path.getsize(os.path.join(HERE, 'g25_collapse.npz')), 'bytes;', len(res['in_on']), 'events ->', len(res['out_on']))


if __name__ == '__main__':
    main()
