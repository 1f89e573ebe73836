#!/usr/bin/env python3
"""Generate tests/golden/g24_conv_forms.npz: for every case of tests/conv_plan_cases.py the launch form ops.conv_fwd / ops.conv_dgrad
choose, whether its operands are split (x3), the hint a recording attaches, the argument blocks of the grouped forms and the label of the
kernel their launch runs on - all on the CPU (stand-in operands, recorded launches, sedt_igemm_group_describe).
tests/test_conv_plan_cpu.py holds the current code to this record.

The record was made ONCE, from the commit before the dispatch moved into ops.conv_form, by driving that commit's entry points through
the same sweep; this generator reproduces it from the current code (--check compares the arrays, byte for byte, with the committed file
instead of writing). It is
re-made on purpose, with the change that moves an envelope or adds a form, never to make a refactor pass.

Stored: `names`, one per case; `answers`, the distinct answer strings; `index`, one uint16 per case into them.

usage:  python tests/golden/make_golden_conv_forms.py [--check]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'g24_conv_forms.npz')


def record():
    sys.path[:0] = [os.path.join(HERE, '..'), os.path.join(HERE, '..', '..')]
    from sound_event_detection_transformer_amd import lib as L, ops
    import conv_plan_cases as S
    cases = S.cases()
    got = [S.answer(ops, L, c) for c in cases]
    answers = sorted(set(got))
    where = {a: i for i, a in enumerate(answers)}
    return dict(names=np.asarray([c['name'] for c in cases]), answers=np.asarray(answers),
                index=np.asarray([where[a] for a in got], np.uint16))


def main():
    rec = record()
    if '--check' in sys.argv[1:]:
        old = np.load(PATH)
        same = sorted(old.files) == sorted(rec) and all(old[k].dtype == rec[k].dtype and old[k].tobytes() == rec[k].tobytes() for k in rec)
        print('G24', 'reproduced byte for byte' if same else 'DIFFERS', len(rec['names']), 'cases')
        sys.exit(0 if same else 1)
    np.savez_compressed(PATH, **rec)
    print('G24 ok', os.path.getsize(PATH), 'bytes;', len(rec['names']), 'cases,', len(rec['answers']), 'distinct answers')


if __name__ == '__main__':
    main()
