#!/usr/bin/env python3
"""Generate tests/golden/g22_gemm_dispatch.npz: the kernel instance, return status and split factor the GEMM dispatcher of ONE build of
the library gives for every problem of tests/gemm_dispatch_sweep.py (sedt_igemm_describe / sedt_igemm_group_describe /
sedt_igemm_splitk: host code on fake addresses, no device).  tests/test_gemm_split_cpu.py holds the current library to this record.

Made from the library built at the commit BEFORE a change to the planning code (build that commit, pass its libsedt_hip.so as --lib);
re-made on purpose, with the change that retunes a rule, never to make a refactor pass.

Stored: `answers`, the distinct answer strings, and `index`, one uint16 per problem into them (the sweep's order).

usage:  python tests/golden/make_golden_dispatch.py --lib <libsedt_hip.so of the recorded commit>
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True, help='the product library of the commit whose dispatch is recorded')
    lib_path = os.path.abspath(ap.parse_args().lib)
    sys.path[:0] = [os.path.join(HERE, '..'), os.path.join(HERE, '..', '..')]
    from sound_event_detection_transformer_amd import lib as L
    import gemm_dispatch_sweep as S
    L.LIB_PATH = lib_path
    got = S.answers(L)
    answers = sorted(set(got))
    assert len(answers) < 65536
    where = {a: i for i, a in enumerate(answers)}
    index = np.asarray([where[a] for a in got], np.uint16)
    refused = sum(any(not part.startswith('0:') for part in a.split('|')[:2]) for a in got)
    path = os.path.join(HERE, 'g22_gemm_dispatch.npz')
    np.savez_compressed(path, answers=np.asarray(answers), index=index)
    labels = {part.split(':', 1)[1] for a in answers for part in a.split('|')[:2]}
    print('G22 ok', os.path.getsize(path), 'bytes;', len(got), 'problems,', len(answers), 'distinct answers,', refused, 'refused,',
          len(labels - {''}), 'instances; missing from the table:', sorted(S.table_instances() - labels))


if __name__ == '__main__':
    main()
