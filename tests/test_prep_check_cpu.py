"""CPU: the checker of tests/test_prep_envelope_gpu.py checked without a GPU (tests/prep_check.py, rows in tests/prep_cases.py).

* the tables hold a row on either side of every condition that reduce_job_mode, reduce_job_blocks and the pack tile rule test, and
  every unroll remainder of the reduce kernel's slice loops (restated in prep_cases): a row deleted later fails here;
* every row's inputs are seeded; the np.float32 restatement of every kernel passes its own checker (bits, and float64 under the bound)
  on every row; the largest ratios are printed (-s);
* every planted fault of prep_check.FAULTS fails at least one row - the tail faults in every mode - and the test names the rows;
* the planted double-rounding products differ from a single rounding of the float64 product;
* the job search restated: every block of a table reaches its job, and the off-by-one search does not.
"""
import collections

import numpy as np
import pytest

import prep_cases as PC
import prep_check as K
from glue_check import F, bits, from_bf16, ratio_key, to_bf16

RATIOS = collections.defaultdict(float)


@pytest.fixture(scope='module', autouse=True)
def _table():
    yield
    if RATIOS:
        print('\nlargest error / bound ratio of the np.float32 restatements:')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')


def test_tables_are_well_formed():
    assert set(PC.CASES) == set(K.KERNELS)
    names = [c['name'] for rows in PC.CASES.values() for c in rows]
    assert len(names) == len(set(names))
    assert all(rows for rows in PC.CASES.values())


def test_pack_rows_reach_every_path_and_tile_edge():
    for dt in PC.DTS:
        rows = [c for c in PC.PACK if c['dt'] == dt]
        shapes = {(c['Co'], c['Ci'], c['taps']) for c in rows}
        assert shapes >= {(co, ci, 1) for co, ci in PC.PACK_T1_VEC + PC.PACK_T1_SCALAR} | {(co, ci, 9) for co, ci in PC.PACK_T9_VEC + PC.PACK_T9_SCALAR}
        assert shapes >= {(co, ci, t) for t in PC.PACK_RT_TAPS for co, ci in PC.PACK_RT_SHAPES}
        by = collections.defaultdict(list)
        for c in rows:
            by[(PC.pack_path(c), c['taps'])].append(c)
        assert {k for k in by} >= {('vec', 1), ('scalar', 1), ('vec', 9), ('scalar', 9)} | {('runtime', t) for t in PC.PACK_RT_TAPS}
        for taps, ts in ((1, 64), (9, 32)):
            v = by[('vec', taps)]
            assert any(c['Co'] == ts and c['Ci'] == ts for c in v)                             # exactly one tile
            assert any(PC.pack_blocks(c) == 1 and c['Co'] < ts and c['Ci'] < ts for c in v)    # one partial tile
            assert any(c['Co'] % ts and c['Co'] > ts for c in v) and any(c['Ci'] % ts and c['Ci'] > ts for c in v)      # a partial last tile either way
            assert taps == 9 or any(c['Co'] % ts and c['Ci'] % ts and PC.pack_blocks(c) > 1 for c in v)                 # ... and both at once
            assert any(c['Ci'] % ts == 8 for c in v)                                           # the last ci tile is 8 wide
            s = by[('scalar', taps)]
            assert any(c['Co'] % 8 and c['Ci'] % 8 == 0 for c in s) and any(c['Ci'] % 8 and c['mis'] == 'none' for c in s)
        # scalar by alignment alone, one pointer each; the same shape runs aligned
        mis = [c for c in rows if c['mis'] != 'none']
        assert {c['mis'] for c in mis} == {'w', 'wf', 'wb'} and all(c['Co'] % 8 == 0 and c['Ci'] % 8 == 0 and PC.pack_path(c) == 'scalar' for c in mis)
        assert all(any(PC.pack_path(a) == 'vec' and (a['Co'], a['Ci'], a['taps']) == (c['Co'], c['Ci'], c['taps']) and a['scale'] and a['wf'] and a['wb']
                       for a in rows) for c in mis)
        for path in ('vec', 'scalar'):
            sel = [c for c in rows if PC.pack_path(c) == path]
            assert any(not c['wf'] for c in sel) and any(not c['wb'] for c in sel) and any(not c['scale'] for c in sel), path
        assert any(PC.pack_path(c) == 'runtime' and not c['scale'] for c in rows) and any(PC.pack_path(c) == 'runtime' and PC.pack_blocks(c) > 1 for c in rows)
        assert (1, 1, 1) in shapes
        table = PC.pack_table(dt)
        nb = [PC.pack_blocks(c) for c in table]
        assert 60 <= len(table) <= 80 and any(nb[i] == nb[i + 1] == nb[i + 2] == 1 for i in range(len(nb) - 2)) and max(nb) >= 4


def test_frag_rows():
    assert {(c['N'], c['K']) for c in PC.FRAG} == set(PC.FRAG_NK) and all(c['N'] % 32 == 0 and c['K'] % 32 == 0 for c in PC.FRAG)
    for src in PC.DTS:
        assert {(c['N'], c['K'], c['wf'], c['wb']) for c in PC.FRAG if c['src'] == src} == {(n, k, f, b) for n, k in PC.FRAG_NK for f, b in ((1, 1), (1, 0), (0, 1))}
        assert len([c for c in PC.FRAG if c['src'] == src]) == 12


def test_reduce_rows_reach_every_mode_block_edge_and_unroll_remainder():
    R = PC.REDUCE
    al = [c for c in R if c['mis'] == 'none' and c['Ci']]
    m = {k: [c for c in al if PC.reduce_mode(c) == k] for k in range(4)}
    per = lambda c: c['R'] * c['taps'] * c['Ci']
    # mode 0: every remainder of the 4-way unroll after the first slice, at every element count; either side of splitk 16
    assert {(c['splitk'], per(c)) for c in m[0] if c['cs'] is None} >= {(sk, p) for sk in PC.RED_SK0 for p in PC.RED_PER0}
    assert {(sk - 1) % 4 for sk in PC.RED_SK0} == {0, 1, 2, 3} and {(sk - 1) // 4 for sk in PC.RED_SK0} >= {0, 1, 2, 3} and max(PC.RED_SK0) == 15
    assert {PC.reduce_blocks(c) for c in m[0]} >= {1, 2} and {per(c) % 1024 for c in m[0]} >= {4, 1020, 0}
    # mode 3: per group the slices z = g, g + 4, ..: pairs and a tail; every count of slices mod 8 that changes which groups have a tail
    assert {(c['splitk'], per(c)) for c in m[3] if c['cs'] is None} >= {(sk, p) for sk in PC.RED_SK3 for p in PC.RED_PER3}
    assert min(PC.RED_SK3) == 16 and {sk % 8 for sk in PC.RED_SK3} >= {0, 1, 4, 5, 7}
    assert {PC.reduce_blocks(c) for c in m[3]} >= {1, 2} and {per(c) for c in m[3]} >= {252, 256, 260}
    # mode 1: the 3x3 form at 64 and 128 channels, one and three rows, even and odd slice counts; the run-time transposition
    assert {(c['Ci'], c['R'], c['splitk']) for c in m[1] if c['taps'] == 9 and c['cs'] is None} >= {(ci, r, sk) for ci in (64, 128) for r in (1, 3) for sk in range(1, 6)}
    assert {c['taps'] for c in m[1]} >= {2, 3, 4, 8, 9}
    # mode 2: by taps, by Ci (both conditions, either side), by alignment of either pointer on every wide mode's shape
    assert any(c['taps'] == 9 and c['Ci'] % 64 for c in m[2]) and any(c['taps'] == 1 and c['Ci'] % 4 for c in m[2]) and any(c['taps'] == 10 and c['Ci'] % 64 == 0 for c in m[2])
    assert {PC.reduce_blocks(c) for c in m[2]} >= {1, 2}
    for which in ('slab', 'out'):
        wide = {PC.reduce_mode(dict(c, mis='none')) for c in R if c['mis'] == which}
        assert wide == {0, 1, 3} and all(PC.reduce_mode(c) == 2 for c in R if c['mis'] == which)
    for k in range(4):
        assert {c['scale'] for c in m[k]} == {0, 1}, k
    # riding column sums
    cs = [c for c in R if c['cs'] is not None and c['Ci']]
    assert {c['R'] for c in cs} >= set(PC.RED_CS_R) and any(c['cs'] == 0 for c in cs) and any(c['cs'] not in (0, c['splitk']) for c in cs)
    assert {PC.cs_slices(c) for c in R if c['cs'] is not None} >= set(PC.RED_CS_SLICES)
    n = sorted({PC.cs_slices(c) for c in R if c['cs'] is not None})
    assert {((k - g + 3) // 4) % 4 for k in n for g in range(4) if k > g} == {0, 1, 2, 3}          # sums per group: every remainder of the 4-sum walk
    assert any(PC.reduce_blocks(c) > PC.reduce_blocks(c, sums=False) for c in cs)
    assert {PC.reduce_mode(c) for c in cs} == {0, 1, 2, 3}
    so = [c for c in R if not c['Ci']]
    assert {(c['R'], c['splitk']) for c in so} >= {(256, 1), (256, 15), (256, 16), (256, 512)} and any(c['R'] == 100 for c in so)
    assert all(c['cs'] == 0 and c['taps'] == 1 for c in so)
    t = PC.reduce_table()
    assert len(t) == PC.MAX_REDUCE_JOBS and {PC.reduce_mode(c) for c in t if c['Ci']} == {0, 1, 2, 3}
    assert any(not c['Ci'] for c in t) and any(c['cs'] is not None and c['Ci'] for c in t) and any(c['mis'] != 'none' for c in t)
    nb = [PC.reduce_blocks(c) for c in t]
    assert any(nb[i] == nb[i + 1] == 1 for i in range(len(nb) - 1)) and max(nb) > 2


def test_bn_and_stem_rows():
    assert [c['n'] for c in PC.BN_FOLD] == [0, 1, 255, 256, 257, 2048]
    rv = K.KERNELS['bn_fold'].make(PC.BN_FOLD[-1])['rv']
    assert {0.0, float(F(1e-5)), 1.0, float(F(1e4))} <= set(rv.tolist())
    assert {c['dt'] for c in PC.STEM_PREP} == set(PC.DTS)
    g = K.KERNELS['stem_conv0_grad'].make(PC.STEM_CONV0_GRAD[0])['G']
    assert np.isnan(g[:, 49:64]).all() and np.isnan(g[:, 113:]).all() and np.isfinite(g[:, :49]).all() and np.isfinite(g[:, 64:113]).all()


@pytest.mark.parametrize('key', sorted(PC.CASES))
def test_inputs_are_seeded(key):
    k = K.KERNELS[key]
    for c in PC.CASES[key]:
        a, b = k.make(c), k.make(c)
        assert a.keys() == b.keys() and all(np.array_equal(bits(a[n]), bits(b[n])) for n in a), c['name']


@pytest.mark.parametrize('key', sorted(PC.CASES))
def test_restatement_passes_its_own_checker(key):
    for c in PC.CASES[key]:
        for name, r in K.restated(key, c).items():
            RATIOS[ratio_key(name, c)] = max(RATIOS[ratio_key(name, c)], r)
            assert name.startswith('k:') or r <= 1.0


@pytest.mark.parametrize('key,fault', K.FAULTS, ids=[f'{k}-{f}' for k, f in K.FAULTS])
def test_planted_fault_fails(key, fault):
    failed = []
    for c in PC.CASES[key]:
        try:
            K.restated(key, c, fault)
        except AssertionError:
            failed.append(c)
    assert failed, f'{fault} passed every row of {key}'
    print(f'\n{key}-{fault}: fails {len(failed)} rows, first {failed[0]["name"]}')
    if key == 'reduce' and fault in ('tail_dropped', 'tail_twice'):
        assert {PC.reduce_mode(c) for c in failed} == {0, 1, 2, 3}, 'the tail fault passes a whole mode'
    if key == 'pack' and fault == 'truncate':
        assert all(c['dt'] == 'bf16' for c in failed)
    if key == 'pack' and fault == 'neighbour_scale':
        assert {PC.pack_path(c) for c in failed} == {'vec', 'scalar', 'runtime'}


def test_planted_products_round_twice():
    """the dgrad image is bf16(float32(w * scale)): at the planted elements one rounding from float64 gives another bf16"""
    k = K.KERNELS['pack']
    n = 0
    for c in PC.PACK:
        inp = k.make(c)
        for co, ci, tap in k.planted(c):
            w, s = inp['w'][co, ci, tap], inp['scale'][co]
            twice = int(to_bf16(np.array([w * s], F))[0])
            once = K.bf16_once(np.float64(w) * np.float64(s))
            assert twice != once and abs(twice - once) == 1, c['name']
            if c['dt'] == 'bf16' and c['wb']:
                assert int(k.images(c, inp)['wb'].reshape(c['Ci'], c['taps'], c['Co'])[ci, tap, co]) == twice
            n += 1
    assert n >= 2 * len([c for c in PC.PACK if c['scale'] and c['Co'] >= 4]) - 8 and n > 50
    assert K.bf16_once(1.00390625) == 0x3F80 and K.bf16_once(1.00390626) == 0x3F81 and K.bf16_once(-1.01171875) == 0xBF82
    assert float(from_bf16(np.array([K.bf16_once(3.0)], np.uint16))[0]) == 3.0


def test_job_search_reaches_every_block_and_the_off_by_one_search_does_not():
    tables = [[PC.reduce_blocks(c) for c in PC.reduce_table()]] + [[PC.pack_blocks(c) for c in PC.pack_table(dt)] for dt in PC.DTS] + [[1], [1, 1], [3, 1, 1, 2]]
    for nb in tables:
        assert PC.table_coverage(nb) == [list(range(n)) for n in nb]
        if len(nb) > 1:
            bad = [j for j, (got, n) in enumerate(zip(PC.table_coverage(nb, 'search_off_by_one'), nb)) if got != list(range(n))]
            assert bad, nb
            print(f'\nsearch_off_by_one: jobs {bad[:6]} of a table of {len(nb)} lose or gain a block')
