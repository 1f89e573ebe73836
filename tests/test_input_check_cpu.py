"""CPU: the checker of tests/test_input_envelope_gpu.py checked without a GPU (tests/input_check.py, rows in tests/input_cases.py).

* every table is well-formed and reaches the edge it names: G, idle threads, trips per thread, LDS bytes, clips per wave, boxes per
  lane and float4 per block are computed from the rows by the helpers of input_cases;
* the LDS byte formulas agree with the refusal thresholds 639 / 640, 622 / 623, 575 / 576 and 2558 / 2559;
* every row's inputs are seeded (two calls give the same bytes) and finite apart from the poison rows;
* the np.float32 restatement of every kernel, in the kernel's summation order, passes its own checker on every row; the largest
  error / bound ratios are printed (-s);
* every injected fault of input_check.FAULTS fails at least one row of its kernel;
* the decisions of utilities.mixup.plan_mixup_label_unlabel on the designed pairs are the ones written down by hand;
* the resampler at 128 rows reproduces the copy, and the local resampler equals transforms_oracle.pil_resize_rows.
"""
import collections

import numpy as np
import pytest

import input_cases as IC
import input_check as K
from oracle import transforms_oracle as TO

RATIOS = collections.defaultdict(float)


@pytest.fixture(scope='module', autouse=True)
def _table():
    yield
    if RATIOS:
        print('\nlargest error / bound ratio of the np.float32 restatements:')
        for k in sorted(RATIOS):
            print(f'  {k:24s} {RATIOS[k]:.3g}')


def _recs(c):
    """the single-view records of a row of either transform table"""
    return [r for q in c['recs'] for r in (q[:2] if isinstance(q[0], tuple) else (q,))]


def test_tables_are_well_formed():
    assert set(IC.CASES) == set(K.KERNELS)
    names = [c['name'] for rows in IC.CASES.values() for c in rows]
    assert len(names) == len(set(names))
    for key, rows in IC.CASES.items():
        assert rows, key
        for c in rows:
            assert c['via'] in ('ops', 'c') and c['edge'], c['name']
    for c in IC.BOX_TRANSFORM + IC.BOX_TRANSFORM_VIEWS:
        F, fr = c['F'], c['frames']
        for nraw, tm_t, tm_t0, fm_f, fm_f0, fm_on, sh in _recs(c):
            assert 0 <= nraw <= IC.raw_stride(c) and 0 <= tm_t0 and tm_t0 + tm_t <= fr and 0 <= fm_f0 and fm_f0 + fm_f <= F and abs(sh) < F, c['name']
        assert IC.raw_stride(c) > max(r[0] for r in _recs(c))            # a stride larger than every clip's rows
    for c in IC.BOX_TRANSFORM_VIEWS:
        assert c['F'] % 2 == 0 and c.get('offset', 0) % 2 == 0
    for c in IC.MIXUP_TARGETS:
        assert 0 <= c['ns1'] <= c['B1'] and 0 <= c['mix_num'] <= min(c['B1'], c['B2']) and 1 <= c['B2'] <= 4096 and c['max_targets'] >= c['max_events']
    for c in IC.QUERY:
        for b, s, e in c['jobs']:
            assert 0 <= b < c['B'] and 0 <= s < e <= c['T'] and (not c['fixed'] or e - s == 128), c['name']


def test_box_transform_rows_reach_their_edges():
    rows = [c for c in IC.BOX_TRANSFORM if not c.get('refuse')]
    assert {c['F'] for c in rows if c['edge'] == 'F'} == set(IC.FS)
    assert {(c['log'], c['norm']) for c in rows if c['edge'] == 'F' and c['F'] == 40} == set(IC.MODES4)
    assert IC.idle_threads(40) == 24 and IC.groups(40) == 25 and IC.idle_threads(64) == 0 and IC.groups(1024) == 1 and IC.groups(2) == 512
    assert all(c['frames'] <= 39 for c in rows if c['F'] == 1024)
    el = {c['frames'] * c['F'] for c in rows if c['edge'] == 'elements'}
    assert el == {960, 1024, 1024 + 64} and [IC.trips(n) for n in sorted(el)] == [1, 1, 2]
    assert any(c['frames'] == 1 for c in rows)
    for c in (c for c in rows if c['edge'] == 'nraw'):
        fr = c['frames']
        assert [r[0] for r in c['recs']] == [0, 1, fr - 1, fr, fr + 1, 2 * fr] and IC.raw_stride(c) == 2 * fr + 3
    tm = [(r, c['frames']) for c in rows if c['edge'] == 'tm' for r in c['recs']]
    assert any(r[2] + r[1] == fr and r[1] > 0 for r, fr in tm)                         # ends at the last frame
    assert any(r[2] >= r[0] and r[1] > 0 for r, fr in tm)                              # entirely in the padding
    assert any(r[1] == 0 and r[2] > 0 for r, fr in tm)
    fm = [r for c in rows if c['edge'] == 'fm' for r in c['recs']]
    assert any(r[5] and r[3] > 0 and r[4] + r[3] == 64 and r[4] > 0 for r in fm) and any(r[5] and (r[4], r[3]) == (0, 64) for r in fm)
    assert any(r[5] and r[3] == 0 for r in fm) and any(not r[5] and r[3] > 0 for r in fm)
    cf = [c for c in rows if c['edge'] == 'const_fill']
    assert cf and all(c['via'] == 'c' and c['fill_mean'] == 0 and c['fill_const'] == -3.5 for c in cf)
    sh = {(c['F'], r[6]) for c in rows if c['edge'] == 'shift' for r in c['recs']}
    assert sh >= {(40, -39), (40, -1), (40, 0), (40, 1), (40, 39), (64, -IC.MAX_BAND), (64, IC.MAX_BAND)}
    assert any(c.get('silent_clips') and c.get('silent_bands') for c in rows)
    big = [c for c in rows if c['edge'] == 'lds']
    assert big and all(IC.lds_box_transform(c['frames'], c['F']) > IC.LDS_MAX - 64 * 4 for c in big)       # red in the last bytes
    assert any(r[5] and r[3] > 0 for c in big for r in c['recs'])                      # ... and used: a mean fill goes through block_sum
    assert [c['frames'] for c in IC.BOX_TRANSFORM if c.get('refuse')] == [640]


def test_views_rows_reach_their_edges():
    rows = [c for c in IC.BOX_TRANSFORM_VIEWS if not c.get('refuse')]
    assert {c['F'] for c in rows if c['edge'] == 'F'} == set(IC.FS)
    for c in (c for c in rows if c['edge'] == 'F'):
        G = IC.groups(c['F'])
        assert [q[0][0] for q in c['recs']] == [1, G - 1, G, G + 1] and all(q[2] for q in c['recs'])
        assert [IC.rows_per_group(n, c['F']) for n in (G - 1, G, G + 1)] == [1 if G > 1 else 0, 1, 2]
    nel = sorted(q[0][0] * c['F'] for c in rows if c['edge'] == 'pair_loop' for q in c['recs'])
    assert nel == [2046, 2048, 2050] and [IC.trips(n, 2048) for n in nel] == [1, 1, 2]
    on = {c['name'].split('_log')[0]: [q[2] for q in c['recs']] for c in rows if c['edge'] == 'noise_on'}
    assert any(not any(v) for v in on.values()) and any(all(v) for v in on.values()) and any(0 in v and 1 in v for v in on.values())
    assert any(c.get('silent_bands') and all(q[2] for q in c['recs']) for c in rows)
    assert all(any(q[0][1:] != q[1][1:] for q in c['recs']) for c in rows if c['edge'] in ('F', 'noise_on', 'lds'))      # two different records
    d = [c for c in rows if c.get('drawn')]
    assert len(d) == 1 and d[0]['F'] == 40 and d[0]['offset'] > 0 and len(d[0]['recs']) == 3 and IC.raw_stride(d[0]) > max(q[0][0] for q in d[0]['recs'])
    big = [c for c in rows if c['edge'] == 'lds']
    assert big and all(IC.lds_views(c['frames'], c['F']) > IC.LDS_MAX - 64 * 4 and all(q[2] for q in c['recs']) for c in big)
    assert [c['frames'] for c in IC.BOX_TRANSFORM_VIEWS if c.get('refuse')] == [623]


def test_scaler_rows_reach_their_edges():
    rows = [c for c in IC.SCALER if not c.get('refuse')]
    assert {c['F'] for c in rows if c['edge'] == 'F'} == set(IC.FS)
    for c in (c for c in rows if c['edge'] == 'F'):
        fr = c['frames']
        assert sum(c['calls'], []) == [0, 1, fr - 1, fr, fr + 1, 2 * fr]
    g = next(c for c in rows if c['edge'] == 'nraw')
    G = IC.groups(g['F'])
    assert {G - 1, G, G + 1, 0, 1} <= set(sum(g['calls'], [])) and G + 1 <= g['frames']
    cl = next(c for c in rows if c['edge'] == 'clamp')
    assert any(n < 0 for n in sum(cl['calls'], [])) and any(n > IC.raw_stride(cl) for n in sum(cl['calls'], [])) and IC.raw_stride(cl) > cl['frames']
    assert {len(b) for c in rows if c['edge'] == 'B' for b in c['calls']} >= {1, 2, 5} and all(len(c['calls']) == 2 for c in rows)
    assert {c['log'] for c in rows} == {0, 1}


def test_mixup_rows_reach_their_edges():
    assert {c['clip4'] for c in IC.MIXUP if c['edge'] == 'c4'} == {1, 255, 256, 257, 16384, 16385, 32773}
    assert [IC.mix_grid_x(n) for n in IC.MIX_C4] == [1, 1, 1, 2, 64, 64, 64] and [IC.mix_trips(n) for n in IC.MIX_C4] == [1, 1, 1, 1, 1, 2, 3]
    for c in (c for c in IC.MIXUP if c['edge'] == 'c4'):
        j = c['jobs']
        assert {q[2] for q in j} == {0, 1, 2} and {q[3] for q in j if q[2] == 0} == {0.0, 1.0, 0.37}
        assert any(q[0] != i for i, q in enumerate(j)) and any(q[1] != i for i, q in enumerate(j))
        assert len({q[0] for q in j}) < len(j) and len({q[1] for q in j}) < len(j)          # sources repeat
    assert any(not c['jobs'] for c in IC.MIXUP) and any(c.get('refuse') and c['rem'] % 4 for c in IC.MIXUP)


def test_mixup_targets_rows_reach_their_edges():
    k = K.KERNELS['mixup_targets']
    rows = IC.MIXUP_TARGETS
    assert {c['B2'] for c in rows} >= set(IC.MT_B2) and [IC.clips_per_wave(b) for b in IC.MT_B2] == [1, 1, 1, 2, 3, 5]
    for c in (c for c in rows if c['edge'] == 'B2' and c['B2'] > 16):       # a wave's later clip decides something other than the default
        assert K.expected_decision(c, c['B2'] - 1) == 1 and (c['B2'] - 1) // 16 + 1 == IC.clips_per_wave(c['B2'])
    cand = {}
    for c in (c for c in rows if c['edge'] == 'nbox'):
        y1t, y1r, y2 = k.targets(c)
        for i in c['design']:
            n = len(y1r[i][1]) + len(y2[i][1])
            cand[n] = IC.boxes_per_lane(n)
            assert n == c['max_events']
    assert cand == {63: 1, 64: 1, 65: 2, 130: 3}
    me = next(c for c in rows if c['edge'] == 'max_events')
    y1t, y1r, y2 = k.targets(me)
    tot = {(len(y1r[i][1]) + len(y2[i][1]) - me['max_events'], len(y2[i][1]) > 0) for i in range(me['B2'])}
    assert tot >= {(0, False), (1, False), (0, True), (1, True)}
    (l1, b1), (l2, b2) = K.DESIGN['touch']
    f = np.float32
    assert f(b1[0][0]) + f(b1[0][1]) / f(2) == f(b2[0][0]) - f(b2[0][1]) / f(2) and l1 == l2
    (l1, b1), (l2, b2) = K.DESIGN['ulp_apart']
    t1, s2 = f(f(b1[0][0]) + f(b1[0][1]) / f(2)), f(f(b2[0][0]) - f(b2[0][1]) / f(2))
    assert t1 < s2 and np.nextafter(t1, f(1)) == s2 and l1 == l2
    used = {d if isinstance(d, str) else d[0] for c in rows for d in c['design'].values()}
    assert used >= {'touch', 'touch_reversed', 'ulp_apart', 'other_class_overlap', 'overlap', 'weak_first', 'weak_plain', 'many', 'many_clash_last', 'count'}
    assert any(c['split'] is not None and c['split'] < c['ns1'] for c in rows) and any(c['split'] is not None and c['split'] > c['ns1'] for c in rows)
    assert any(c['mix_num'] == 0 for c in rows) and any(c['mix_num'] == c['B2'] == c['B1'] for c in rows)
    assert {(c['ratio1'], c['ratio_out']) for c in rows} == {(1, 1), (0, 1), (1, 0), (0, 0)}
    for c in (c for c in rows if c['edge'] == 'cap'):
        inp = k.make(c)
        e = k.expected(c, inp)
        assert inp['cap'] - max(e['lab_off'][-1], e['box_off'][-1]) == c['cap'] and c['cap'] in (-1, 0)
    assert {c['cap'] for c in rows if c['edge'] == 'cap'} == {-1, 0}


@pytest.mark.parametrize('c', IC.MIXUP_TARGETS, ids=lambda c: c['name'])
def test_plan_decisions_are_the_ones_written_down(c):
    k = K.KERNELS['mixup_targets']
    modes = k.expected(c, k.make(c))['modes']
    assert modes == [K.expected_decision(c, i) for i in range(c['B2'])]
    if c['mix_num'] > 2 and c['edge'] not in ('cap', 'mix_num'):
        assert len(set(modes[:c['mix_num']])) >= 2 or c['edge'] == 'B2'


def test_query_rows_reach_their_edges():
    rows = [c for c in IC.QUERY if not c.get('refuse')]
    free = [c for c in rows if not c['fixed']]
    big = next(c for c in free if c['F'] == 64 and c['edge'] == 'h')
    hs = {e - s for b, s, e in big['jobs']}
    assert hs == {1, 2, 3, 127, 128, 129, 255, 256, big['T']}
    for h in hs:
        assert any(s == 0 and e - s == h for b, s, e in big['jobs']) and any(e == big['T'] and e - s == h for b, s, e in big['jobs'])
    assert {c['F'] for c in free} >= {8, 24, 64}
    odd = [(e - s) for c in free if c['F'] == 24 for b, s, e in c['jobs'] if (e - s) % 2]
    assert odd and all(IC.query_scratch_offset(h, 24) != h * 24 for h in odd) and IC.query_scratch_offset(128, 64) == 128 * 64
    fx = [c for c in rows if c['fixed']]
    assert any(s == 0 for c in fx for b, s, e in c['jobs']) and any(e == c['T'] for c in fx for b, s, e in c['jobs'])
    assert all(len({b for b, s, e in c['jobs']}) > 1 for c in rows if len(c['jobs']) > 3)       # patches of different clips in one launch
    assert any(not c['jobs'] for c in rows) and any(c['via'] == 'ops' for c in rows)
    assert any(c['T'] == 2558 and any(e - s == 2558 for b, s, e in c['jobs']) for c in rows)
    for c in (c for c in rows if c['via'] == 'ops'):
        assert all(K.box_of_rows(s, e, c['T']) is not None for b, s, e in c['jobs'])


def test_lds_formulas_agree_with_the_refusal_thresholds():
    L = IC.LDS_MAX
    assert IC.lds_box_transform(639, 64) <= L < IC.lds_box_transform(640, 64)
    assert IC.lds_views(622, 64) <= L < IC.lds_views(623, 64)
    assert IC.lds_scaler(575, 64) <= L < IC.lds_scaler(576, 64)
    assert IC.lds_query(2558, 64) <= L < IC.lds_query(2559, 64)
    for key, fn in (('box_transform', IC.lds_box_transform), ('box_transform_views', IC.lds_views), ('scaler_update', IC.lds_scaler)):
        for c in IC.CASES[key]:
            assert (fn(c['frames'], c['F']) > L) == bool(c.get('refuse')), c['name']
    for c in IC.QUERY:
        assert (IC.lds_query(c['T'], c['F']) > L) == bool(c.get('refuse')), c['name']


def _poisoned(a, nraws, what):
    """rows < nraw finite, rows >= nraw NaN (even clips) or 1e30 (odd clips)"""
    for i, n in enumerate(nraws):
        assert np.isfinite(a[i, :n]).all(), (what, i)
        assert np.isnan(a[i, n:]).all() if i % 2 == 0 else (a[i, n:] == np.float32(1e30)).all(), (what, i)


@pytest.mark.parametrize('key', sorted(IC.CASES))
def test_inputs_are_seeded_and_finite_apart_from_the_poison(key):
    k = K.KERNELS[key]
    for c in IC.CASES[key]:
        a, b = k.make(c), k.make(c)
        assert a.keys() == b.keys()

        def arrays(d):
            return {n: v for n, v in d.items() if isinstance(v, np.ndarray)} | \
                   {f'{n}{i}.{m}': w for n, v in d.items() if n == 'calls' for i, q in enumerate(v) for m, w in q.items()}
        for n, v in arrays(a).items():
            assert v.dtype == arrays(b)[n].dtype and v.tobytes() == arrays(b)[n].tobytes(), (c['name'], n)
            if v.dtype.kind == 'f' and n not in ('amp', 'z') and not n.endswith('.amp'):
                assert np.isfinite(v).all(), (c['name'], n)
        if key in ('box_transform', 'box_transform_views'):
            nraws = [r[0] for r in _recs(c)][::2 if key == 'box_transform_views' else 1]
            _poisoned(a['amp'], nraws, c['name'])
            if 'z' in a and not c.get('drawn'):
                _poisoned(a['z'], nraws, c['name'])
        if key == 'scaler_update':
            for call in a['calls']:
                _poisoned(call['amp'], [k.eff(c, n) for n in call['nf']], c['name'])


def test_clips_differ_by_decades():
    c = next(c for c in IC.BOX_TRANSFORM if c['edge'] == 'nraw')
    a = K.KERNELS['box_transform'].make(c)['amp']
    med = [np.median(a[b, :r[0]]) for b, r in enumerate(c['recs']) if r[0] > 1]
    assert max(med) / min(med) > 100.0


@pytest.mark.parametrize('key', sorted(IC.CASES))
def test_restatement_passes_its_own_checker(key):
    for c in IC.CASES[key]:
        if c.get('refuse'):                                      # nothing runs: the entry point raises (GPU module)
            continue
        for name, r in K.restated(key, c).items():
            RATIOS[name] = max(RATIOS[name], r)
            assert r <= 1.0


@pytest.mark.parametrize('key,fault', K.FAULTS, ids=[f'{k}-{f}' for k, f in K.FAULTS])
def test_injected_fault_fails(key, fault):
    failed = []
    for c in IC.CASES[key]:
        if c.get('refuse'):
            continue
        try:
            K.restated(key, c, fault)
        except AssertionError:
            failed.append(c['name'])
            break
    assert failed, f'{fault} passed every row of {key}'


def test_the_issues_faults_are_all_listed():
    want = [('box_transform', 'shift_off_by_one'), ('box_transform', 'mask_end_inclusive'), ('box_transform', 'floor_from_kept'),
            ('box_transform', 'stride_is_nraw'), ('box_transform_views', 'sd_div_frames'), ('mixup_targets', 'second_clip_skipped'),
            ('mixup_targets', 'box64_ignored'), ('mixup_targets', 'max_events_ge'), ('mixup_targets', 'touch_separate'),
            ('mixup', 'last_float4_dropped'), ('query_patches', 'copy_branch_from_128'), ('scaler_update', 'divisor_keep')]
    assert set(want) <= set(K.FAULTS)


def test_frame_sees_a_write_in_either_guard():
    for where in (K.GUARD - 1, K.GUARD + 5):
        f = K.Frame(np.float32, 5)
        f.own()[:] = 0
        f.check_guard(f.buf, 'clean')
        f.buf[where] = 0
        with pytest.raises(AssertionError):
            f.check_guard(f.buf, 'dirty')
    assert K.GUARD * 4 % 16 == 0                                 # a framed output stays float4-aligned


def test_resampler_at_128_rows_is_the_copy():
    """query_patch_kernel's h == 128 branch is Pillow's same-size copy; the resampler at scale 1 has the weights 1 and 0 and gives the
    same codes, so taking the resampler there is not an observable fault"""
    code = np.random.default_rng(1).integers(0, 256, (128, 24)).astype(np.uint8)
    assert np.array_equal(K.resample_rows(code, 128, copy_branch=False), code)
    for h in (1, 2, 3, 127, 129, 255, 256, 300, 2558):
        code = np.random.default_rng(h).integers(0, 256, (h, 8)).astype(np.uint8)
        assert np.array_equal(K.resample_rows(code), TO.pil_resize_rows(code, 128)), h


def test_query_reference_is_the_oracles_on_rows_a_box_reaches():
    k = K.KERNELS['query_patches']
    n = 0
    for c in IC.QUERY:
        if c.get('refuse') or c['T'] > 1000:
            continue
        inp = k.make(c)
        for (b, s, e, _), ref in zip(inp['jobs'], k.reference(c, inp)):
            box = K.box_of_rows(int(s), int(e), c['T'])
            if box is not None and (c['fixed'] or e - s > 1):
                assert np.array_equal(TO.query_patches(inp['data'][b][None], [box], bool(c['fixed']))[0][0, 0], ref), (c['name'], s, e)
                n += 1
    assert n > 20
