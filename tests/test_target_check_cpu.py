"""CPU: the checker of tests/test_target_envelope_gpu.py tested on itself (tests/target_check.py, rows in tests/target_cases.py).

For every family a float32 restatement of the kernel (the reference run in float32) must pass the comparators that the device
results face; deliberately wrong outputs must fail them: two matched queries swapped, a gradient row scaled by 1 + 1e-3, the no-object
column's gradient dropped, non-zero rows for the audio-tag query, one event kept that overlap removal should drop, an offset not
clamped at cap, a guard byte touched; also a row loss wrong by 1e-4 of itself and 1e-5 in a feature-gradient row that must be zero.  The conditions the rows rely on are asserted for the exact seeds of the table: scipy's optimum is
the same on float64 costs and on their float32 roundings, the fine-tune comparisons sit away from their thresholds, no two surviving
scores of a pseudo-label clip are equal, the special clips and caps are what their rows say, the coincident row really pairs the
coincident intervals, and the table holds the sizes on both sides of every stride.

Largest error / bound ratio of the float32 restatements (pytest -s prints them); index outputs and copied values are exact (0):
  match          gt_weak 0.000124   coef 0   wbox 0
  criterion      out 0.013   dl 0.00346   db 0.000263   db2 0.0119   dat 0.00116   dat_p 0.000465
  criterion_bwd  glogits 0.00569   gboxes 0.0122   gat 0.00116   gat_p 0.000459
  post           scores 0.107   boxes 0.0511
  feature        out 0.0132   rowloss 0.0202   dpred 0.00265   total 0.00509
  sum_f32        0.00662        scale_layers 0.266
"""
import collections

import numpy as np
import pytest
import torch

import target_cases as TC
import target_check as K

RATIOS = collections.defaultdict(float)


def teardown_module(module):
    if RATIOS:
        print('\nlargest error / bound ratio of the float32 restatements:')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')


def _note(fam, r):
    for k, v in r.items():
        RATIOS[f'{fam} {k}'] = max(RATIOS[f'{fam} {k}'], v)
    assert all(v <= 1.0 for v in r.values()), (fam, r)


def _ids(rows):
    return [c.name for c in rows]


# ------------------------------------------------------------------------------------------------ the table itself
def test_table_sits_on_the_edges():
    names = [(c.family, c.name) for c in TC.ALL]
    assert len(set(names)) == len(names)
    cr = {c.name: c.shape for c in TC.CRITERION}
    assert sorted(s['L'] * s['B'] * s['Q'] for n, s in cr.items() if n.startswith('lbq')) == [1023, 1024, 1025]
    assert sorted(s['B'] * s['Q'] for n, s in cr.items() if n.startswith('bq')) == [63, 64, 65]
    assert cr['lb8192_q1']['L'] * cr['lb8192_q1']['B'] == 8192
    assert [cr[n]['Bat'] * cr[n]['C'] for n in ('bat16_c63', 'bat17_c63')] == [1008, 1071]
    assert cr['atp_weak']['Bp'] > cr['atp_weak']['n_lab']
    assert {c.shape['C'] + 1 for c in TC.CRITERION} >= {16, 17, 64} and {c.shape['L'] for c in TC.CRITERION} >= {1, 8}
    for c in TC.MATCH + TC.CRITERION:
        s = c.shape
        assert 1 <= s['Q'] <= 63 and 1 <= s['C'] <= 63 and 1 <= s['L'] <= 8 and max(s['n']) <= s['mt'] <= 63 and s['q0'] + s['Q'] <= s['Qs']
        assert s['ns'] <= s['n_lab'] <= s['B'] and s['L'] * s['B'] <= 8192
        assert s['Q'] * (s['C'] + 1 + 2 * s['mt']) * 4 <= 64 * 1024                       # the matching tile fits the default LDS
        if c.flags.get('ratio'):
            assert max(s['n']) <= s['Q']              # positional ratios are undefined in the reference with more targets than queries
        if c.flags.get('ft'):
            assert min(s['n']) > 0 and (not c.flags.get('ratio') or c.flags.get('norm'))
    lds = lambda s: (2 * s['B'] + 1 + 3 * s['B'] * s['Q'] + s['C']) * 4
    assert max(lds(c.shape) for c in TC.PSEUDO) > 64 * 1024 and all(lds(c.shape) <= 150 * 1024 for c in TC.PSEUDO)
    assert {c.shape['B'] for c in TC.PSEUDO} >= {15, 16, 17, 33, 100}
    assert {c.shape['F'] for c in TC.FEATURE} >= {4, 252, 256, 260}
    assert {c.shape['L'] * c.shape['B'] * c.shape['Q'] for c in TC.FEATURE} >= {5, 8}
    assert {c.shape['ns'] * c.shape['Q'] for c in TC.FEATURE} >= {255, 257}
    big = next(c for c in TC.SCALE if c.name == 'l1_above_cap')
    assert big.shape['per'] // 4 > 256 * (2048 // big.shape['L'] + 1)


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize('c', TC.MATCH, ids=_ids(TC.MATCH))
def test_match_restatement_passes_and_seed_is_stable(c):
    inp = K.match_inputs(c)
    assert c.flags.get('tie') or K.assignment_stable(inp), 'the optimum changes under float32 rounding of the costs: pick another seed'
    margins = []
    ref = K.match_ref(inp, margins=margins)
    assert all(m > 1e-4 for m in margins), margins          # fine-tune: epsilon, the uniforms and the nearest target are clear-cut
    f32 = K.match_ref(inp, np.float32)
    if c.flags.get('tie'):
        host = K.host_assign(inp)
        assert K.check_tie(inp, host) <= 1e-12 and K.check_tie(inp, f32['assign']) <= 1e-12
        bad = host.copy()
        bad[0, 0, 0] = bad[0, 0, 2]                          # two queries on one target
        assert K.check_tie(inp, bad) == float('inf')
        return
    _note('match', K.check_dense(f32, ref, inp))
    assert np.array_equal(ref['assign'] >= 0, ref['wbox'] > 0)


def test_host_solver_agrees_with_scipy_on_plain_rows():
    for c in TC.MATCH:
        if not (c.flags.get('tie') or c.flags.get('ft')) and c.shape['split'] is None:
            inp = K.match_inputs(c)
            assert np.array_equal(K.host_assign(inp), K.match_ref(inp)['assign']), c.name


def test_swapped_queries_fail():
    c = next(c for c in TC.MATCH if c.name == 'q63_n63_62_1')
    inp = K.match_inputs(c)
    ref = K.match_ref(inp)
    bad = {k: v.copy() for k, v in ref.items()}
    q = np.nonzero(ref['assign'][1, 1] >= 0)[0][:2]
    for k in ('tc', 'coef', 'wbox', 'tbox', 'tidx', 'assign'):
        bad[k][1, 1, q] = bad[k][1, 1, q[::-1]]
    r = K.check_dense(bad, ref, inp)
    assert r['assign'] == float('inf') and r['tidx'] == float('inf') and r['tbox'] == float('inf')
    lost = {k: v.copy() for k, v in ref.items()}
    lost['gt_weak'][0, inp['labels'][0][0]] = 0             # a clip-level tag target dropped
    assert K.check_dense(lost, ref, inp)['gt_weak'] > 1


# ------------------------------------------------------------------------------------------------ criterion
@pytest.fixture(scope='module')
def crit_rows():
    """{name: (inp, float64 reference)} computed once"""
    out = {}
    for c in TC.CRITERION:
        inp = K.crit_inputs(c)
        out[c.name] = (inp, K.criterion_ref(inp))
    return out


@pytest.mark.parametrize('c', TC.CRITERION, ids=_ids(TC.CRITERION))
def test_criterion_restatement_passes(c, crit_rows):
    inp, ref = crit_rows[c.name]
    assert K.assignment_stable(inp)
    f32 = K.criterion_ref(inp, torch.float32)
    _note('criterion', K.check_criterion(f32['out'], f32['terms'], ref, inp))
    for mode in ('g', 'gtotal', 'both'):
        _note('criterion_bwd', K.check_bwd(f32['bwd'][mode], ref['bwd'][mode], inp))


def test_no_events_row_is_not_finite_and_coincident_row_coincides(crit_rows):
    inp, ref = crit_rows['no_events']
    s = K.SLOTS(inp['L'])
    assert np.isinf(ref['out'][0]) and np.isnan(ref['out'][1]) and np.isnan(ref['out'][2]) and np.isnan(ref['out'][s['total']])
    assert not np.isfinite(ref['terms']['dl']).all() and np.isfinite(ref['out'][s['weak']])
    inp, ref = crit_rows['coincident']
    assert inp['dense']['assign'][0, 0].tolist() == [0, 1, 2, -1]
    se = lambda b: (b[..., 0].astype(np.float64) - b[..., 1] / 2, b[..., 0].astype(np.float64) + b[..., 1] / 2)
    (s1, e1), (s2, e2) = se(inp['boxes'][0, 0]), se(inp['tboxes'][0])
    assert s1[0] == s2[0] and e1[1] == e2[1] and e1[2] == s2[2]
    # the float64 autograd of the oracle at these points: min / max split a tie evenly, clamp(min=0) passes at 0, |x| has slope 0 at 0
    assert np.all(ref['terms']['db'][0, 0, 0] == np.asarray([-1.0, -0.5]) * inp['dense']['wbox'][0, 0, 0] / inp['nb'])
    assert np.all(np.isfinite(ref['terms']['db2'])) and np.all(ref['terms']['db2'][0, 0, :3] != 0)


def test_wrong_gradients_fail(crit_rows):
    inp, ref = crit_rows['q0_1']
    f32 = K.criterion_ref(inp, torch.float32)
    assert max(K.check_criterion(f32['out'], f32['terms'], ref, inp).values()) <= 1
    # a gradient row scaled by 1 + 1e-3 (the row that holds the largest entry)
    t = {k: None if v is None else v.copy() for k, v in f32['terms'].items()}
    i = np.unravel_index(np.abs(t['dl']).argmax(), t['dl'].shape)[:3]
    t['dl'][i] *= 1 + 1e-3
    assert K.check_criterion(f32['out'], t, ref, inp)['dl'] > 1
    # the no-object column's gradient dropped
    t = {k: None if v is None else v.copy() for k, v in f32['terms'].items()}
    t['dl'][..., -1] = 0
    assert K.check_criterion(f32['out'], t, ref, inp)['dl'] > 1
    # one loss value off by 3e-5 of itself
    o = f32['out'].copy()
    o[1] *= 1 + 3e-5 * max(1.0, 1.0 / abs(o[1]))
    assert K.check_criterion(o, f32['terms'], ref, inp)['out'] > 1
    # the rows of the audio-tag query (outside the window) not zero
    gl, gb, ga, gp = (None if v is None else v.copy() for v in f32['bwd']['both'])
    assert max(K.check_bwd((gl, gb, ga, gp), ref['bwd']['both'], inp).values()) <= 1
    gl[1, 0, 0, 2] = 1e-9
    assert K.check_bwd((gl, gb, ga, gp), ref['bwd']['both'], inp)['glogits'] == float('inf')
    # a finite value where the reference has none, and the reverse
    inp, ref = crit_rows['no_events']
    o = ref['out'].copy()
    o[1] = 0.0
    assert K.check_criterion(o, ref['terms'], ref, inp)['out'] == float('inf')


# ------------------------------------------------------------------------------------------------ postprocess, pseudo labels
@pytest.mark.parametrize('c', TC.POST, ids=_ids(TC.POST))
def test_post_restatement_passes(c):
    inp = K.post_inputs(c)
    ref = K.post_ref(inp)
    if c.flags['lane63']:
        e = np.exp(inp['logits'].astype(np.float64))
        assert np.all((e / e.sum(-1, keepdims=True))[:, :, c.shape['C'] // 2].argmax(1) == c.shape['Q'] - 1)
    _note('post', K.check_post(K.post_ref(inp, np.float32), ref, inp))
    bad = dict(ref, labels=ref['labels'].copy())
    bad['labels'][0, 0] = (bad['labels'][0, 0] + 1) % max(c.shape['C'], 2)
    assert K.check_post(bad, ref, inp)['labels'] == float('inf')


@pytest.mark.parametrize('c', TC.PSEUDO, ids=_ids(TC.PSEUDO))
def test_pseudo_restatement_passes(c):
    inp = K.pseudo_inputs(c)
    ref = K.pseudo_ref(inp)
    for s in ref['survivors']:
        assert len(np.unique(s)) == len(s) and len(np.unique(s.astype(np.float32))) == len(s), 'two surviving scores are equal'
    Q, cnt = c.shape['Q'], ref['cnt']
    assert len(ref['survivors'][0]) == Q and len(ref['survivors'][1]) == 0 and cnt[1] == 0
    assert len(ref['survivors'][2]) == Q and cnt[2] == (1 if c.flags['nms'] else Q)
    total, off = int(cnt.sum()), np.concatenate([[0], np.cumsum(cnt)])
    want = {'big': inp['cap'] > total, 'total': inp['cap'] == total, 'minus1': inp['cap'] == total - 1,
            'mid': inp['cap'] < total and inp['cap'] not in off, 'boundary': 0 < inp['cap'] < total and inp['cap'] in off}
    assert want[c.flags['cap']], (inp['cap'], total)
    f32 = K.pseudo_ref(inp, np.float32)
    got = dict(lab_cat=f32['lab_cat'], box_cat=f32['box_cat'], lab_off=f32['off'], box_off=f32['off'], hist=f32['hist'])
    r = K.check_pseudo(got, ref)
    _note('pseudo', r)


def test_wrong_pseudo_labels_fail():
    c = next(c for c in TC.PSEUDO if c.flags['cap'] == 'mid' and c.flags['nms'])
    inp = K.pseudo_inputs(c)
    ref = K.pseudo_ref(inp)
    ok = dict(lab_cat=ref['lab_cat'], box_cat=ref['box_cat'], lab_off=ref['off'], box_off=ref['off'], hist=ref['hist'])
    assert max(K.check_pseudo(ok, ref).values()) == 0
    # one event kept that overlap removal should drop: clip 2 keeps two of its class-0 events
    keep2 = K.pseudo_ref(dict(inp, cap=1 << 30))
    o2 = int(keep2['off'][2]) + 1
    lab = np.insert(keep2['lab_cat'], o2, 0)[:inp['cap']]
    box = np.insert(keep2['box_cat'], o2, inp['boxes'][2, 0], axis=0)[:inp['cap']]
    off = keep2['off'].copy()
    off[3:] += 1
    r = K.check_pseudo(dict(ok, lab_cat=lab, box_cat=box, lab_off=np.minimum(off, inp['cap']), box_off=np.minimum(off, inp['cap']),
                            hist=ref['hist'] + (np.arange(c.shape['C']) == 0)), ref)
    assert r['lab_off'] == float('inf') and r['counter'] == float('inf') and r['box_cat'] == float('inf')
    # an offset not clamped at cap
    assert keep2['off'][-1] > inp['cap']
    r = K.check_pseudo(dict(ok, lab_off=keep2['off']), ref)
    assert r['lab_off'] == float('inf') and r['box_off'] == 0


# ------------------------------------------------------------------------------------------------ feature loss, sum, scale, guards
@pytest.mark.parametrize('c', TC.FEATURE, ids=_ids(TC.FEATURE))
def test_feature_restatement_passes(c):
    inp = K.feature_inputs(c)
    ref = K.feature_ref(inp)
    f32 = K.feature_ref(inp, torch.float32)
    _note('feature', K.check_feature(f32, ref))
    i = np.unravel_index(np.abs(f32['dpred']).argmax(), f32['dpred'].shape)[:3]
    if c.flags['zero'] == 'pred':
        assert np.abs(ref['dpred'][inp['layer_of'][0], 0, 0]).max() > 1e10 and ref['rowloss'][0, 0, 0] * float(inp['num_boxes']) == 1.0
        i = (inp['layer_of'][1], 0, int(np.nonzero(inp['wbox'][1, 0] > 0)[0][0]))      # an ordinary live row beside the 1e12 one
    if c.flags['zero'] == 'target':
        # the row that points at the zero-norm target: |s / |s| - 0|^2 = 1 whatever s is, so its gradient is zero up to rounding and
        # faces the absolute 1e-6 alone
        t = (inp['layer_of'][1], 1, 1)
        assert ref['rowloss'][1, 1, 1] * float(inp['num_boxes']) == 1.0 and np.abs(ref['dpred'][t]).max() < 1e-12
        bad = dict(f32, dpred=f32['dpred'].copy())
        bad['dpred'][t + (3,)] = 1e-5
        assert K.check_feature(bad, ref)['dpred'] > 1
    bad = dict(f32, dpred=f32['dpred'].copy())
    bad['dpred'][i] *= 1 + 1e-3
    assert K.check_feature(bad, ref)['dpred'] > 1
    dead = np.nonzero(np.abs(ref['dpred']).max(-1) == 0)
    if len(dead[0]):                                                                    # a row that must be zero holds 1e-5
        bad = dict(f32, dpred=f32['dpred'].copy())
        bad['dpred'][dead[0][0], dead[1][0], dead[2][0], 0] = 1e-5
        assert K.check_feature(bad, ref)['dpred'] > 1
    bad = dict(f32, rowloss=f32['rowloss'].copy())
    j = np.unravel_index(np.abs(ref['rowloss']).argmax(), ref['rowloss'].shape)
    bad['rowloss'][j] *= 1 + 1e-4                                                       # a row loss wrong by 1e-4 of itself
    assert K.check_feature(bad, ref)['rowloss'] > 1


def test_sum_and_scale_restatements_pass():
    for n in TC.SUM_N:
        x = K.sum_input(n)
        RATIOS['sum_f32'] = max(RATIOS['sum_f32'], K.check_sum(np.float32(x.sum()) if n else np.float32(0), x))
        assert K.check_sum(np.float32(x.sum()) if n else np.float32(0), x) <= 1
        if n > 1:
            assert K.check_sum(np.float32(x[:-1].sum()), x) > 1              # the last element left out
    for c in TC.SCALE:
        inp = K.scale_inputs(c)
        r = K.check_scale(K.scale_ref(inp, np.float32), inp)
        RATIOS['scale_layers'] = max(RATIOS['scale_layers'], r)
        assert r <= 1, (c.name, r)
        if inp['idx'] is not None:
            assert K.check_scale(K.scale_ref(dict(inp, idx=None)), inp) > 1   # the permutation ignored


def test_guard_check_sees_one_byte():
    a = K.Arena()
    o1 = a.add('x', 40)
    o2 = a.add('y', 7)
    assert o1 % 16 == 0 and o2 % 16 == 0 and o2 - (o1 + 10) >= K.GUARD and a.words - (o2 + 2) >= K.GUARD
    before = np.full(4 * a.words, 0x5a, np.uint8)
    after = before.copy()
    after[4 * o1:4 * o1 + 40] = 1
    after[4 * o2:4 * o2 + 7] = 2
    assert K.guard_check(before, after, a.regions()) is None
    for byte in (4 * o1 - 1, 4 * o1 + 40, 4 * o2 + 7, 0, 4 * a.words - 1):
        bad = after.copy()
        bad[byte] ^= 1
        assert K.guard_check(before, bad, a.regions()) == byte
    assert K.guard_check(before, after, a.regions(only=('x',))) == 4 * o2
