"""CPU: the launch form of every backbone convolution (ops.conv_form) against the record of tests/golden/g24_conv_forms.npz.

The record was made from the commit before the dispatch moved into one planning function, by driving ITS conv_fwd / conv_dgrad through
tests/conv_plan_cases.py: stand-in operands on fake addresses, launches recorded instead of issued, labels from
sedt_igemm_group_describe.  Held with ==:

* the entry points still choose the same form, build the grouped forms' argument blocks field for field, and hint a recording the same;
* ops.conv_form / ops.conv_hint / ops.conv_group_jobs, asked directly, say what the entry points do, with or without a recording on;
* the sweep itself reaches every form for every kind it can occur for, and around each envelope it holds, for every refusing clause, a
  case that differs from an accepted one in that clause alone and is refused.
"""
import json
import os

import numpy as np
import pytest

import conv_plan_cases as S


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import _build, lib as L, ops
    _build.build()
    L.load()
    return ops, L


@pytest.fixture(scope='module')
def record():
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g24_conv_forms.npz'))
    return [str(n) for n in rec['names']], [str(a) for a in rec['answers'][rec['index']]]


@pytest.fixture(scope='module')
def cases():
    return S.cases()


def test_entry_points_equal_the_record(env, record, cases):
    ops, L = env
    names, want = record
    assert [c['name'] for c in cases] == names
    got = [S.answer(ops, L, c) for c in cases]
    diff = [(n, w[:200], g[:200]) for n, w, g in zip(names, want, got) if w != g]
    assert not diff, '%d of %d cases moved, the first: %s' % (len(diff), len(want), diff[:3])
    assert ops.PROFILE is None and not ops._co['on'] and not L.GEMM_X3              # the sweep leaves the switches as it found them


@pytest.mark.parametrize('recording', [False, True])
def test_the_planner_says_what_the_entry_points_do(env, record, cases, recording):
    ops, L = env
    for c, want in zip(cases, record[1]):
        form, x3, hint, label, blocks = json.loads(want)
        with S.switches(ops, L, c):
            dtype, t, B, g, w, out, ep = S.operands(ops, c)
            ops.PROFILE = [] if recording else None                                 # (the plan does not read it)
            plan = ops.conv_form(c['kind'], dtype, t, g, w, out, ep)
            assert plan == (form, x3, S.SHARE[form]), c['name']
            seen = {}
            with S.recording_library(ops, L, seen):
                got = ops.conv_hint(c['kind'], plan, t, B, g, w, out, ep)
                assert (list(got) if isinstance(got, tuple) else got) == hint, c['name']
                if blocks:
                    jobs = ops.conv_group_jobs(form, c['kind'], t, B, g, w, out, ep, x3)
                    assert [S._block(a) for a in jobs] == blocks and S.group_label(L, jobs) == label is not None, c['name']
            assert ops.PROFILE == ([] if recording else None) and not seen              # nothing launched, nothing recorded
        if hint is not None and form != 'direct3x3':
            assert hint == ['group', label, S.SHARE[form]] and not x3, c['name']
        assert (hint == 'conv3x3_c64_kernel') == (form == 'direct3x3') and (hint is None) == (form == 'gemm' or x3), c['name']


def test_the_sweep_reaches_every_form_and_every_clause(record, cases):
    ans = {c['name']: json.loads(a) for c, a in zip(cases, record[1])}
    seen = {(c['kind'], ans[c['name']][0], ans[c['name']][1]) for c in cases}
    assert seen == {('fwd', 'direct3x3', False), ('fwd', 'dil_halves', False), ('fwd', 'dil_halves', True), ('fwd', 'gemm', False),
                    ('dgrad', 'direct3x3', False), ('dgrad', 's2_parity', False), ('dgrad', 's2_parity', True), ('dgrad', 'dil_halves', False),
                    ('dgrad', 'dil_halves', True), ('dgrad', 'gemm', False)}, seen
    # the backbone's own geometries reach the three special forms (not only the cases built around the envelopes)
    assert {ans[c['name']][0] for c in cases if c['base'] is None and c['expect'] is None} == {'direct3x3', 's2_parity', 'dil_halves', 'gemm'}
    edges = [c for c in cases if c['expect']]
    for c in edges:
        assert ans[c['name']][0] == c['expect'], c['name']
        if c['base']:                       # one clause away from an accepted case
            assert ans[c['base']][0] in ('direct3x3', 's2_parity', 'dil_halves'), c['name']
    refused = {c['name'] for c in edges if c['base'] and c['expect'] == 'gemm'}
    want = ['direct fwd bf16 t stride 72', 'direct fwd bf16 out stride 72', 'direct fwd bf16 Wi=8', 'direct fwd bf16 key alpha', 'direct fwd bf16 tile',
            'direct fwd bf16 sigmoid', 'direct fwd bf16 ldm', 'direct fwd bf16 mask+relu', 'direct dgrad bf16 ldm', 'direct dgrad bf16 mask+relu',
            'direct dgrad bf16 scale', 'direct dgrad bf16 bias', 'direct fwd bf16 switch', 'direct fwd f32',
            'parity dgrad bf16 Co % 64', 'parity dgrad bf16 Ci % 8', 'parity dgrad bf16 w ld', 'parity dgrad bf16 dy stride',
            'parity dgrad bf16 out stride', 'parity dgrad bf16 key scale', 'parity dgrad bf16 switch', 'parity dgrad bf16 co', 'parity fwd']
    for kind in ('fwd', 'dgrad'):
        want += ['halves %s bf16 %s' % (kind, q) for q in ('95 tiles', 'cout % 128', 'cin % 64', 'Wi != 2 d', 'w ld', 't stride', 'out stride',
                                                           'key tile', 'switch', 'co')]
        want += ['direct %s bf16 %s' % (kind, q) for q in ('Ci', 'Co', 'KH', 'KW', 'sh', 'sw', 'ph', 'pw', 'dh', 'dw')]
        want += ['halves %s bf16 %s' % (kind, q) for q in ('KH', 'KW', 'sh', 'sw', 'dw', 'ph', 'pw', 'Ho', 'Wo')]
    want += ['parity dgrad bf16 %s' % q for q in ('KH', 'KW', 'sh', 'sw', 'ph', 'pw', 'dh', 'dw')]
    for fam in ('parity dgrad', 'halves fwd', 'halves dgrad'):
        want += ['%s x3 %s' % (fam, q) for q in ('t 8 bytes off', 'bf16 res', 'bf16 t', 'bf16 out', 'X3_FAST', 'GEMM_X3')]
    want += ['parity dgrad x3 bf16 mask', 'halves dgrad x3 bf16 mask']
    assert set(want) <= refused, sorted(set(want) - refused)
    # the tile threshold from both sides, maps of one row, odd maps
    assert ans['halves fwd bf16 96 tiles ok'][0] == ans['halves dgrad bf16 96 tiles ok'][0] == 'dil_halves'
    special = [c for c in cases if ans[c['name']][0] != 'gemm']
    for form in ('direct3x3', 's2_parity', 'dil_halves'):
        assert any(c['geom'][0] == 1 for c in special if ans[c['name']][0] == form), form
    assert any(c['geom'][0] % 2 and c['geom'][1] % 2 for c in special if ans[c['name']][0] == 's2_parity')
    assert any(len(ans[c['name']][4]) == 2 for c in special if ans[c['name']][0] == 's2_parity')        # (one column: two parities are empty)
