"""CPU: the checker of tests/slab_check.py tried on torch emulations of the slab kernels' rounding decisions (csrc/enc_slab.hip,
csrc/heads_slab.hip): the honest emulation passes every bound and every exact mask check at every row of tests/slab_cases.py, and each
planted numerics-only fault fails."""
import pytest
import torch

import slab_cases as SC
import slab_check as K

_CACHE = {}


def _enc(c):
    if c['name'] not in _CACHE:
        t = K.enc_inputs(c)
        _CACHE[c['name']] = (t, K.emulate_enc(c, t))
    return _CACHE[c['name']]


def _heads(c):
    if c['name'] not in _CACHE:
        t = K.heads_inputs(c)
        _CACHE[c['name']] = (t, K.emulate_heads(c, t))
    return _CACHE[c['name']]


def test_the_tables_cover_what_they_claim():
    enc, hd = SC.ENC, SC.HEADS
    assert len(set(c['name'] for c in enc)) == len(enc) and len(set(c['name'] for c in hd)) == len(hd)
    assert set((c['B'], c['S']) for c in enc) >= {(1, 1), (2, 31), (1, 32), (3, 33), (2, 64), (2, 97), (1, 127), (2, 128)}
    for FF in (512, 1024, 1536, 2048):
        rows = [c for c in enc if c['FF'] == FF]
        assert any(c['S'] % 32 for c in rows) and any(c['S'] >= 32 for c in rows), FF      # a tail slab and a full slab
    assert set(c['p'] for c in enc) == {0.0, 0.1} and set(c['kind'] for c in enc) == {'steps', 'mean100'}
    assert set(c['kpm'] for c in enc) == {None, 'tail', 'scattered', 'key0', 'single', 'differ'}
    for c in enc:
        pat = K.kpm_pattern(c['kpm'], c['B'], c['S'])
        if pat is None:
            continue
        assert all(not all(r) for r in pat), c['name']
        if c['kpm'] == 'tail':                                  # the padded run starts in one 32-key tile and ends in the next
            assert all(r.index(True) // 32 < (c['S'] - 1) // 32 and r[-1] for r in pat), c['name']
        if c['kpm'] == 'single':
            assert sum(not x for x in pat[0]) == 1
        if c['kpm'] == 'differ':
            assert pat[0] != pat[1]
        if c['kpm'] == 'key0':
            assert all(r[0] for r in pat)
    assert set((c['L'], c['B'], c['Qp']) for c in hd) == {(1, 1, 1), (1, 1, 31), (1, 1, 32), (1, 1, 33), (1, 2, 32), (1, 2, 31), (2, 3, 11), (3, 2, 21)}
    assert set((c['C1'], c['CA']) for c in hd) == {(1, 0), (11, 10), (16, 16), (11, 0), (16, 1)}
    assert any(c['CA'] and not c['g_at'] for c in hd)
    at = set(r % 32 for c in hd if c['CA'] for r in K.at_rows(c['L'], c['B'], c['Qp']))
    assert {0, 31} <= at and any(0 < r < 31 for r in at), at


@pytest.mark.parametrize('c', SC.ENC, ids=[c['name'] for c in SC.ENC])
def test_emulated_encoder_kernels_pass_every_bound(c):
    t, o = _enc(c)
    r = K.check_enc_all(c, t, o)
    # a bf16 output's own rounding sits at 0.5; nothing of an honest emulation comes near its bound
    assert 0.0 < max(r.values()) <= 0.8, r


@pytest.mark.parametrize('c', SC.HEADS, ids=[c['name'] for c in SC.HEADS])
def test_emulated_heads_kernels_pass_every_bound(c):
    t, o = _heads(c)
    r = K.check_heads_all(c, t, o)
    assert 0.0 < max(r.values()) <= 0.8, r


def _rows_for(fault):
    """the table rows at which a fault can show"""
    enc = SC.ENC
    return {'tail_row': [c for c in enc if c['S'] % 32 and c['S'] > 1],
            'pos_v': enc,
            'hid_idx256': [c for c in enc if c['p'] > 0 and c['B'] * c['S'] > 1],      # (row 0's indices are f under either pitch)
            'chunk_c2': [c for c in enc if c['FF'] >= 1536],
            'res_x': enc,
            'attn_nohead': [c for c in enc if c['p'] > 0 and c['S'] > 1],
            'bwd_mask_seed': [c for c in enc if c['p'] > 0],
            'ln_part_shift': [c for c in enc if c['B'] * ((c['S'] + 31) // 32) > 1]}[fault]


@pytest.mark.parametrize('fault', K.FAULTS_ENC)
def test_planted_encoder_faults_fail_the_checker(fault):
    rows = _rows_for(fault)
    assert len(rows) >= 3, fault
    if fault == 'chunk_c2':
        assert set(c['FF'] for c in rows) == {1536, 2048}
    for c in rows:
        t, _ = _enc(c)
        with pytest.raises(AssertionError, match='over the bound|must be exact|keep decisions differ'):
            K.check_enc_all(c, t, K.emulate_enc(c, t, fault))


@pytest.mark.parametrize('fault', K.FAULTS_HEADS)
def test_planted_heads_faults_fail_the_checker(fault):
    rows = {'at_first_layer': [c for c in SC.HEADS if c['CA'] and c['L'] > 1],
            'cls_bias_32': [c for c in SC.HEADS if c['L'] * c['B'] * c['Qp'] > 32],
            'part_row31': [c for c in SC.HEADS if c['L'] * c['B'] * c['Qp'] >= 32]}[fault]
    assert len(rows) >= 2, fault
    for c in rows:
        t, _ = _heads(c)
        with pytest.raises(AssertionError, match='over the bound'):
            K.check_heads_all(c, t, K.emulate_heads(c, t, fault))


def test_a_single_wrong_element_fails():
    """one element of one 4-feature group off by two bf16 ulps; one dropped element of x2 that is not x1; one non-zero h under a zero
    keep bit: each is an assertion, however small the value"""
    c = next(c for c in SC.ENC if c['S'] == 33 and c['p'] > 0)
    t, o = _enc(c)
    m = K.enc_masks(c, t, t['x'].device)
    bad = dict(o, qk=o['qk'].clone())
    bad['qk'][40, 7] *= 1 + 2.0 ** -6
    with pytest.raises(AssertionError, match='over the bound'):
        K.check_enc_qkv(c, t, bad)
    i, j = (~m['f']).nonzero()[3].tolist()
    bad = dict(o, x2=o['x2'].clone())
    bad['x2'][i, j] = bad['x2'][i, j] * (1 + 2.0 ** -7) if bad['x2'][i, j] != 0 else 2.0 ** -20      # the next bf16 value
    with pytest.raises(AssertionError, match='must be exact'):
        K.check_enc_attn_ffn(c, t, bad, m)
    i, j = (~m['h']).nonzero()[5].tolist()
    bad = dict(o, h=o['h'].clone())
    bad['h'][i, j] = 2.0 ** -100
    with pytest.raises(AssertionError, match='over the bound|must be exact'):
        K.check_enc_attn_ffn(c, t, bad, m)
