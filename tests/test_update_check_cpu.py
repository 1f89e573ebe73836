"""CPU: the checker of tests/update_check.py tried on float32 numpy restatements of the clip / AdamW / EMA / gather kernels
(csrc/misc.hip): the honest restatement stays at or below HALF of every bound at every row of tests/update_cases.py - with two
summation orders for the norm, with and without an emulated multiply-add for the EMA - and each planted fault fails the checker on its
own."""
import numpy as np
import pytest

import update_cases as UC
import update_check as K

_CACHE = {}


def _row(case):
    if case['name'] not in _CACHE:
        lay = K.Layout(case)
        _CACHE[case['name']] = (lay, K.make_image(case, lay))
    return _CACHE[case['name']]


def _by_name(name):
    return next(c for c in UC.ALL if c['name'] == name)


def test_the_tables_cover_what_they_claim():
    names = [c['name'] for c in UC.ALL]
    assert len(set(names)) == len(names)
    full = _by_name('adamw_full_step1_clip')['chunks']
    assert set(ch['n'] for ch in full) == {1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4097, 65535, 65536}
    f32 = set(ch['off'] for ch in full if not ch['bf'])
    # each of p, g, m, v misaligned alone, all four at once, every offset 0 / 4 / 8 / 12 somewhere
    assert f32 >= {(0, 0, 0, 0), (4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 4, 0), (0, 0, 0, 12)} and any(all(o) for o in f32)
    assert set(x for o in f32 for x in o) == {0, 4, 8, 12}
    assert set(ch['off'][1] for ch in full if ch['bf']) == {0, 2, 8}
    hyp = set((ch['lr'], ch['wd']) for ch in full)
    assert len(set(lr for lr, _ in hyp)) == 3 and any(lr == 0 for lr, _ in hyp) and any(wd == 0 for _, wd in hyp)
    assert max(lr for lr, _ in hyp) == 3 * UC.LR
    for n in set(ch['n'] for ch in full):                       # every length meets every (lr, wd) pair
        assert len(set((ch['lr'], ch['wd']) for ch in full if ch['n'] == n)) >= 2
    assert set(c['step'] for c in UC.ADAMW) == {1, 2, 3, 10, 1000, 100000}
    assert any(c['max_norm'] is None for c in UC.ADAMW) and any(c['gscale'] == 0 and c['moments'] == 'zero' for c in UC.ADAMW)
    assert set(c['gscale'] for c in UC.ADAMW) == {0.0, 1e-6, 1.0} and set(c['moments'] for c in UC.ADAMW) == {'zero', 'nonzero'}
    sq = UC.SUMSQ[0]['chunks']
    assert set(ch['n'] >> 2 for ch in sq) >= {767, 768, 769, 1023, 1024, 1025}
    for n4 in (767, 768, 769, 1023, 1024, 1025):
        assert set(ch['n'] & 3 for ch in sq if ch['n'] >> 2 == n4) >= {0, 3}
    assert set((ch['off'][1], ch['bf']) for ch in sq) == {(0, False), (4, False), (8, False), (12, False), (0, True), (2, True), (8, True)}
    assert [c['decay'] for c in UC.EMA] == [0.0, 1.0, 0.999, 0.9996]
    assert set(ch['n'] for ch in UC.EMA[0]['chunks']) == set(UC.LEN)
    assert [c['mode'] for c in UC.GATHER] == [0, 1, 2, 3]
    for c in UC.GATHER:
        assert set(ch['n'] for ch in c['chunks']) == {1, 7, 8, 9, 56, 57, 63, 64, 65, 16383, 16384, 16385, 65535, 65536}
    for c in UC.ALL:
        assert all(1 <= ch['n'] <= 65536 for ch in c['chunks'])


def test_layout_guards_and_offsets():
    for c in UC.ALL:
        lay = K.Layout(c)
        spans = sorted((s - K.GUARD * es, s + (n + K.GUARD) * es) for s, n, es, _ in lay.slots.values())
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), c['name']          # guards never shared between slots
        for ci, ch in enumerate(c['chunks']):
            for f in K.fields(c):
                assert lay.addr((ci, f)) % 16 == ch['off'][K._OFF[f]]
    lay = K.Layout(UC.GATHER[2])
    img = lay.blank()
    assert np.all(np.isnan(lay.get(img, (0, 'p')))) and np.all(np.isnan(lay.get(img, (0, 'g'))))


def test_bf16_rounding_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38], np.float32)      # 1 + 2^-8 and 1 + 3 2^-8 are ties
    assert K.bf2f(K.f2bf(x)).tolist() == [1.0, 1.0, 1.015625, -1.0, float(K.bf2f(K.f2bf(x[4:]))[0])]
    assert K.bf2f(K.f2bf_trunc(x))[:3].tolist() == [1.0, 1.0, 1.0078125]
    import torch
    t = torch.randn(4096)
    assert np.array_equal(K.f2bf(t.numpy()), t.bfloat16().view(torch.int16).numpy().view(np.uint16))


@pytest.mark.parametrize('order', ['lanes', 'pairwise'])
@pytest.mark.parametrize('c', UC.ADAMW + UC.SUMSQ, ids=[c['name'] for c in UC.ADAMW + UC.SUMSQ])
def test_honest_norm_and_adamw_stay_below_half(c, order):
    lay, img = _row(c)
    r = K.check_row(c, lay, img, K.emulate(c, lay, img, order=order))
    assert r and max(r.values()) <= 0.5, r


@pytest.mark.parametrize('fma', [False, True])
@pytest.mark.parametrize('c', UC.EMA, ids=[c['name'] for c in UC.EMA])
def test_honest_ema_stays_below_half(c, fma):
    lay, img = _row(c)
    r = K.check_row(c, lay, img, K.emulate(c, lay, img, fma=fma))
    assert r and max(r.values()) <= 0.5, r


@pytest.mark.parametrize('c', UC.GATHER, ids=[c['name'] for c in UC.GATHER])
def test_honest_gather_is_exact(c):
    lay, img = _row(c)
    K.check_row(c, lay, img, K.emulate(c, lay, img))
    if c['mode'] & 2:                 # the table does hold ties: truncation and rounding disagree on them
        src = lay.get(img, (3, 'g'))
        assert np.any((src.view(np.uint32) & 0xffff) == 0x8000) and np.any(K.f2bf(src) != K.f2bf_trunc(src))


@pytest.mark.parametrize('order', ['lanes', 'pairwise'])
def test_honest_single_tensor_norm_stays_below_half(order):
    for n in (1, 2047, 2048, 2049, 300001):
        g = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        s = K._f32_sum(g * g, order)
        assert K.sumsq1_check(g, s, 0.0, 0, f'n={n}')['sumsq'] <= 0.5
        assert K.sumsq1_check(g, np.float32(3.0) + s, 3.0, 1, f'n={n}')['sumsq accumulate'] <= 0.5


# the rows at which each fault must show (a fault is tried on every one of them)
FAULT_ROWS = {
    'tail_unwritten': ['adamw_full_step1_clip', 'ema_decay0.999', 'gather_mode1', 'gather_mode2'],
    'past_n': ['adamw_full_step3_noclip', 'ema_decay0.9996', 'gather_mode0', 'gather_mode3'],
    # (p - B) decay differs from p decay - B by lr wd |B|: 1e-5 |B|, which the bias-correction term (9e-5 |B| at step 1) hides early on
    'wd_after': ['adamw_core_step10_clip', 'adamw_core_step1000_clip', 'adamw_core_step100000_clip'],
    'coef_unclamped': ['adamw_core_step2_below', 'adamw_core_step1_below_zero_moments'],
    'eps_inside': ['adamw_core_step2_below', 'adamw_full_step1_clip'],
    'step_minus_1': ['adamw_core_step1_clip', 'adamw_core_step2_clip', 'adamw_core_step3_clip', 'adamw_core_step10_clip'],
    'swap_mv': ['adamw_full_step3_noclip', 'adamw_core_step1000_clip'],
    'lr_next': ['adamw_full_step1_clip', 'adamw_core_step3_clip'],
    'bf16_wrong_half': ['adamw_full_step1_clip', 'adamw_core_step100000_clip'],
    'ema_swapped': ['ema_decay0.0', 'ema_decay1.0', 'ema_decay0.999', 'ema_decay0.9996'],
    'gather_trunc': ['gather_mode2', 'gather_mode3'],
    'gather_overwrite': ['gather_mode1', 'gather_mode3'],
    'sumsq_drop_tail': ['sumsq_full', 'sumsq_core_1e-6'],
}


def test_every_fault_has_rows():
    assert set(FAULT_ROWS) == set(K.FAULTS)


@pytest.mark.parametrize('fault,name', [(f, n) for f in K.FAULTS for n in FAULT_ROWS[f]])
def test_planted_fault_fails(fault, name):
    c = _by_name(name)
    lay, img = _row(c)
    bad = K.emulate(c, lay, img, fault=fault)
    with pytest.raises(AssertionError):
        K.check_row(c, lay, img, bad)
