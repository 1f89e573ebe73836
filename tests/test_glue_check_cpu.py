"""CPU: the checker of tests/test_glue_envelope_gpu.py checked without a GPU (tests/glue_check.py, rows in tests/glue_cases.py).

* every table is well-formed and reaches the edge it names: thread, block, chunk counts and LDS bytes are computed from the rows;
* every row's inputs are seeded (two calls give the same bytes) and finite (the cast rows' listed specials aside);
* the np.float32 restatement of every kernel passes its own checker on every row; the largest ratios of the bounded kernels are
  printed (-s);
* every injected fault of glue_check.FAULTS fails at least one row of the kernel it applies to;
* the bf16x3 split's subtraction x - bf16(x) is exact in f32 (1e5 samples over ten decades and more), and the kernel's nearest-index
  formula of mask_resize agrees with F.interpolate for the seven sizes.
"""
import collections

import numpy as np
import pytest
import torch

import glue_cases as GC
import glue_check as K

RATIOS = collections.defaultdict(float)


@pytest.fixture(scope='module', autouse=True)
def _table():
    yield
    if RATIOS:
        print('\nlargest error / bound ratio of the np.float32 restatements:')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')


def test_tables_are_well_formed():
    assert set(GC.CASES) == set(K.KERNELS)
    names = [c['name'] for rows in GC.CASES.values() for c in rows]
    assert len(names) == len(set(names))
    for key, rows in GC.CASES.items():
        assert rows, key
        for c in rows:
            assert 'dt' not in c or c['dt'] in GC.DTS


def test_elementwise_rows_reach_their_block_edges():
    assert [GC.nblk(n) for n in GC.N_EDGE] == [1, 1, 1, 2, 3]
    assert [GC.nblk(n // 8) for n in GC.N8_EDGE] == [1, 1, 1, 2] and [n // 8 for n in GC.N8_EDGE] == [1, 255, 256, 257]
    for key, field in (('add', 'cols'), ('cast', 'n'), ('relu_mask', 'n'), ('sigmoid_grad', 'n')):
        ns = {c[field] if key != 'add' else c['rows'] * c['cols'] for c in GC.CASES[key]}
        assert set(GC.N_EDGE) <= ns and 0 in ns, key
    assert {(c['rows'], c['cols'], c['b_mod']) for c in GC.ADD} >= {(13, 24, 5), (1, 256, 0), (37, 7, 37), (9, 40, 1)}
    assert {(c['src'], c['dst']) for c in GC.CAST} == {(a, b) for a in GC.DTS for b in GC.DTS}
    assert {(c['k'], c['n']) for c in GC.ADD_N if c['via'] == 'c'} >= {(k, n) for k in (1, 2, 3, 8) for n in GC.N8_EDGE}
    assert any(c['k'] == 9 and c['via'] == 'ops' for c in GC.ADD_N) and all(c['k'] <= 8 for c in GC.ADD_N if c['via'] == 'c')
    assert {c['p'] for c in GC.DROPOUT_GRAD} == {0.0, 0.1, 0.5} and {c['seed'] for c in GC.DROPOUT_GRAD} == {'val', 'ptr', 'both'}
    assert {c['n'] for c in GC.GELU} == {0} | set(GC.N8_EDGE) and {c['p'] for c in GC.GELU} == {0.0, 0.1}
    for key in ('add', 'cast', 'relu_mask', 'sigmoid_grad', 'add_n', 'dropout_grad', 'gelu', 'avgpool', 'mask_resize'):
        k = K.KERNELS[key]                                   # an empty row per entry point that can be handed an empty tensor
        assert any(all(f.span == 0 for f in k.frames(c, k.make(c)).values()) for c in GC.CASES[key]), key


def test_copy_and_split_rows_reach_their_job_edges():
    assert [len(c['jobs']) for c in GC.COPY2D] == [1, 3, 8, 9] and GC.COPY2D[-1]['via'] == 'ops'
    jobs = [j for c in GC.COPY2D for j in c['jobs']]
    assert {j[1] for j in jobs} >= {4, 12, 1024, 1028} and {j[0] for j in jobs} == {1, 3, 70}
    assert {j[0] * j[1] // 4 for j in jobs} >= {255, 256, 257}
    assert all(j[1] % 4 == 0 for j in jobs)
    for c in GC.COPY2D[1:]:                                  # a one-block job followed by a many-block one
        b = [GC.copy_blocks(j) for j in c['jobs']]
        assert any(b[i] == 1 and b[i + 1] > 8 for i in range(len(b) - 1)), c['name']
    assert sorted({len(c['jobs']) for c in GC.SPLIT3}) == [1, 3, 8]
    sj = [j for c in GC.SPLIT3 for j in c['jobs']]
    assert {j[:2] for j in sj} == {(1, 4), (3, 260), (5, 1024), (7, 148)} and {j[2] for j in sj} == {0, 12} and {j[3] for j in sj} == {0, 1}
    assert all(j[1] % 4 == 0 and (j[1] + j[2]) % 4 == 0 for j in sj)
    assert {GC.split_blocks(j) for j in sj} >= {1, 2, 5}     # (7, 148): 259 vectors, a second block of three


def test_dec_in_rows_reach_their_edges():
    rows = {c['B'] * c['Q'] for c in GC.DEC_IN}
    assert min(rows) < 8 and any(r % 8 for r in rows) and max(rows) > 8          # eight rows per block
    assert any((c['Q'] + c['qpp'] - 1) // c['qpp'] == c['P'] and c['Q'] % c['qpp'] == 1 and c['qpp'] > 1 for c in GC.DEC_IN)
    assert all((c['Q'] + c['qpp'] - 1) // c['qpp'] <= c['P'] and c['D'] % 8 == 0 for c in GC.DEC_IN)
    assert {(c['mode'], c['ratio']) for c in GC.DEC_IN} == {('eval', 0.0), ('given', 0.0), ('drawn', 0.0), ('drawn', 0.3), ('drawn', 1.0)}
    Bs = {c['B'] for c in GC.DEC_IN_BWD}
    assert Bs == {1, 2, 3, 4, 5, 9, 33, 37}
    per = {B: (B + 3) // 4 for B in Bs}
    assert any(p >= 8 and p % 8 for p in per.values()) and any(p == 8 or p == 9 for p in per.values())       # the unroll and its tail
    assert any(B < 4 for B in Bs)                            # empty clip groups
    assert {4 * c['D'] for c in GC.DEC_IN_BWD} == {256, 512, 1024} and all(c['D'] % 64 == 0 for c in GC.DEC_IN_BWD)


def test_reduction_and_pooling_rows_reach_their_edges():
    assert {c['rows'] for c in GC.COLSUM} >= {1, 3, 4, 5, 255, 256, 257, 513, 65537} and {c['cols'] for c in GC.COLSUM} >= {1, 63, 64, 65, 130}
    assert GC.colsum_chunks(256) == 1 and GC.colsum_chunks(257) == 2 and GC.colsum_chunks(65537) == 256
    assert GC.colsum_last_chunk_rows(65537) == 2
    assert any(c['view'] for c in GC.COLSUM) and any(c['in_f32'] and c['dt'] == 'bf16' for c in GC.COLSUM)
    assert {c['P'] for c in GC.AVGPOOL} >= {1, 3, 4, 5, 32}
    assert {c['C'] for c in GC.AVGPOOL if GC.avgpool_kernel(c) == 'vec8'} == {8, 688, 2048}
    assert {c['C'] for c in GC.AVGPOOL if GC.avgpool_kernel(c) == 'scalar'} == {4, 2044, 688}
    assert any(c['B'] * c['C'] // 8 == 258 for c in GC.AVGPOOL)
    hw = {(c['H'], c['W']) for c in GC.MAXPOOL}
    assert {h for h, w in hw} >= {1, 2, 3, 4, 5} and {w for h, w in hw} >= {1, 2, 3, 4, 5}
    assert {(h % 2, w % 2) for h, w in hw} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    big = [c for c in GC.MAXPOOL if (c['B'], c['H'], c['W'], c['C']) == (2, 5, 33, 128)]
    assert len(big) == 2 and all(GC.maxpool_blocks(c) >= 2 for c in big)
    assert all(c['C'] % 8 == 0 for c in GC.MAXPOOL)


def test_layout_and_skinny_rows_reach_their_edges():
    assert len(GC.MASK_RESIZE) == 8 and len(GC.POSENC) == 4 * 4 * 2
    assert all(c['D'] % 8 == 0 for c in GC.POSENC)
    assert {c['W'] for c in GC.STEM_IM2COL} == {20, 33, 64, 2042} and GC.stem_lds(2042) == 57344 <= 64 * 1024
    assert any(((c['W'] - 1) // 2 + 1) % 16 == 1 for c in GC.STEM_IM2COL)         # a column block that holds one pixel
    assert {c['M'] for c in GC.SKINNY_FWD} == set(GC.SK_M) and {(c['N'], c['K']) for c in GC.SKINNY_FWD} == set(GC.SK_NK)
    for N, K_ in GC.SK_NK:
        for dt in GC.DTS:
            assert {(c['bias'], c['act'], c['out_f32']) for c in GC.SKINNY_FWD if (c['N'], c['K'], c['dt']) == (N, K_, dt)} == set(GC.SK_OPTS)
            assert {c['M'] for c in GC.SKINNY_FWD if (c['N'], c['K'], c['dt']) == (N, K_, dt)} == set(GC.SK_M)
    assert GC.skinny_fwd_lds(16, 256) <= 64 * 1024 < GC.skinny_fwd_lds(16, 512) == 66048 and GC.skinny_fwd_lds(16, 1024) == 131584 <= 160 * 1024
    assert all(c['K'] % 4 == 0 and c['N'] <= 16 for c in GC.SKINNY_FWD)
    assert any(c['M'] * c['K'] // 8 > 256 and c['K'] == 64 for c in GC.SKINNY_DGRAD)
    assert max(GC.skinny_dgrad_lds(c['N'], c['K']) for c in GC.SKINNY_DGRAD) == 64 * 1024
    assert any(c['mask'] for c in GC.SKINNY_DGRAD) and any(c['acc'] for c in GC.SKINNY_DGRAD)
    assert {c['M'] for c in GC.SKINNY_WGRAD} == {1, 15, 16, 17, 33, 1000, 16384}
    assert GC.skinny_wgrad_lds(16384) == 64 * 1024 < GC.skinny_wgrad_lds(16385)
    assert any(c['deferred'] for c in GC.SKINNY_WGRAD) and {c['db'] for c in GC.SKINNY_WGRAD} == {0, 1}
    assert all(c['K'] % 64 == 0 for c in GC.SKINNY_WGRAD + GC.SKINNY_DGRAD)


@pytest.mark.parametrize('key', sorted(GC.CASES))
def test_inputs_are_seeded_and_finite(key):
    k = K.KERNELS[key]
    for c in GC.CASES[key]:
        a, b = k.make(c), k.make(c)
        assert a.keys() == b.keys()
        for n in a:
            assert a[n].dtype == b[n].dtype and np.array_equal(K.bits(a[n]), K.bits(b[n])), (c['name'], n)
            if key != 'cast' and a[n].dtype == np.float32:
                assert np.isfinite(a[n]).all(), (c['name'], n)
            if key != 'cast' and a[n].dtype == np.uint16:
                assert np.isfinite(K.from_bf16(a[n])).all(), (c['name'], n)


@pytest.mark.parametrize('key', sorted(GC.CASES))
def test_restatement_passes_its_own_checker(key):
    for c in GC.CASES[key]:
        for name, r in K.restated(key, c).items():
            RATIOS[K.ratio_key(name, c)] = max(RATIOS[K.ratio_key(name, c)], r)
            assert name.startswith('k:') or r <= 1.0


@pytest.mark.parametrize('key,fault', K.FAULTS, ids=[f'{k}-{f}' for k, f in K.FAULTS])
def test_injected_fault_fails(key, fault):
    assert fault in K.KERNELS[key].faults or fault in ('last_vector', 'past_n')
    failed = []
    for c in GC.CASES[key]:
        try:
            K.restated(key, c, fault)
        except AssertionError:
            failed.append(c['name'])
    assert failed, f'{fault} passed every row of {key}'


def test_frame_sees_a_write_in_a_row_gap_and_in_either_guard():
    for where in ('front', 'gap', 'back'):
        f = K.Frame('bf16', 3, 5, 9)
        f.region()[:] = 0
        f.check_guard(f.buf, 'clean')
        f.buf[{'front': f.off - 1, 'gap': f.off + 6, 'back': f.off + f.span}[where]] = 0
        with pytest.raises(AssertionError):
            f.check_guard(f.buf, where)
    f = K.Frame('f32', 2, 4)
    f.region()[0] = 1
    with pytest.raises(AssertionError):
        f.check_finite(f.buf, 'row 1 unwritten')
    assert K.Frame('u8', 0, 7).span == 0 and K.GUARD >= 32


def test_split_subtraction_is_exact_in_f32():
    r = np.random.default_rng(5)
    x = (r.standard_normal(100000) * 10.0 ** r.uniform(-12, 12, 100000)).astype(np.float32)
    hi = K.from_bf16(K.to_bf16(x))
    assert np.array_equal((x - hi).astype(np.float64), x.astype(np.float64) - hi.astype(np.float64))
    h2, lo = K.split_hi_lo(x)
    err = np.abs(x.astype(np.float64) - K.from_bf16(h2) - K.from_bf16(lo))
    assert (err <= 2.0 ** -16 * np.abs(x) + 2.0 ** -134).all()


def test_bf16_rounding_ties_to_even():
    sp = K.cast_specials()
    got = K.to_bf16(sp[:4])
    assert got.tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82]      # low half 0x8000: down under an even upper half, up under an odd one
    assert K.to_bf16(sp[9:10])[0] == 0x7F80                      # the largest finite f32 rounds to inf
    assert K.to_bf16(sp[11:13]).tolist() == [0x3F80, 0x3F81]


def test_mask_resize_index_formula_agrees_with_interpolate():
    for c in GC.MASK_RESIZE:
        for n_in, n_out in ((c['Hin'], c['Hout']), (c['Win'], c['Wout'])):
            src = torch.arange(n_in).float()[None, None, :, None]
            ref = torch.nn.functional.interpolate(src, size=(n_out, 1))[0, 0, :, 0].long().numpy()
            assert np.array_equal(K.resize_index(n_in, n_out), ref), (n_in, n_out)


def test_keep_decisions_follow_the_seed_and_the_dense_index():
    k = K.KERNELS['dropout_grad']
    c = next(c for c in GC.DROPOUT_GRAD if c['p'] == 0.5 and c['rows'] == 5 and c['seed'] == 'both')
    keep = k.keep(c)
    assert 0.3 < keep.mean() < 0.7 and not np.array_equal(keep, k.keep(c, 'index_from_ld'))
    assert K.eff_seed('both') == (K.SEED + 0x00C0FFEE) & 0xffffffff and len({K.eff_seed(m) for m in ('val', 'ptr', 'both')}) == 3
    p0 = next(c for c in GC.DROPOUT_GRAD if c['p'] == 0.0 and c['rows'] == 5)
    assert k.keep(p0).all()
