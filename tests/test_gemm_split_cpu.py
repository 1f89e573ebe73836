"""CPU: the GEMM dispatcher's host-side rules over the envelope table of tests/test_gemm_envelope_gpu.py (tests/gemm_cases.py).

* Every row's kernel instance resolves on the host (sedt_igemm_describe launches nothing and reads only addresses): a retuned threshold
  that moves a row to another kernel fails here first, and the table has to be updated on purpose.
* The split-K rule (sedt_igemm_splitk) gives a factor between 1 and the number of K blocks for every weight gradient of the training
  step and of the table, and the table keeps the split cases that matter: factor 1, 2, an odd one, a multiple of 8, a split whose
  trailing slice gets no K block (the kernels must write zero partial tiles for it) and the <= 2-tile long-K form (up to 512 slices).
* The whole dispatch - status, instance and split factor of some 27 000 problems around every threshold (tests/gemm_dispatch_sweep.py) -
  equals the record of tests/golden/g22_gemm_dispatch.npz (tests/golden/make_golden_dispatch.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import gemm_cases as G


@pytest.fixture(scope='module')
def lib():
    from sound_event_detection_transformer_amd import _build, lib as L
    _build.build()
    L.load()
    return L


def _describe(L, a, code, grouped=0):
    buf = C.create_string_buffer(160)
    r = L.load().sedt_igemm_describe(C.byref(a), code, grouped, buf, 160)
    assert r == 0, L.load().sedt_last_error().decode()
    return buf.value.decode()


def _code(c):
    return {'bf16': 1, 'f32': 0}[c['mode']]


@pytest.mark.parametrize('case', [c for c in G.CASES if c['mode'] != 'x3'], ids=lambda c: c['name'])
def test_table_instance_resolves_on_host(lib, case):
    code = _code(case)
    a = G.fake_args(case, lib, code)
    if case['op'] == G.LINEAR and case['ep'].get('out_f32') and code == 1:
        a.f32ep = 1                                 # (ops.igemm asks for the f32 epilogue when the LDS-DMA family takes the problem)
        if not _describe(lib, a, code).startswith('igemm3'):
            a.f32ep = 0
    assert _describe(lib, a, code) == case['expect']


def test_group_instances_resolve_on_host(lib):
    for c in G.GROUP_WGRAD:
        assert _describe(lib, G.fake_args(c, lib, 1), 1, grouped=1) == c['expect'], c['name']
    for shapes, kw, expect in G.GROUP_LINEAR:
        arr = (lib.SedtIgemm * len(shapes))(*[G.fake_args(G.lin('g', M, N, K, None, **kw), lib, 1) for M, N, K in shapes])
        buf = C.create_string_buffer(160)
        assert lib.load().sedt_igemm_group_describe(arr, len(shapes), 1, buf, 160) == 0
        assert buf.value.decode() == expect, shapes


def _step_wgrad_shapes():
    """(Cout, taps * Cin, K) of every weight gradient of one training step at 64 clips of 500 x 64 (bench.py's default), read off the
    CPU oracle model with forward hooks at 2 clips and scaled"""
    import torch
    from oracle import sedt_oracle as O
    model = O.build_oracle_model(10, 10, 3, 3, True, True, True, dropout=0.0).eval()
    B, scale, shapes = 2, 32, set()

    def conv_hook(m, inp, out):
        shapes.add((m.out_channels, m.in_channels * m.kernel_size[0] * m.kernel_size[1], out.shape[0] * out.shape[2] * out.shape[3] * scale))

    def lin_hook(m, inp, out):
        shapes.add((m.out_features, m.in_features, inp[0].numel() // inp[0].shape[-1] * scale))

    def mha_hook(m, inp, out):
        q, k = inp[0], inp[1]
        E = m.embed_dim
        shapes.add((E, E, q.shape[0] * q.shape[1] * scale))
        shapes.add((2 * E, E, k.shape[0] * k.shape[1] * scale))

    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.register_forward_hook(conv_hook)
        elif isinstance(m, torch.nn.Linear):
            m.register_forward_hook(lin_hook)
        elif isinstance(m, O.MultiheadAttention):
            m.register_forward_hook(mha_hook)
    with torch.no_grad():
        model(torch.randn(B, 1, 500, 64, generator=torch.Generator().manual_seed(0)))
    return sorted(shapes)


def test_split_rule_over_step_and_table(lib):
    l = lib.load()
    step = _step_wgrad_shapes()
    assert len(step) >= 20, step                     # the ResNet body, the stem, the transformer's projections and FFN, the heads
    table = [(c['M'], c['N'], c['K'], _code(c)) for c in G.CASES + G.GROUP_WGRAD if c['op'] == G.WGRAD and c['mode'] != 'x3']
    for M, N, K, code in [(M, N, K, 1) for M, N, K in step] + [(M, N, K, 0) for M, N, K in step] + table:
        sk = l.sedt_igemm_splitk(M, N, K, code)
        nkb = (K + (63 if code == 1 else 31)) // (64 if code == 1 else 32)
        assert 1 <= sk <= nkb, (M, N, K, code, sk, nkb)
        if sk > 1:
            _, per, empty = G.split_plan(M, N, K, sk, 64 if code == 1 else 32)
            assert per * (sk - empty - 1) < nkb <= per * (sk - empty), (M, N, K, sk)      # every K block in exactly one slice


def test_table_keeps_the_split_edge_cases(lib):
    l = lib.load()
    factors, empty_lds, long_k = set(), [], []
    for c in G.CASES + G.GROUP_WGRAD:
        if c['op'] != G.WGRAD or c['mode'] != 'bf16':
            continue
        sk = l.sedt_igemm_splitk(c['M'], c['N'], c['K'], 1)
        factors.add(sk)
        _, _, empty = G.split_plan(c['M'], c['N'], c['K'], sk)
        if empty > 0 and c['expect'].startswith('wgrad'):
            empty_lds.append(c['name'])
        if G.out_tiles(c['M'], c['N']) <= 2 and sk > 64:
            long_k.append(c['name'])
    assert 1 in factors and 2 in factors, factors
    assert any(f > 2 and f % 2 for f in factors), factors
    assert any(f >= 8 and f % 8 == 0 for f in factors), factors
    assert empty_lds, 'no LDS-DMA wgrad case leaves an empty trailing split-K slice'
    assert long_k, 'no <= 2-tile long-K case'
    assert any(c['name'] in empty_lds for c in G.GROUP_WGRAD), 'the grouped wgrad launch has no empty-slice problem'


def test_dispatch_sweep_equals_the_record(lib):
    import gemm_dispatch_sweep as S
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_gemm_dispatch.npz'))
    want = [str(a) for a in rec['answers'][rec['index']]]
    got = S.answers(lib)
    # the sweep itself: large enough, almost all of it problems the library accepts, every instance of the envelope table in it
    assert len(got) >= 20000 and len(got) == len(want), (len(got), len(want))
    parts = [a.split('|')[:2] for a in want]
    refused = sum(any(not q.startswith('0:') for q in ps) for ps in parts)
    assert refused <= 0.02 * len(want), (refused, len(want))
    seen = {q.split(':', 1)[1] for ps in parts for q in ps}
    assert S.table_instances() <= seen, sorted(S.table_instances() - seen)
    # every status, label and split factor
    diff = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, '%d of %d problems moved, the first: %s' % (len(diff), len(want), diff[:5])
