"""CPU: the attention dispatch of every row of tests/attn_cases.py resolved on the host (sedt_attention_describe is host-only, like
sedt_igemm_splitk: fake pointer values carry the rows' alignment), and the checker of tests/attn_check.py tried on torch emulations of
the kernels' rounding decisions: they must pass at the table's shapes, and each planted numerics-only fault must fail."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import attn_cases as AC
import attn_check as K
from conftest import ROOT
from gemm_check import U_BF16


@pytest.fixture(scope='module')
def lib():
    from sound_event_detection_transformer_amd import _build, lib as L
    _build.build()
    L.load()
    return L


def _describe(L, c, backward):
    """the row's layout as pointer VALUES: every allocation on a 4 KiB boundary, views at the offsets the GPU test gives them"""
    lay, W = AC.layout_of(c), c['H'] * 32
    eb = lay['eb']
    q = 0x100000
    k = q + 256 * eb if lay['packed'] else 0x200000
    ldqk, ldv = (512, W) if lay['packed'] else (lay['ld_in'], lay['ld_in'])
    outs = [0x400000 + 0x100000 * n + AC.out_start(c, w) * eb for n, w in enumerate(('o', 'dq', 'dk', 'dv'))]
    buf = C.create_string_buffer(96)
    r = L.load().sedt_attention_describe(q, ldqk, k, ldqk, 0x300000, ldv, outs[0], lay['ld_out'], 0x380000, ldv, outs[1], lay['ld_out'],
                                         outs[2], lay['ld_out'], outs[3], lay['ld_out'], int(c['amask']), c['Lq'], c['Lk'], c['p'],
                                         L.BF16 if c['dt'] == 'bf16' else L.F32, backward, buf, 96)
    name = buf.value.decode()
    assert (r == 0) == (name != ''), (c['name'], r, name)
    return name


def test_every_row_resolves_to_the_instance_it_names(lib):
    for c in AC.ATTN:
        assert _describe(lib, c, 0) == c['fwd'], c['name']
        assert _describe(lib, c, 1) == c['bwd'], c['name']
        if c['bwd'] == '':
            assert b'LDS' in lib.load().sedt_last_error(), c['name']
    assert len(set(c['name'] for c in AC.ATTN)) == len(AC.ATTN) and len(set(c['name'] for c in AC.LN)) == len(AC.LN)


def test_the_table_reaches_all_76_instances_and_every_tile_edge():
    reached = set(c['fwd'] for c in AC.ATTN) | set(c['bwd'] for c in AC.ATTN if c['bwd'])
    assert reached == AC.all_instances(), (AC.all_instances() - reached, reached - AC.all_instances())
    lk = set(c['Lk'] for c in AC.ATTN if c['fwd'].startswith('attn_fwd_mfma'))
    assert lk >= {1, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256}, sorted(lk)
    lq = set(c['Lq'] for c in AC.ATTN if c['bwd'].startswith('attn_bwd_mfma'))
    assert lq >= {1, 11, 21, 32, 33, 64, 65, 96, 97, 127, 128}, sorted(lq)
    waves = set(min(4, max((c['Lq'] + 31) // 32, (c['Lk'] + 31) // 32)) for c in AC.ATTN if c['bwd'].startswith('attn_bwd_mfma'))
    assert waves == {1, 2, 3, 4}
    for dt in ('bf16', 'f32'):
        rows = [c for c in AC.ATTN if c['dt'] == dt]
        assert set(c['B'] for c in rows) == {1, 3, 5} and set(c['H'] for c in rows) == {8, 3, 1}
        assert set(c['kpm'] for c in rows) == {None, 'tail', 'one', 'tiles', 'mid'} and set(c['amask'] for c in rows) == {False, True}
        assert set(c['p'] for c in rows) == {0.0, 0.1, 0.5} and set(c['gain'] for c in rows) == {1, 3}
        assert set(c['layout'] for c in rows) == {'packed', 'stride', 'o_off'}
        assert any(c['bwd'] == '' and c['Lq'] == c['Lk'] == 512 for c in rows)
    for c in AC.ATTN:                                       # 'tiles' does empty a whole 32-key tile of some clip
        if c['kpm']:
            pat = AC.kpm_pattern(c['kpm'], c['B'], c['Lk'])
            assert all(not all(r) for r in pat)
            if c['kpm'] == 'tiles':
                assert any(all(r[t:t + 32]) for r in pat for t in range(0, c['Lk'] - 31, 32)), c['name']
    ln = AC.LN
    assert set(c['rows'] for c in ln) >= {1, 3, 4, 5, 2047, 2048, 2049, 8195} and set(c['D'] for c in ln) == {256, 512}
    assert set(c['kind'] for c in ln) == {'normal', 'steps', 'mean100', 'const'}
    for f in ('add', 'dy2', 'dres', 'dres2', 'drop'):
        assert set(c[f] for c in ln) == {False, True}, f


def test_misaligned_o_is_generic_only_for_the_kernels_that_vector_access_it(lib):
    """the alignment of o: the bf16 MFMA forward writes it element by element (stays), the bf16 MFMA backward and both f32 MFMA
    kernels move it as 16-byte vectors (generic); one element further (16 bytes) everything is back"""
    c = dict(next(c for c in AC.ATTN if c['name'] == 'bf16_o_off'))
    assert (_describe(lib, c, 0), _describe(lib, c, 1)) == ('attn_fwd_mfma_kernel<4, false>', 'attn_bwd_kernel<__bf16>')
    c['layout'] = 'packed'
    assert _describe(lib, c, 1) == 'attn_bwd_mfma_kernel<1, 4, false>'


def _emulate_and_check(c, fault=None, only=None):
    inp = K.case_inputs(c)
    bf = c['dt'] == 'bf16'
    u_out = U_BF16 if bf else 0.0
    up_f = U_BF16 if 'mfma_kernel' in c['fwd'] else 0.0
    up_b = U_BF16 if 'mfma_kernel' in c['bwd'] else 0.0
    am = None if inp['amask'] is None else inp['amask'].double()
    em = K.attention_emulate(inp['q'], inp['k'], inp['v'], inp['do'], inp['kpm'], am, inp['keep'], c['p'], up_f > 0, bf, fault, mfma_bwd=up_b > 0)
    rf = K.attention_fwd_ref(inp['q'], inp['k'], inp['v'], inp['kpm'], am, inp['keep'], c['p'], up_f, u_out)
    out = {}
    for n in ('o', 'lse'):
        if only is None or n in only:
            out[n] = K.check(em[n], rf[n], rf['bound_' + n], f"{c['name']} {n}")
    if only is None:
        rb = K.attention_bwd_ref(inp['q'], inp['k'], inp['v'], inp['do'], em['o'], em['lse'], inp['kpm'], am, inp['keep'], c['p'], up_b, u_out)
        for n in ('dq', 'dk', 'dv'):
            out[n] = K.check(em[n], rb[n], rb['bound_' + n], f"{c['name']} {n}")
    return out


def test_emulated_kernels_pass_the_checker_at_the_tables_shapes():
    worst = {}
    for c in AC.ATTN:
        if c['Lq'] * c['Lk'] > 300 * 300:
            continue                                         # (512, 512): only the forward exists; covered by (257, 257)
        for n, r in _emulate_and_check(c).items():
            key = (c['dt'], n)
            worst[key] = max(worst.get(key, 0.0), r)
    # a bf16 output's own rounding sits at 0.5; the f32 outputs stay clear of their bounds
    for (dt, n), r in worst.items():
        assert r <= (0.75 if dt == 'bf16' and n != 'lse' else 0.6), worst


FAULT_ROWS = ['bf16_q65_k97_am', 'bf16_enc_s124', 'bf16_dec_cross_q21_k127', 'f32_enc_s128', 'f32_dec_cross_q21_k124']


@pytest.mark.parametrize('fault', ['last_key', 'scale', 'kpm', 'heads'])
def test_planted_faults_fail_the_checker(fault):
    rows = [c for c in AC.ATTN if c['name'] in FAULT_ROWS]
    assert len(rows) >= 4
    for c in rows:
        assert c['kpm'] and c['B'] >= 3 and c['H'] >= 3
        _emulate_and_check(c, None, only=('o',))
        with pytest.raises(AssertionError, match='over the bound'):
            _emulate_and_check(c, fault, only=('o',))


def test_one_flipped_keep_bit_fails_the_probe_check():
    B, H, Lq, Lk, p, t = 2, 3, 43, 45, 0.5, 1
    keep = K.keep_mask(77, B, H, Lq, Lk, p)
    gen = torch.Generator().manual_seed(5)
    for kind in ('fwd', 'pd', 'passA', 'ds'):
        q, k, v, do = K.probe_inputs(kind, B, H, Lq, Lk, t, gen)
        keep_t = torch.from_numpy(keep)
        rf = K.attention_fwd_ref(q, k, v, None, None, keep_t, p, 0.0, 0.0)
        assert float(rf['P'].min()) >= 2.0 ** -20
        rb = dict(dPraw=do @ v.transpose(-1, -2))
        if kind in ('passA', 'ds'):
            assert 0.5 <= float(rb['dPraw'].abs().min()) and float(rb['dPraw'].abs().max()) <= 1.5
        for bf in (True, False):
            o_in = torch.zeros(B, H, Lq, 32, dtype=torch.float64) if kind in ('passA', 'ds') else None      # the dS probes: o = 0
            em = K.attention_emulate(q, k, v, do, None, None, keep_t, p, bf, bf, o_in=o_in)
            got = {'fwd': lambda: em['o'], 'pd': lambda: em['dv'].transpose(-1, -2), 'passA': lambda: em['dq'],
                   'ds': lambda: em['dk'].transpose(-1, -2)}[kind]()
            val, keep_blk = K.probe_expected(kind, rf, rb, keep, t, Lq, Lk)
            n = val.shape[-1] if kind in ('fwd', 'passA') else val.shape[-2]
            got = got[..., :n] if kind in ('fwd', 'passA') else got[..., :n, :]
            K.probe_check(kind, got, keep_blk, val, kind)
            flipped = keep_blk.copy()
            flipped[1, 2, 3, 4] ^= True
            with pytest.raises(AssertionError, match='keep decisions differ'):
                K.probe_check(kind, got, flipped, val, kind)
            with pytest.raises(AssertionError, match='zero reference'):
                K.probe_check(kind, got, keep_blk, val * (torch.arange(val.numel()).reshape(val.shape) != 7), kind)


def test_drop_threshold_rounds_like_the_header():
    """csrc/common.h: t = (double)p * 65536.0 + 0.5 on the C float p, truncated, saturating at 0xffff.  Worked by hand:
    p = 2^-16 -> 1.5 -> 1; 0.1f = 0.100000001490116 -> 6554.1 -> 6554; 0.5 -> 32768.5 -> 32768; 0.99999f -> 65535.84 -> 0xffff"""
    assert [K.drop_threshold(p) for p in (1.0 / 65536, 0.1, 0.5, 0.99999)] == [1, 6554, 32768, 0xffff]
    src = open(os.path.join(ROOT, 'sound_event_detection_transformer_amd', 'csrc', 'common.h')).read()
    body = re.search(r'uint32_t drop_threshold\(float p\) \{(.*?)\n\}', src, re.S).group(1)
    assert 'double t = (double)p * 65536.0 + 0.5;' in body and 'return t >= 65535.0 ? 0xffffU : (uint32_t)t;' in body, body
    # drop_keep: the low half of the hash word for even elements, the high half for odd ones; an element pair shares one word
    from noise_views_ref import rng32
    h = rng32(9, np.arange(4, dtype=np.uint64))
    k = K.drop_keep(9, np.arange(8, dtype=np.uint64), 0x8000)
    assert k.tolist() == [bool(((h[i // 2] >> (16 * (i & 1))) & 0xffff) >= 0x8000) for i in range(8)]
    assert abs(K.keep_mask(3, 2, 3, 21, 45, 0.1).mean() - 0.9) < 0.02 and K.inv_keep(0.5) == 2.0


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_layernorm_emulation_passes_and_a_planted_fault_fails(dt):
    bf = dt == 'bf16'
    u_out = U_BF16 if bf else 0.0
    td = torch.bfloat16 if bf else torch.float32
    worst = 0.0
    for D in (256, 512):
        for n in (1, 5, 2049, 8192):
            g = torch.Generator().manual_seed(n + D)
            for kind in ('normal', 'mean100', 'const'):
                if kind == 'mean100' and bf:
                    continue
                x = torch.randn(n, D, generator=g, dtype=torch.float64)
                x = 100 + 0.05 * x if kind == 'mean100' else (x[:, :1] * 3).expand(n, D).clone() if kind == 'const' else x
                x = x.to(td).double()
                gamma, beta = (1 + 0.5 * torch.randn(D, generator=g)).double(), torch.randn(D, generator=g).double()
                add, dy = torch.randn(n, D, generator=g).to(td).double(), torch.randn(n, D, generator=g).to(td).double()
                em = K.layernorm_emulate(x, gamma, beta, add, dy, bf)
                rf = K.layernorm_fwd_ref(x, gamma, beta, add, u_out)
                for f in ('y', 'y2', 'mean', 'rstd'):
                    worst = max(worst, K.check(em[f], rf[f], rf['bound_' + f], f'{kind} {n}x{D} {f}'))
                rb = K.layernorm_bwd_ref(dy, None, x, gamma, em['mean'], em['rstd'], None, None, u_out)
                for f in ('dx', 'dgamma', 'dbeta'):
                    worst = max(worst, K.check(em[f], rb[f], rb['bound_' + f], f'{kind} {n}x{D} {f}'))
                if kind == 'normal' and n == 5:
                    bad = dict(em, y=em['y'].roll(1, 1), mean=em['mean'] * (1 + 2.0 ** -12))         # a lane shifted; a mean a few ulps off
                    for f in ('y', 'mean'):
                        with pytest.raises(AssertionError, match='over the bound'):
                            K.check(bad[f], rf[f], rf['bound_' + f], f)
    assert 0.0 < worst <= 1.0, worst
