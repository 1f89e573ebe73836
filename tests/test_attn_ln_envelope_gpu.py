"""GPU: the stand-alone attention and LayerNorm kernels (csrc/attn_mfma.hip, csrc/attn_f32_mfma.hip, csrc/norm_attn.hip) at their tile
edges, element by element against float64 (tests/attn_check.py: references, bounds and their derivation).

Attention.  Each row of tests/attn_cases.py names the kernel instance its forward and its backward must reach - all 76 instances of
sedt_attention_fwd / sedt_attention_bwd, tile counts on both sides of every 32-edge, 1 to 4 waves, the generic kernels by size, by
stride and by a misaligned o, and the refused backward.  Per row: the dispatch is asserted through sedt_attention_describe BEFORE the
launch (and again through the lib.launch_log() key the launch records); the outputs live inside NaN-filled buffers with a guard row
above and below and guard columns left and right, which must keep their bits; every output element must be finite and within its
bound; a second run must be bit-identical.  A refused call is asserted through describe and the raised RuntimeError.

Dropout.  test_keep_mask_* pin the numpy restatement of drop_keep to the device (ops.dropout_grad on ones) and then read each of the
four places that draw a keep decision - forward, backward pass A (drop_keep4, odd and even first index), backward pass B for Pd and for
dS (drop_keep_in) - out of the kernels, block by block, as the zero pattern of an output: exact, for all three kernel families.

LayerNorm.  f32 / bf16, D = 256 / 512, rows on both sides of the forward's 4-row workgroups and of the backward's 512-workgroup grid cap,
optional tensors present and absent, inputs with magnitude steps, mean 100 / std 0.05 and constant rows; dx_drop exact from the
kernel's own dx; the split parameter-gradient reduction (sedt_layernorm_bwd_final) bit-identical to the fused one; a misaligned view
refused without a launch.

Nothing here launches a call that is expected to be refused past its check, and nothing is skipped.

Largest error / bound ratio per kernel family and output measured on MI355X (printed at the end of the module with -s; every bound
held on the unmodified kernels):
  attn_fwd_mfma_kernel      o 0.46   lse 0.11          attn_bwd_mfma_kernel      dq 0.44  dk 0.46  dv 0.47
  attn_f32_fwd_kernel       o 0.078  lse 0.26          attn_f32_bwd_kernel       dq 0.17  dk 0.18  dv 0.30
  attn_fwd_kernel<__bf16>   o 0.49   lse 0.084         attn_bwd_kernel<__bf16>   dq 0.50  dk 0.50  dv 0.50
  attn_fwd_kernel<float>    o 0.039  lse 0.086         attn_bwd_kernel<float>    dq 0.080 dk 0.097 dv 0.16
  LayerNorm bf16 (256 / 512)  y, y2, dx 0.50 (the output's own rounding); mean 0.073 / 0.067; rstd 0.054 / 0.051; dgamma 0.20; dbeta 0.050 / 0.060
  LayerNorm f32  (256 / 512)  y 0.43 / 0.45; y2 0.44 / 0.46; mean 0.13 / 0.11; rstd 0.053 / 0.049; dx 0.88 / 0.86; dgamma 0.23; dbeta 0.18 / 0.15
The whole module (159 tests) runs in about 10 s.
"""
import ctypes as C
import time
import zlib
from collections import defaultdict

import numpy as np
import pytest
import torch

import attn_cases as AC
import attn_check as K
from gemm_check import U_BF16, nan_buffer, poison

pytestmark = pytest.mark.gpu

RATIOS = defaultdict(float)
T0 = [None]


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, ops
    assert torch.cuda.is_available()
    L.load()
    T0[0] = time.time()
    yield L, ops
    if RATIOS:
        print('\nlargest error / bound ratio per kernel family and output:')
        for k in sorted(RATIOS):
            print(f'  {k:44s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - T0[0]:.1f} s')


def _record(key, ratio):
    RATIOS[key] = max(RATIOS[key], ratio)


def _td(c):
    return torch.bfloat16 if c['dt'] == 'bf16' else torch.float32


GUARD = AC.GUARD


class Guarded(object):
    """an output [rows, W] inside a NaN-filled buffer: one guard row above and below, GUARD columns left, ld - W - GUARD right, the
    whole thing `off` elements into its allocation"""

    def __init__(self, rows, W, ld, off, dtype):
        assert ld >= W and rows >= 1
        self.left = AC.guard_left(W, ld)
        self.buf = nan_buffer(off + (rows + 2) * ld, dtype)
        self.full = self.buf[off:].view(rows + 2, ld)
        self.view = self.full[1:rows + 1, self.left:self.left + W]
        self.fill = self.bits().clone()
        inner = torch.zeros_like(self.fill, dtype=torch.bool)
        inner[off:].view(rows + 2, ld)[1:rows + 1, self.left:self.left + W] = True
        self.outer = ~inner

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.element_size() == 2 else torch.int32)

    def assert_guards(self, what):
        changed = (self.bits() != self.fill) & self.outer
        assert not bool(changed.any()), f'{what}: {int(changed.sum())} elements outside the output were written (first at element ' \
                                       f'{int(changed.nonzero()[0])} of the buffer)'


def _place(t, ld, dtype, col0=0, buf=None):
    """[rows, W] float64 -> device view with row stride ld (inside buf [*, ld] at column col0 when given)"""
    rows, W = t.shape
    if buf is None:
        buf = torch.zeros(rows, ld, device='cuda', dtype=dtype)
    v = buf[:rows, col0:col0 + W]
    v.copy_(t.to(dtype))
    return v


def _device_case(c, inp):
    """the row's operands as device views in its layout"""
    B, H, Lq, Lk = c['B'], c['H'], c['Lq'], c['Lk']
    lay, td, W = AC.layout_of(c), _td(c), c['H'] * 32
    q2, k2, v2, d2 = (K.rows(inp[n]) for n in ('q', 'k', 'v', 'do'))
    if lay['packed']:
        qk = torch.zeros(max(B * Lq, B * Lk), 512, device='cuda', dtype=td)
        q, k = _place(q2, 512, td, 0, qk), _place(k2, 512, td, 256, qk)
        v, do = _place(v2, W, td), _place(d2, W, td)
    else:
        q, k, v, do = (_place(t, lay['ld_in'], td) for t in (q2, k2, v2, d2))
    dev = dict(q=q, k=k, v=v, do=do, kpm=None, amask=None)
    if inp['kpm'] is not None:
        dev['kpm'] = inp['kpm'].to(torch.uint8).cuda()
    if inp['amask'] is not None:
        dev['amask'] = inp['amask'].cuda().contiguous()
    dev['seed_ptr'] = torch.from_numpy(np.array([inp['word']], np.uint32).view(np.int32)).cuda()
    return dev, lay


def _dt_code(L, c):
    return L.BF16 if c['dt'] == 'bf16' else L.F32


def _family(inst, c):
    return inst.split('<')[0] + ('[bf16]' if c['dt'] == 'bf16' and 'mfma' not in inst else '[f32]' if 'mfma' not in inst else '')


@pytest.mark.parametrize('c', AC.ATTN, ids=[c['name'] for c in AC.ATTN])
def test_attention_envelope(env, c):
    L, ops = env
    B, H, Lq, Lk, p = c['B'], c['H'], c['Lq'], c['Lk'], c['p']
    dt, td, W = _dt_code(L, c), _td(c), c['H'] * 32
    inp = K.case_inputs(c)
    dev, lay = _device_case(c, inp)
    u_out = U_BF16 if c['dt'] == 'bf16' else 0.0
    kw = dict(kpm=dev['kpm'], amask=dev['amask'], drop_p=p, seed=inp['seed'], seed_ptr=dev['seed_ptr'])

    # ---------------------------------------------------------------- forward
    poison(64)
    og = Guarded(B * Lq, W, lay['ld_out'], lay['o_off'], td)
    inst = ops.attention_instance(dt, dev['q'], dev['k'], dev['v'], og.view, Lq, Lk, dev['amask'], p)
    assert inst == c['fwd'], f"{c['name']}: the forward would run on {inst!r}, the row expects {c['fwd']!r} - not launched"
    with L.launch_log() as log:
        _, lse = ops.attention_fwd(dt, dev['q'], dev['k'], dev['v'], B, H, Lq, Lk, out=og.view, **kw)
    assert log['attention:' + c['fwd']] == 1 and log['attention_fwd'] == 1, dict(log)
    torch.cuda.synchronize()
    og.assert_guards(c['name'] + ' o')
    g64 = {n: inp[n].cuda() for n in ('q', 'k', 'v', 'do')}
    kpm64 = None if inp['kpm'] is None else inp['kpm'].cuda()
    am64 = None if inp['amask'] is None else inp['amask'].double().cuda()
    keep = inp['keep'].cuda()
    rf = K.attention_fwd_ref(g64['q'], g64['k'], g64['v'], kpm64, am64, keep, p, U_BF16 if 'mfma_kernel' in inst else 0.0, u_out)
    o_k = K.heads(og.view, B, H, Lq)
    fam = _family(inst, c)
    _record(fam + ' o', K.check(o_k, rf['o'], rf['bound_o'], c['name'] + ' o'))
    _record(fam + ' lse', K.check(lse, rf['lse'], rf['bound_lse'], c['name'] + ' lse'))
    og2 = Guarded(B * Lq, W, lay['ld_out'], lay['o_off'], td)
    _, lse2 = ops.attention_fwd(dt, dev['q'], dev['k'], dev['v'], B, H, Lq, Lk, out=og2.view, **kw)
    assert torch.equal(og2.bits(), og.bits()) and torch.equal(lse2.view(torch.int32), lse.view(torch.int32)), 'forward: second run differs'

    # ---------------------------------------------------------------- backward
    gq, gk, gv = (Guarded(B * n, W, lay['ld_out'], 0, td) for n in (Lq, Lk, Lk))
    binst = ops.attention_instance(dt, dev['q'], dev['k'], dev['v'], og.view, Lq, Lk, dev['amask'], p, dev['do'], gq.view, gk.view, gv.view)
    assert binst == c['bwd'], f"{c['name']}: the backward would run on {binst!r}, the row expects {c['bwd']!r} - not launched"
    bargs = (dt, dev['q'], dev['k'], dev['v'], og.view, dev['do'], lse, B, H, Lq, Lk)
    if c['bwd'] == '':
        with pytest.raises(RuntimeError, match='LDS'):
            ops.attention_bwd(*bargs, gq.view, gk.view, gv.view, **kw)
        for g_, n in ((gq, 'dq'), (gk, 'dk'), (gv, 'dv')):
            assert torch.equal(g_.bits(), g_.fill), f'{n}: a refused call wrote'
        return
    poison(64)
    with L.launch_log() as log:
        ops.attention_bwd(*bargs, gq.view, gk.view, gv.view, **kw)
    assert log['attention:' + c['bwd']] == 1 and log['attention_bwd'] == 1, dict(log)
    torch.cuda.synchronize()
    rb = K.attention_bwd_ref(g64['q'], g64['k'], g64['v'], g64['do'], o_k, lse.double(), kpm64, am64, keep, p,
                             U_BF16 if 'mfma_kernel' in binst else 0.0, u_out)
    fam = _family(binst, c)
    for g_, n, Ln in ((gq, 'dq', Lq), (gk, 'dk', Lk), (gv, 'dv', Lk)):
        g_.assert_guards(f"{c['name']} {n}")
        _record(f'{fam} {n}', K.check(K.heads(g_.view, B, H, Ln), rb[n], rb['bound_' + n], f"{c['name']} {n}"))
    hq, hk, hv = (Guarded(B * n, W, lay['ld_out'], 0, td) for n in (Lq, Lk, Lk))
    ops.attention_bwd(*bargs, hq.view, hk.view, hv.view, **kw)
    for a, b_, n in ((gq, hq, 'dq'), (gk, hk, 'dk'), (gv, hv, 'dv')):
        assert torch.equal(a.bits(), b_.bits()), f'backward: second run differs in {n}'


# ==================================================================================================== exact keep masks
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_keep_mask_restatement_matches_the_device(env, dt, p):
    """attn_check.drop_keep / drop_threshold against the device's drop_keep: ops.dropout_grad on ones, exact"""
    L, ops = env
    rows_, cols = 37, 77                                   # odd row length: both halves of a hash word start a row
    td = torch.float32 if dt == 'f32' else torch.bfloat16
    seed, word = 0x7fff1234, 0xfedcba98
    sp = torch.from_numpy(np.array([word], np.uint32).view(np.int32)).cuda()
    out = ops.dropout_grad(L.F32 if dt == 'f32' else L.BF16, torch.ones(rows_, cols, device='cuda', dtype=td), p, seed, sp)
    keep = K.drop_keep((seed + word) & 0xffffffff, np.arange(rows_ * cols, dtype=np.uint64), K.drop_threshold(p)).reshape(rows_, cols)
    want = torch.where(torch.from_numpy(keep), torch.tensor(K.inv_keep(p), dtype=torch.float32), torch.tensor(0.0)).to(td)
    assert torch.equal(out.cpu(), want)
    assert 0 < keep.mean() < 1


PROBE_FAMILIES = [('bf16', 'mfma'), ('f32', 'mfma'), ('bf16', 'generic'), ('f32', 'generic')]


@pytest.mark.parametrize('dt,path', PROBE_FAMILIES, ids=[f'{a}_{b}' for a, b in PROBE_FAMILIES])
@pytest.mark.parametrize('Lq,Lk,p', [(45, 77, 0.1), (21, 64, 0.5), (11, 11, 0.5), (70, 33, 0.1)])
def test_keep_mask_probes(env, dt, path, Lq, Lk, p):
    """each of the four keep draws read out of the kernels, one 32-wide block at a time (attn_check.probe_inputs), for every
    (b, h, i, j): B H = 15 so that clip and head enter the element index; odd and even Lk; Lq not a multiple of 32"""
    L, ops = env
    B, H, W = 5, 3, 96
    code, td = (L.BF16, torch.bfloat16) if dt == 'bf16' else (L.F32, torch.float32)
    ld = W if path == 'mfma' else W + (4 if dt == 'bf16' else 2)          # a row stride the MFMA kernels refuse -> generic
    seed, word = 0x1234abcd, 0xf0000001
    sp = torch.from_numpy(np.array([word], np.uint32).view(np.int32)).cuda()
    keep = K.keep_mask((seed + word) & 0xffffffff, B, H, Lq, Lk, p)
    keep_t = torch.from_numpy(keep)
    gen = torch.Generator().manual_seed(Lq * 1000 + Lk)
    kw = dict(drop_p=p, seed=seed, seed_ptr=sp)
    for kind in ('fwd', 'pd', 'passA', 'ds'):
        nblk = (Lk + 31) // 32 if kind in ('fwd', 'passA') else (Lq + 31) // 32
        for t in range(nblk):
            q, k, v, do = K.probe_inputs(kind, B, H, Lq, Lk, t, gen)
            qd, kd, vd, dd = (_place(K.rows(x), ld, td) for x in (q, k, v, do))
            od = torch.zeros(B * Lq, ld, device='cuda', dtype=td)[:, :W]
            inst = ops.attention_instance(code, qd, kd, vd, od, Lq, Lk, None, p)
            assert inst.startswith(('attn_fwd_kernel<', 'attn_bwd_kernel<')) == (path == 'generic'), inst
            _, lse = ops.attention_fwd(code, qd, kd, vd, B, H, Lq, Lk, out=od, **kw)
            rf = K.attention_fwd_ref(q, k, v, None, None, keep_t, p, 0.0, 0.0)
            assert float(rf['P'].min()) >= 2.0 ** -20
            if kind == 'fwd':
                got = K.heads(od, B, H, Lq)
            else:
                o_in = od if kind == 'pd' else torch.zeros_like(od)          # the dS probes: o = 0, so delta = 0
                dq, dk, dv = (torch.zeros(B * n, ld, device='cuda', dtype=td)[:, :W] for n in (Lq, Lk, Lk))
                inst = ops.attention_instance(code, qd, kd, vd, o_in, Lq, Lk, None, p, dd, dq, dk, dv)
                assert inst.startswith(('attn_fwd_kernel<', 'attn_bwd_kernel<')) == (path == 'generic'), inst
                ops.attention_bwd(code, qd, kd, vd, o_in, dd, lse, B, H, Lq, Lk, dq, dk, dv, **kw)
                got = {'pd': K.heads(dv, B, H, Lk).transpose(-1, -2), 'passA': K.heads(dq, B, H, Lq),
                       'ds': K.heads(dk, B, H, Lk).transpose(-1, -2)}[kind]
            rb = dict(dPraw=do @ v.transpose(-1, -2))
            if kind in ('passA', 'ds'):
                assert 0.5 <= float(rb['dPraw'].abs().min()) and float(rb['dPraw'].abs().max()) <= 1.5
            val, keep_blk = K.probe_expected(kind, rf, rb, keep, t, Lq, Lk)
            n = val.shape[-1] if kind in ('fwd', 'passA') else val.shape[-2]
            got = got[..., :n] if kind in ('fwd', 'passA') else got[..., :n, :]
            K.probe_check(kind, got, keep_blk, val, f'{dt} {path} Lq {Lq} Lk {Lk} p {p} block {t}')


# ==================================================================================================== LayerNorm
def _ln_inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    n, D = c['rows'], c['D']
    td = torch.bfloat16 if c['dt'] == 'bf16' else torch.float32
    x = torch.randn(n, D, generator=g, dtype=torch.float64)
    if c['kind'] == 'steps':
        x = x * (4.0 ** ((torch.arange(n) % 9) - 4).double())[:, None] + (torch.arange(n) % 5 - 2).double()[:, None]
    elif c['kind'] == 'mean100':
        x = 100.0 + 0.05 * x
    elif c['kind'] == 'const':
        x = (torch.randn(n, 1, generator=g, dtype=torch.float64) * 3).expand(n, D).clone()

    def rnd(t):
        return t.to(td).double()
    out = dict(x=rnd(x), gamma=(1.0 + 0.5 * torch.randn(D, generator=g)).float().double(), beta=torch.randn(D, generator=g).float().double(),
               dy=rnd(torch.randn(n, D, generator=g, dtype=torch.float64) * (2.0 ** ((torch.arange(n) % 5) - 2).double())[:, None]))
    for name in ('add', 'dy2', 'dres', 'dres2'):
        out[name] = rnd(torch.randn(n, D, generator=g, dtype=torch.float64)) if c[name] else None
    return out, td


@pytest.mark.parametrize('c', AC.LN, ids=[c['name'] for c in AC.LN])
def test_layernorm_envelope(env, c):
    L, ops = env
    lib = L.load()
    code = L.BF16 if c['dt'] == 'bf16' else L.F32
    u_out = U_BF16 if c['dt'] == 'bf16' else 0.0
    inp, td = _ln_inputs(c)
    n, D = c['rows'], c['D']
    d = {k_: (None if v_ is None else v_.to(td if k_ not in ('gamma', 'beta') else torch.float32).cuda().contiguous()) for k_, v_ in inp.items()}
    d64 = {k_: (None if v_ is None else v_.cuda()) for k_, v_ in inp.items()}
    fam = f"ln[{c['dt']} {D}]"
    poison(64)
    y, mean, rstd = nan_buffer(n * D, td).view(n, D), nan_buffer(n, torch.float32), nan_buffer(n, torch.float32)
    y, y2, mean, rstd = ops.layernorm_fwd(code, d['x'], d['gamma'], d['beta'], d['add'], out=(y, mean, rstd))
    rf = K.layernorm_fwd_ref(d64['x'], d64['gamma'], d64['beta'], d64['add'], u_out)
    _record(fam + ' y', K.check(y, rf['y'], rf['bound_y'], c['name'] + ' y'))
    _record(fam + ' mean', K.check(mean, rf['mean'], rf['bound_mean'], c['name'] + ' mean'))
    _record(fam + ' rstd', K.check(rstd, rf['rstd'], rf['bound_rstd'], c['name'] + ' rstd'))
    assert (y2 is None) == (not c['add'])
    if c['add']:
        _record(fam + ' y2', K.check(y2, rf['y2'], rf['bound_y2'], c['name'] + ' y2'))

    # backward from the kernel's own mean / rstd
    p, seed, word = 0.1, 0x0badf00d, 0xfffffff0
    sp = torch.from_numpy(np.array([word], np.uint32).view(np.int32)).cuda()
    poison(64)
    res = ops.layernorm_bwd(code, d['dy'], d['x'], d['gamma'], mean, rstd, dy2=d['dy2'], dres=d['dres'], dres2=d['dres2'],
                            drop=(p, seed, sp) if c['drop'] else None)
    dx, dg, db = res[:3]
    rb = K.layernorm_bwd_ref(d64['dy'], d64['dy2'], d64['x'], d64['gamma'], mean.double(), rstd.double(), d64['dres'], d64['dres2'], u_out)
    _record(fam + ' dx', K.check(dx, rb['dx'], rb['bound_dx'], c['name'] + ' dx'))
    _record(fam + ' dgamma', K.check(dg, rb['dgamma'], rb['bound_dgamma'], c['name'] + ' dgamma'))
    _record(fam + ' dbeta', K.check(db, rb['dbeta'], rb['bound_dbeta'], c['name'] + ' dbeta'))
    if c['drop']:
        keep = K.drop_keep((seed + word) & 0xffffffff, np.arange(n * D, dtype=np.uint64), K.drop_threshold(p)).reshape(n, D)
        want = torch.where(torch.from_numpy(keep).cuda(), (dx.float() * torch.tensor(K.inv_keep(p), dtype=torch.float32, device='cuda')).to(td),
                           torch.zeros((), dtype=td, device='cuda'))
        assert torch.equal(res[3], want), 'dx_drop differs from where(keep, dtype(dx / (1 - p)), 0)'

    # the split reduction: sedt_layernorm_bwd without parameter gradients, then sedt_layernorm_bwd_final - bit-identical to the fused call
    if not c['dres2'] and not c['drop']:
        nb = lib.sedt_layernorm_bwd_scratch(n, D)
        scratch = nan_buffer(nb // 4, torch.float32)
        dx2, dg2, db2 = nan_buffer(n * D, td).view(n, D), nan_buffer(D, torch.float32), nan_buffer(D, torch.float32)
        L.check(lib.sedt_layernorm_bwd(L.p(d['dy']), L.p(d['dy2']), L.p(d['x']), L.p(d['gamma']), L.p(mean), L.p(rstd), L.p(d['dres']), L.p(dx2),
                                       None, None, L.p(scratch), nb, n, D, code, L.stream_ptr()), 'layernorm_bwd')
        L.check(lib.sedt_layernorm_bwd_final(L.p(scratch), n, D, L.p(dg2), L.p(db2), L.stream_ptr()), 'layernorm_bwd_final')
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), 'split reduction differs from the fused call'


@pytest.mark.parametrize('dt,D', [('f32', 256), ('f32', 512), ('bf16', 256), ('bf16', 512)])
def test_layernorm_refuses_misaligned_views(env, dt, D):
    """a tensor that does not start on the boundary of the kernels' vector accesses is an error return, not a launch: every output keeps
    its NaN fill"""
    L, ops = env
    lib = L.load()
    code, td = (L.BF16, torch.bfloat16) if dt == 'bf16' else (L.F32, torch.float32)
    n = 5
    vec = D // 64                                            # elements per vector access
    big = torch.randn(n * D + vec, device='cuda').to(td)
    x_ok, x_off = big[:n * D].view(n, D), big[vec // 2:vec // 2 + n * D].view(n, D)      # half a vector into the allocation
    g = torch.ones(D + 4, device='cuda')
    gamma, beta = g[:D], torch.zeros(D, device='cuda')
    y, mean, rstd = nan_buffer(n * D, td).view(n, D), nan_buffer(n, torch.float32), nan_buffer(n, torch.float32)

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(y.float()).all() and torch.isnan(mean).all() and torch.isnan(rstd).all())
    with pytest.raises(RuntimeError, match='aligned'):
        ops.layernorm_fwd(code, x_off, gamma, beta, out=(y, mean, rstd))
    with pytest.raises(RuntimeError, match='aligned'):
        ops.layernorm_fwd(code, x_ok, g[1:D + 1], beta, out=(y, mean, rstd))
    with pytest.raises(RuntimeError, match='aligned'):
        ops.layernorm_fwd(code, x_ok, gamma, beta, add_t=x_off, out=(y, mean, rstd))
    assert untouched()
    with pytest.raises(AssertionError, match='contiguous'):
        ops.layernorm_fwd(code, torch.zeros(n, 2 * D, device='cuda', dtype=td)[:, :D], gamma, beta, out=(y, mean, rstd))
    ops.layernorm_fwd(code, x_ok, gamma, beta, out=(y, mean, rstd))
    with pytest.raises(RuntimeError, match='aligned'):
        ops.layernorm_bwd(code, x_off, x_ok, gamma, mean, rstd)
    with pytest.raises(RuntimeError, match='aligned'):
        ops.layernorm_bwd(code, x_ok, x_ok, gamma, mean, rstd, dres=x_off)
    # dx_drop is allocated by ops: the C entry point directly
    nb = lib.sedt_layernorm_bwd_scratch(n, D)
    scratch, dx = torch.empty(nb // 4, device='cuda'), nan_buffer(n * D + vec, td)
    r = lib.sedt_layernorm_bwd_drop(L.p(x_ok), None, L.p(x_ok), L.p(gamma), L.p(mean), L.p(rstd), None, None, L.p(dx[:n * D]), None, None,
                                    L.p(scratch), nb, n, D, L.p(dx[vec // 2:]), 0.1, 1, None, code, L.stream_ptr())
    assert r != 0 and b'aligned' in lib.sedt_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.float()).all())
