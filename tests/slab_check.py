"""Float64 references, element-wise error bounds, exact mask checks and torch emulations for the x-stationary slab kernels
(csrc/slab.h, csrc/enc_slab.hip, csrc/heads_slab.hip).  A helper of tests/test_slab_envelope_gpu.py and tests/test_slab_check_cpu.py,
not a conftest.  It stands on tests/attn_check.py (attention and LayerNorm references, the dropout restatement, check()) and
tests/gemm_check.py (the GEMM bound).  Everything is torch float64 on the device of its arguments.

Unit roundoffs as in tests/gemm_check.py: u_acc = 2^-24, u_bf16 = 2^-8, c = 2 (a bf16 result whose only error is its own rounding sits
at ratio 0.5).  Every stage is checked against a reference computed from the KERNEL'S OWN output of the stage before, so no error is
charged twice; a stage that is never stored (g_x1n, g_xn) is carried through the next stage's bound instead.

Building blocks
  lin(x, W, b):  z = x W^T + b from bf16-exact x and the bf16-rounded weight (the fragment packing rounds the f32 master once),
                 E(z) = sqrt(K) u_acc (|x| |W|^T) + u_acc (|z| + |b|)           f32 accumulation (tests/gemm_check.py), one f32 bias add
  a bf16 store of a value r with f32 error E:     |got - r| <= c (E + u_bf16 |r|) + tiny
  residual + dropout (x1, x2), ik = 1 / (1 - p):  r = res + keep ik z;   E = keep ik (E(z) + u_acc |z|) + u_acc |r|
                 (one f32 product with ik, one f32 add).  A dropped element adds 0.f to a bf16 value and rounds it back: it must equal
                 the residual BIT FOR BIT, which is asserted apart from the bound.
  ReLU + dropout (h):  r = keep ik relu(z);  E = keep (ik E(z) + u_acc |r|)    (ReLU is 1-Lipschitz).  keep = 0 gives a bound of
                 `tiny`, and h == 0 there is asserted exactly.
  masked gradient (g2, g1):  r = keep ik g;  E = u_acc |r|  (one f32 product; for p = 0 the value is copied).  The zero pattern must
                 equal the mask exactly wherever g != 0.

enc_qkv          mean, rstd, xn, xnp: attn_check.layernorm_fwd_ref with add = pos (y2 = xnp is formed in f32 from the unrounded
                 LayerNorm output); qk = lin(xnp_k, Wqk), v = lin(xn_k, Wv) from the kernel's own xnp / xn.
enc_attn_ffn     ctx, lse: attn_check.attention_fwd_ref on the kernel's qk, v with u_p = u_bf16 (the probabilities enter a bf16 MFMA),
                 keep index ((b 8 + h) S + i) S + j; x1 = residual(x, lin(ctx_k, Wo)), index row 256 + f; mean2, rstd2, x1n:
                 layernorm_fwd_ref(x1_k); h = relu-drop(lin(x1n_k, W1)), index row FF + f; x2 = residual(x1_k, lin(h_k, W2)),
                 index row 256 + f.
enc_ffn_bwd      g2 = masked(gx2) (the FFN-output mask again); gh = [h_k > 0] ik (g2_k W2): E = ik sqrt(256) u_acc |g2||W2| + u_acc |r|,
                 exactly zero where h_k is zero; g_x1n = gh_k W1 is rounded to bf16 in LDS and never stored:
                     E(g_x1n) = sqrt(FF) u_acc (|gh_k| |W1|) + u_bf16 |g_x1n|
                 LayerNorm backward is linear in dy, dx = rstd (a - mean(a) - xh mean(a xh)) + dres with a = dy gamma, so an error E on dy
                 moves dx by at most
                     D(E) = rstd ( |gamma| E + mean(|gamma| E) + |xh| mean(|gamma| E |xh|) )
                 and |gx1 - ref| <= layernorm_bwd_ref's bound_dx (u_out = u_bf16, dres = gx2) + c D(E(g_x1n)).
                 ln_part, one row of 512 per slab: sums over the slab's valid rows of dy xh (256) and of dy (256):
                     |part - ref| <= c [ (sqrt(32) + 4) u_acc sum_rows |dy xh| + sum_rows E(g_x1n) |xh| ] + tiny   (dbeta: without xh)
                 (at most 32 rows per slab; the + 4 covers xh formed in f32, as layernorm_bwd_ref's dgamma bound does).
                 g1 = masked(gx1_k) with the out-proj mask; gctx = g1_k Wo: the plain GEMM bound (gemm_check.check, K = 256, bf16 out).
enc_qkv_bwd      g_xn = [dq | dk | dv] W_in (K = 768) is rounded to bf16 in LDS as g_x1n is: E(g_xn) = sqrt(768) u_acc (...) + u_bf16 |g_xn|;
                 gx and ln_part as above with x, mean1_k, rstd1_k, gamma1 and dres = gx1.
heads_fwd        h1 = relu(lin(x, W1)), h2 = relu(lin(h1_k, W2)) (bf16); cls = lin(x, wc) with the f32 master weight and an f32 output:
                 |cls - ref| <= c E(z) + tiny; box = sigmoid(lin(h2_k, w3)), at = sigmoid(lin(x rows ((L-1) B + b) Qp, wa)):
                     y = 1 / (1 + e), e = exp(-z) by the fast exponential with relative error d_e <= 2^-22 (2 + |z|) (argument and result
                     rounding, as attn_check's eps); dy/dz = y (1 - y) and dy/de = -y^2 with y e = 1 - y, hence
                     |y - ref| <= c [ y (1 - y) (E(z) + d_e) + 4 u_acc y ] + tiny
                 The constant 4: one rounding of 1 + e (u_acc), the reciprocal / division (at most 1 ulp = 2 u_acc), one spare for the
                 f32 negation-free path through v_rcp.  Inference (h1 / h2 null) must equal training bit for bit.
heads_bwd        the folded gradients G = g_cls | g_at y (1 - y) | g_box y (1 - y) from the kernel's saved box / at, three f32
                 operations: E(G) = 3 u_acc |G|.  g_h2 = [h2 > 0] (G_box0 w3_0 + G_box1 w3_1): E = 5 u_acc (|G0 w3_0| + |G1 w3_1|);
                 g_h1 = [h1 > 0] (g_h2_k W2): GEMM bound; dhs = g_h1_k W1 + sum_c G_c w_c (c over the class and audio-tag rows, a serial
                 f32 sum of NC <= 32 terms on top of the accumulator): E = sqrt(256) u_acc |g_h1_k||W1| + (NC + 3) u_acc sum_c |G_c||w_c|.
                 part, per slab: [NG][256] sums over the slab's rows of G_c x (class, audio tag) or G_c h2 (box), then [NG] sums of G_c:
                     |part - ref| <= c (sqrt(32) + 4) u_acc sum_rows |G_c| |x| + tiny      (32 serial terms; + 3 for E(G), + 1 spare)

A clip whose keys are ALL padded has no finite reference (every score is -inf) and is not part of any table row.  The
weight-gradient GEMMs that read g2 / gh / g1 / h are the GEMM tests' business.

Emulations (emulate_enc, emulate_heads) make the kernels' rounding decisions in torch f32 on any device - bf16 at every LDS / global
tile, f32 inside - and can plant numerics-only faults (FAULTS_ENC, FAULTS_HEADS); tests/test_slab_check_cpu.py shows that the honest
emulation passes every bound at every table row and that each fault fails.
"""
import math
import zlib

import numpy as np
import torch

import attn_check as A
import gemm_check
from attn_check import attention_fwd_ref, check, drop_keep, drop_threshold, inv_keep, keep_mask, layernorm_bwd_ref, layernorm_fwd_ref
from gemm_check import TINY, U_ACC, U_BF16

C_ = 2.0
D = 256
H = 8
SR = 32
NEG = float('-inf')

FAULTS_ENC = ('tail_row', 'pos_v', 'hid_idx256', 'chunk_c2', 'res_x', 'attn_nohead', 'bwd_mask_seed', 'ln_part_shift')
FAULTS_HEADS = ('at_first_layer', 'cls_bias_32', 'part_row31')


# ------------------------------------------------------------------------------------------------ small pieces
def bfw(w):
    """the fragment packing's rounding of an f32 master weight"""
    return w.float().bfloat16().double()


def lin(x, w, b=None):
    """z = x w^T (+ b) and its f32 error E(z); x [M, K], w [N, K], b [N] float64"""
    K = x.shape[1]
    z = x @ w.t()
    ab = x.abs() @ w.abs().t()
    if b is not None:
        z = z + b
    E = math.sqrt(K) * U_ACC * ab + U_ACC * (z.abs() + (b.abs() if b is not None else 0.0))
    return z, E


def bf16_bound(ref, E):
    return C_ * (E + U_BF16 * ref.abs()) + TINY


def elem_keep(seed, rows, cols, p, ld=None):
    """keep decisions [rows, cols] (numpy bool) of element index row ld + col"""
    if p <= 0:
        return np.ones((rows, cols), bool)
    ld = cols if ld is None else ld
    idx = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(ld) + np.arange(cols, dtype=np.uint64)[None, :])
    return drop_keep(seed & 0xffffffff, idx, drop_threshold(p))


def ikeep(p):
    return inv_keep(p) if p > 0 else 1.0


def assert_bits_where(got, want, where, what):
    """got == want bit for bit at the positions of `where` (bf16 tensors compared as values: no NaN is expected there)"""
    g, w = got.double(), want.double()
    bad = where & ~(g == w)
    if bool(bad.any()):
        rr, cc = bad.nonzero(as_tuple=True)
        raise AssertionError(f'{what}: {int(bad.sum())} elements that must be exact differ, first (row, col) = ({int(rr[0])}, {int(cc[0])}); '
                             f'rows {gemm_check._ranges(rr.tolist())}')


def assert_zero_pattern(got, keep, live, what):
    """(got != 0) == keep wherever `live` (the positions whose kept value is non-zero)"""
    nz = got.double() != 0
    bad = live & (nz != keep)
    if bool(bad.any()):
        rr, cc = bad.nonzero(as_tuple=True)
        raise AssertionError(f'{what}: {int(bad.sum())} keep decisions differ from drop_keep, first (row, col) = ({int(rr[0])}, {int(cc[0])}); '
                             f'rows {gemm_check._ranges(rr.tolist())}')


def residual_drop(res, z, E, keep, ik):
    k = keep.double()
    r = res + k * ik * z
    return r, bf16_bound(r, k * ik * (E + U_ACC * z.abs()) + U_ACC * r.abs())


def masked_grad(g, keep, ik):
    r = keep.double() * ik * g
    return r, bf16_bound(r, U_ACC * r.abs())


def slab_sum(v, B, S):
    """[B S, N] -> [B ceil(S / 32), N]: sums over the rows of each 32-token slab of each clip"""
    N = v.shape[1]
    SL = (S + SR - 1) // SR
    pad = torch.zeros(B, SL * SR, N, dtype=v.dtype, device=v.device)
    pad[:, :S] = v.reshape(B, S, N)
    return pad.reshape(B * SL, SR, N).sum(1)


def rows_slab_sum(v):
    """[rows, N] -> [ceil(rows / 32), N] (the heads' slabs run over the stacked rows)"""
    return slab_sum(v, 1, v.shape[0])


def ln_bwd_slab(dy, E, x, gamma, mean_k, rstd_k, dres, B, S):
    """LayerNorm backward of an unstored bf16 dy with error E -> (dx, bound_dx, part [slabs, 512], bound_part)"""
    lb = layernorm_bwd_ref(dy, None, x, gamma, mean_k, rstd_k, dres, None, U_BF16)
    rs = rstd_k[:, None]
    xh = (x - mean_k[:, None]) * rs
    aE = gamma.abs() * E
    extra = rs * (aE + aE.mean(1, keepdim=True) + xh.abs() * (aE * xh.abs()).mean(1, keepdim=True))
    k = (math.sqrt(SR) + 4) * U_ACC
    part = torch.cat([slab_sum(dy * xh, B, S), slab_sum(dy, B, S)], 1)
    bpart = C_ * torch.cat([k * slab_sum((dy * xh).abs(), B, S) + slab_sum(E * xh.abs(), B, S),
                            k * slab_sum(dy.abs(), B, S) + slab_sum(E, B, S)], 1) + TINY
    return lb['dx'], lb['bound_dx'] + C_ * extra, part, bpart


def sigmoid_ref(z, E):
    y = torch.sigmoid(z)
    de = 2.0 ** -22 * (2.0 + z.abs())
    return y, C_ * (y * (1.0 - y) * (E + de) + 4 * U_ACC * y) + TINY


def at_rows(L, B, Qp, first_layer=False):
    return [((0 if first_layer else L - 1) * B + b) * Qp for b in range(B)]


# ------------------------------------------------------------------------------------------------ encoder: masks
def enc_masks(c, t, dev):
    """the four keep masks of a row (torch bool on dev) from its effective seeds"""
    B, S, FF, p = c['B'], c['S'], c['FF'], c['p']
    M = B * S
    sa, so, sh, sf = [(s + t['word']) & 0xffffffff for s in t['seeds']]
    return dict(attn=torch.from_numpy(keep_mask(sa, B, H, S, S, p)).to(dev), o=torch.from_numpy(elem_keep(so, M, D, p)).to(dev),
                h=torch.from_numpy(elem_keep(sh, M, FF, p)).to(dev), f=torch.from_numpy(elem_keep(sf, M, D, p)).to(dev))


def _dev(t, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in t.items()}


# ------------------------------------------------------------------------------------------------ encoder: checks
def check_enc_qkv(c, t, o):
    """t: inputs (float64), o: the kernel's xn, xnp, mean, rstd, qk, v -> dict output -> largest error / bound ratio"""
    n = c['name']
    ln = layernorm_fwd_ref(t['x'], t['gamma1'], t['beta1'], t['pos'], U_BF16)
    r = dict(xn=check(o['xn'], ln['y'], ln['bound_y'], n + ' xn'), xnp=check(o['xnp'], ln['y2'], ln['bound_y2'], n + ' xnp'),
             mean=check(o['mean'], ln['mean'], ln['bound_mean'], n + ' mean'), rstd=check(o['rstd'], ln['rstd'], ln['bound_rstd'], n + ' rstd'))
    w = bfw(t['w_in'])
    z, E = lin(o['xnp'].double(), w[:2 * D], t['b_in'][:2 * D])
    r['qk'] = check(o['qk'], z, bf16_bound(z, E), n + ' qk')
    z, E = lin(o['xn'].double(), w[2 * D:], t['b_in'][2 * D:])
    r['v'] = check(o['v'], z, bf16_bound(z, E), n + ' v')
    return r


def check_enc_attn_ffn(c, t, o, m):
    """o holds the kernel's qk, v (enc_qkv) and ctx, lse, x1, mean2, rstd2, x1n, h, x2; m = enc_masks"""
    n, B, S, p = c['name'], c['B'], c['S'], c['p']
    ik = ikeep(p)
    qk, v = o['qk'].double(), o['v'].double()
    rf = attention_fwd_ref(A.heads(qk[:, :D], B, H, S), A.heads(qk[:, D:], B, H, S), A.heads(v, B, H, S), t['kpm'], None, m['attn'], p,
                           U_BF16, U_BF16)
    r = dict(ctx=check(A.heads(o['ctx'], B, H, S), rf['o'], rf['bound_o'], n + ' ctx'),
             lse=check(o['lse'].reshape(B, H, S), rf['lse'], rf['bound_lse'], n + ' lse'))
    z, E = lin(o['ctx'].double(), bfw(t['w_o']), t['b_o'])
    ref, bound = residual_drop(t['x'], z, E, m['o'], ik)
    r['x1'] = check(o['x1'], ref, bound, n + ' x1')
    assert_bits_where(o['x1'], t['x'], ~m['o'], n + ' x1 (dropped: = x)')
    x1 = o['x1'].double()
    ln = layernorm_fwd_ref(x1, t['gamma2'], t['beta2'], None, U_BF16)
    r['x1n'] = check(o['x1n'], ln['y'], ln['bound_y'], n + ' x1n')
    r['mean2'] = check(o['mean2'], ln['mean'], ln['bound_mean'], n + ' mean2')
    r['rstd2'] = check(o['rstd2'], ln['rstd'], ln['bound_rstd'], n + ' rstd2')
    z, E = lin(o['x1n'].double(), bfw(t['w1']), t['b1'])
    kh = m['h'].double()
    ref = kh * ik * torch.relu(z)
    r['h'] = check(o['h'], ref, kh * (C_ * (ik * E + (U_ACC + U_BF16) * ref.abs())) + TINY, n + ' h')
    assert_bits_where(o['h'], torch.zeros_like(ref), ~m['h'], n + ' h (dropped: = 0)')
    z, E = lin(o['h'].double(), bfw(t['w2']), t['b2'])
    ref, bound = residual_drop(x1, z, E, m['f'], ik)
    r['x2'] = check(o['x2'], ref, bound, n + ' x2')
    assert_bits_where(o['x2'], x1, ~m['f'], n + ' x2 (dropped: = x1)')
    return r


def check_enc_ffn_bwd(c, t, o, m):
    """o: the kernel's h, x1, mean2, rstd2 (forward) and g2, gh, gx1, g1, gctx, ln_part2"""
    n, B, S, FF, p = c['name'], c['B'], c['S'], c['FF'], c['p']
    ik = ikeep(p)
    ref, bound = masked_grad(t['gx2'], m['f'], ik)
    r = dict(g2=check(o['g2'], ref, bound, n + ' g2'))
    assert_zero_pattern(o['g2'], m['f'], t['gx2'] != 0, n + ' g2')
    hk = o['h'].double()
    live = (hk > 0).double()
    z, E = lin(o['g2'].double(), bfw(t['w2']).t())                        # [M, 256] x W2 [256, FF]
    ref = live * ik * z
    r['gh'] = check(o['gh'], ref, live * (C_ * (ik * E + (U_ACC + U_BF16) * ref.abs())) + TINY, n + ' gh')
    assert_bits_where(o['gh'], torch.zeros_like(ref), hk == 0, n + ' gh (h = 0: = 0)')
    gh = o['gh'].double()
    w1t = bfw(t['w1']).t()                                                # [256, FF]: g_x1n = gh W1
    dy = gh @ w1t.t()
    Edy = math.sqrt(FF) * U_ACC * (gh.abs() @ w1t.abs().t()) + U_BF16 * dy.abs()
    dx, bdx, part, bpart = ln_bwd_slab(dy, Edy, o['x1'].double(), t['gamma2'], o['mean2'].double(), o['rstd2'].double(), t['gx2'], B, S)
    r['gx1'] = check(o['gx1'], dx, bdx, n + ' gx1')
    r['ln_part2'] = check(o['ln_part2'], part, bpart, n + ' ln_part (LayerNorm2)')
    ref, bound = masked_grad(o['gx1'].double(), m['o'], ik)
    r['g1'] = check(o['g1'], ref, bound, n + ' g1')
    assert_zero_pattern(o['g1'], m['o'], o['gx1'].double() != 0, n + ' g1')
    g1 = o['g1'].double()
    wo = bfw(t['w_o'])                                                    # gctx = g1 Wo
    r['gctx'] = gemm_check.check(o['gctx'], (g1 @ wo).cpu(), (g1.abs() @ wo.abs()).cpu(), D, U_BF16, what=n + ' gctx')
    return r


def check_enc_qkv_bwd(c, t, o):
    """o: the kernel's mean, rstd (enc_qkv), gx1 (enc_ffn_bwd: the residual gradient) and gx, ln_part1"""
    n, B, S = c['name'], c['B'], c['S']
    dqkv = torch.cat([t['dqk'], t['dv']], 1)
    w = bfw(t['w_in'])                                                    # [768, 256]: g_xn = dqkv W_in
    dy = dqkv @ w
    Edy = math.sqrt(3 * D) * U_ACC * (dqkv.abs() @ w.abs()) + U_BF16 * dy.abs()
    dx, bdx, part, bpart = ln_bwd_slab(dy, Edy, t['x'], t['gamma1'], o['mean'].double(), o['rstd'].double(), o['gx1'].double(), B, S)
    return dict(gx=check(o['gx'], dx, bdx, n + ' gx'), ln_part1=check(o['ln_part1'], part, bpart, n + ' ln_part (LayerNorm1)'))


# ------------------------------------------------------------------------------------------------ encoder: emulation
def _bf(t):
    return t.to(torch.bfloat16).float()


def _f(t):
    return t.to(torch.float32)


def _ln32(x, g, b):
    mu = x.sum(1, keepdim=True) * np.float32(1.0 / D)
    xc = x - mu
    rs = torch.rsqrt((xc * xc).sum(1, keepdim=True) * np.float32(1.0 / D) + np.float32(1e-5))
    return xc * rs * g + b, mu[:, 0], rs[:, 0]


def _ln_bwd32(dy, x, g, mu, rs, dres, B, S):
    rs = rs[:, None]
    xh = (x - mu[:, None]) * rs
    a = dy * g
    c1, c2 = a.sum(1, keepdim=True) * np.float32(1.0 / D), (a * xh).sum(1, keepdim=True) * np.float32(1.0 / D)
    return rs * (a - c1 - xh * c2) + dres, torch.cat([slab_sum(dy * xh, B, S), slab_sum(dy, B, S)], 1)


def emulate_enc(c, t, fault=None):
    """torch f32 emulation of the four encoder slab kernels on a row's inputs -> dict of every output (float64 / float32 values)"""
    assert fault is None or fault in FAULTS_ENC, fault
    B, S, FF, p = c['B'], c['S'], c['FF'], c['p']
    M = B * S
    dev = t['x'].device
    ik = np.float32(ikeep(p))
    m = enc_masks(c, t, dev)
    sa, so, sh, sf = [(s + t['word']) & 0xffffffff for s in t['seeds']]
    if p > 0 and fault == 'hid_idx256':
        m['h'] = torch.from_numpy(elem_keep(sh, M, FF, p, ld=D)).to(dev)
    if p > 0 and fault == 'attn_nohead':
        idx = ((np.arange(B, dtype=np.uint64)[:, None, None, None] * np.uint64(H) * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, None, :, None])
               * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, None, None, :])
        m['attn'] = torch.from_numpy(np.broadcast_to(drop_keep(sa, idx, drop_threshold(p)), (B, H, S, S)).copy()).to(dev)
    x, pos = _f(t['x']), _f(t['pos'])
    wi, wo, w1, w2 = (_f(bfw(t[k])) for k in ('w_in', 'w_o', 'w1', 'w2'))
    o = {}
    # ---- enc_qkv
    y, mu, rs = _ln32(x, _f(t['gamma1']), _f(t['beta1']))
    o['xn'], o['xnp'], o['mean'], o['rstd'] = _bf(y), _bf(y + pos), mu, rs
    o['qk'] = _bf(o['xnp'] @ wi[:2 * D].t() + _f(t['b_in'][:2 * D]))
    o['v'] = _bf((o['xnp'] if fault == 'pos_v' else o['xn']) @ wi[2 * D:].t() + _f(t['b_in'][2 * D:]))
    if fault == 'tail_row' and S % SR and S > 1:
        for b in range(B):
            o['v'][b * S + S - 1] = o['v'][b * S + S - 2]
    # ---- enc_attn_ffn
    q, k, v = A.heads(o['qk'][:, :D], B, H, S).float(), A.heads(o['qk'][:, D:], B, H, S).float(), A.heads(o['v'], B, H, S).float()
    s = (q @ k.transpose(-1, -2)) * np.float32(A.SCALE)
    if t['kpm'] is not None:
        s = s.masked_fill(t['kpm'][:, None, None, :], NEG)
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    ssum = e.sum(-1, keepdim=True)
    o['lse'] = (mx + torch.log(ssum)).squeeze(-1)
    kf = m['attn'].float() * ik
    o['ctx'] = _bf(A.rows((_bf(e * kf) @ v) / ssum))
    z = o['ctx'] @ wo.t() + _f(t['b_o'])
    o['x1'] = _bf(torch.where(m['o'], z * ik, torch.zeros_like(z)) + x)
    y, o['mean2'], o['rstd2'] = _ln32(o['x1'], _f(t['gamma2']), _f(t['beta2']))
    o['x1n'] = _bf(y)
    z = o['x1n'] @ w1.t() + _f(t['b1'])
    o['h'] = _bf(torch.where(m['h'], torch.relu(z) * ik, torch.zeros_like(z)))
    hop = o['h']
    if fault == 'chunk_c2':                                   # chunk c of linear2's operand comes from chunk c - 2's buffer
        hop = o['h'].clone()
        for cch in range(2, FF // 512):
            hop[:, cch * 512:(cch + 1) * 512] = o['h'][:, (cch - 2) * 512:(cch - 1) * 512]
    z = hop @ w2.t() + _f(t['b2'])
    o['x2'] = _bf(torch.where(m['f'], z * ik, torch.zeros_like(z)) + (x if fault == 'res_x' else o['x1']))
    if fault == 'tail_row' and S % SR and S > 1:
        for b in range(B):
            o['x2'][b * S + S - 1] = o['x2'][b * S + S - 2]
    # ---- enc_ffn_bwd
    gx2 = _f(t['gx2'])
    mf = torch.from_numpy(elem_keep(so, M, D, p)).to(dev) if fault == 'bwd_mask_seed' else m['f']
    o['g2'] = _bf(torch.where(mf, gx2 * ik, torch.zeros_like(gx2)))
    z = o['g2'] @ w2
    o['gh'] = _bf(torch.where(o['h'] > 0, z * ik, torch.zeros_like(z)))
    gx1n = _bf(o['gh'] @ w1)
    dx, part = _ln_bwd32(gx1n, o['x1'], _f(t['gamma2']), o['mean2'], o['rstd2'], gx2, B, S)
    o['gx1'] = _bf(dx)
    o['ln_part2'] = part.roll(-1, 0) if fault == 'ln_part_shift' else part
    o['g1'] = _bf(torch.where(m['o'], o['gx1'] * ik, torch.zeros_like(dx)))
    o['gctx'] = _bf(o['g1'] @ wo)
    # ---- enc_qkv_bwd
    gxn = _bf(torch.cat([_f(t['dqk']), _f(t['dv'])], 1) @ wi)
    dx, part = _ln_bwd32(gxn, x, _f(t['gamma1']), o['mean'], o['rstd'], o['gx1'], B, S)
    o['gx'] = _bf(dx)
    o['ln_part1'] = part.roll(-1, 0) if fault == 'ln_part_shift' else part
    return o


def check_enc_all(c, t, o):
    """every stage of a row -> dict 'kernel output' -> ratio"""
    m = enc_masks(c, t, t['x'].device)
    r = {}
    for kern, res in (('enc_qkv', check_enc_qkv(c, t, o)), ('enc_attn_ffn', check_enc_attn_ffn(c, t, o, m)),
                      ('enc_ffn_bwd', check_enc_ffn_bwd(c, t, o, m)), ('enc_qkv_bwd', check_enc_qkv_bwd(c, t, o))):
        r.update({f'{kern} {k}': v for k, v in res.items()})
    return r


# ------------------------------------------------------------------------------------------------ encoder: inputs
def kpm_pattern(kind, B, S):
    """bool [B][S] (True = padded) or None.  Every clip keeps a live key.
      'tail'       the last keys of every clip from 3 + b keys in front of the last 32-key tile edge (the padded run crosses it)
      'scattered'  keys with (7 j + b) % 3 == 0
      'key0'       key 0 (and key b)
      'single'     clip 0 keeps the single key (2 S) // 3, the other clips keep everything
      'differ'     clip 0 nothing, clip 1 its last 7 keys, clip 2 scattered"""
    if kind is None:
        return None
    rows = []
    for b in range(B):
        if kind == 'tail':
            edge = SR * ((S - 1) // SR)
            assert edge >= SR, 'no 32-key tile edge to cross'
            r = [j >= edge - 3 - b for j in range(S)]
        elif kind == 'scattered':
            r = [(7 * j + b) % 3 == 0 for j in range(S)]
        elif kind == 'key0':
            r = [j == 0 or j == b for j in range(S)]
        elif kind == 'single':
            r = [j != (2 * S) // 3 for j in range(S)] if b == 0 else [False] * S
        elif kind == 'differ':
            r = [False] * S if b % 3 == 0 else [j >= S - 7 for j in range(S)] if b % 3 == 1 else [(7 * j + b) % 3 == 0 for j in range(S)]
        else:
            raise ValueError(kind)
        assert not all(r), (kind, b, S)
        rows.append(r)
    return rows


def _steps(n, g, base=4.0, cyc=9):
    return (base ** ((torch.arange(n) % cyc) - cyc // 2).double())[:, None]


def enc_inputs(c):
    """the seeded operands of a row of slab_cases.ENC on the CPU: float64 tensors holding bf16-exact activations and f32-exact
    parameters.  LayerNorm parameters and biases sit away from 1 and 0; rows of x carry magnitude steps (4^-4 .. 4^4, offsets -2 .. 2)
    or, kind 'mean100', mean 100 / std 0.05."""
    B, S, FF = c['B'], c['S'], c['FF']
    M = B * S
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))

    def rn(*sh):
        return torch.randn(*sh, generator=g, dtype=torch.float64)

    def b16(t):
        return t.to(torch.bfloat16).double()

    def f32(t):
        return t.float().double()
    x = rn(M, D)
    x = 100.0 + 0.05 * x if c['kind'] == 'mean100' else x * _steps(M, g) + (torch.arange(M) % 5 - 2).double()[:, None]
    t = dict(x=b16(x), pos=b16(0.5 * rn(M, D)), gamma1=f32(1.0 + 0.5 * rn(D)), beta1=f32(rn(D)), gamma2=f32(1.0 + 0.5 * rn(D)),
             beta2=f32(0.7 * rn(D)), w_in=f32(0.08 * rn(3 * D, D)), b_in=f32(0.3 * rn(3 * D)), w_o=f32(0.08 * rn(D, D)), b_o=f32(0.3 * rn(D)),
             w1=f32(0.08 * rn(FF, D)), b1=f32(0.3 * rn(FF)), w2=f32(0.04 * rn(D, FF)), b2=f32(0.3 * rn(D)),
             gx2=b16(rn(M, D) * _steps(M, g, 2.0, 5)), dqk=b16(rn(M, 2 * D) * _steps(M, g, 2.0, 7)), dv=b16(rn(M, D) * _steps(M, g, 2.0, 3)))
    pat = kpm_pattern(c['kpm'], B, S)
    t['kpm'] = None if pat is None else torch.tensor(pat)
    s0 = zlib.crc32(c['name'].encode()[::-1])
    t['seeds'] = tuple((s0 * (i + 1) + 0x1234567 * i) & 0x7fffffff for i in range(4))
    t['word'] = 0x9e3779b1 ^ (s0 >> 3)                       # the device seed word: seed + word wraps past 2^32 for some rows
    return t


# ------------------------------------------------------------------------------------------------ heads
def heads_inputs(c):
    """seeded operands of a row of slab_cases.HEADS: hs rows with per-row magnitude steps (neighbouring rows never share one), f32
    parameters with biases away from 0, upstream gradients"""
    L, B, Qp, C1, CA = c['L'], c['B'], c['Qp'], c['C1'], c['CA']
    R = L * B * Qp
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))

    def rn(*sh):
        return torch.randn(*sh, generator=g, dtype=torch.float64)

    def f32(t):
        return t.float().double()
    t = dict(x=(rn(R, D) * _steps(R, g, 1.5, 7)).to(torch.bfloat16).double(), wc=f32(0.08 * rn(C1, D)), bc=f32(0.5 * rn(C1)),
             w1=f32(0.08 * rn(D, D)), b1=f32(0.3 * rn(D)), w2=f32(0.08 * rn(D, D)), b2=f32(0.3 * rn(D)), w3=f32(0.08 * rn(2, D)), b3=f32(0.5 * rn(2)),
             wa=f32(0.08 * rn(CA, D)) if CA else None, ba=f32(0.5 * rn(CA)) if CA else None,
             g_cls=f32(rn(R, C1) * _steps(R, g, 2.0, 5)), g_box=f32(rn(R, 2) * _steps(R, g, 2.0, 3)),
             g_at=f32(rn(B, CA)) if (CA and c['g_at']) else None)
    return t


def _folded(c, t, o):
    """G [rows, NG] float64 from the kernel's saved box / at: g_cls | g_at y (1 - y) on the audio-tag rows | g_box y (1 - y)"""
    L, B, Qp, C1, CA = c['L'], c['B'], c['Qp'], c['C1'], c['CA']
    R = L * B * Qp
    G = torch.zeros(R, C1 + CA + 2, dtype=torch.float64, device=t['x'].device)
    G[:, :C1] = t['g_cls']
    if CA and t['g_at'] is not None:
        y = o['at'].double()
        G[at_rows(L, B, Qp), C1:C1 + CA] = t['g_at'] * y * (1 - y)
    y = o['box'].double()
    G[:, C1 + CA:] = t['g_box'] * y * (1 - y)
    return G


def check_heads_fwd(c, t, o):
    n, L, B, Qp, CA = c['name'], c['L'], c['B'], c['Qp'], c['CA']
    z, E = lin(t['x'], bfw(t['w1']), t['b1'])
    ref = torch.relu(z)
    r = dict(h1=check(o['h1'], ref, bf16_bound(ref, E), n + ' h1'))
    z, E = lin(o['h1'].double(), bfw(t['w2']), t['b2'])
    ref = torch.relu(z)
    r['h2'] = check(o['h2'], ref, bf16_bound(ref, E), n + ' h2')
    z, E = lin(t['x'], t['wc'], t['bc'])
    r['cls'] = check(o['cls'], z, C_ * E + TINY, n + ' cls')
    z, E = lin(o['h2'].double(), t['w3'], t['b3'])
    y, by = sigmoid_ref(z, E)
    r['box'] = check(o['box'], y, by, n + ' box')
    if CA:
        z, E = lin(t['x'][at_rows(L, B, Qp)], t['wa'], t['ba'])
        y, by = sigmoid_ref(z, E)
        r['at'] = check(o['at'], y, by, n + ' at')
    return r


def check_heads_bwd(c, t, o):
    """o: the kernel's h1, h2, box, at (forward) and g_h2, g_h1, dhs, part"""
    n, C1, CA = c['name'], c['C1'], c['CA']
    NC, NG = C1 + CA, C1 + CA + 2
    G = _folded(c, t, o)
    h1, h2, x = o['h1'].double(), o['h2'].double(), t['x']
    live = (h2 > 0).double()
    a0, a1 = G[:, NC:NC + 1] * t['w3'][0][None, :], G[:, NC + 1:NC + 2] * t['w3'][1][None, :]
    ref = live * (a0 + a1)
    r = dict(g_h2=check(o['g_h2'], ref, live * (C_ * (5 * U_ACC * (a0.abs() + a1.abs()) + U_BF16 * ref.abs())) + TINY, n + ' g_h2'))
    assert_bits_where(o['g_h2'], torch.zeros_like(ref), h2 == 0, n + ' g_h2 (h2 = 0: = 0)')
    gh2 = o['g_h2'].double()
    live = (h1 > 0).double()
    z, E = lin(gh2, bfw(t['w2']).t())
    ref = live * z
    r['g_h1'] = check(o['g_h1'], ref, live * (C_ * (E + U_BF16 * ref.abs())) + TINY, n + ' g_h1')
    assert_bits_where(o['g_h1'], torch.zeros_like(ref), h1 == 0, n + ' g_h1 (h1 = 0: = 0)')
    gh1 = o['g_h1'].double()
    z, E = lin(gh1, bfw(t['w1']).t())
    wn = t['wc'] if not CA else torch.cat([t['wc'], t['wa']], 0)                  # [NC, 256]
    ref = z + G[:, :NC] @ wn
    r['dhs'] = check(o['dhs'], ref, bf16_bound(ref, E + (NC + 3) * U_ACC * (G[:, :NC].abs() @ wn.abs())), n + ' dhs')
    k = C_ * (math.sqrt(SR) + 4) * U_ACC
    pw, pb, bw, bb = [], [], [], []
    for cix in range(NG):
        tile = x if cix < NC else h2
        gcol = G[:, cix:cix + 1]
        pw.append(rows_slab_sum(gcol * tile))
        bw.append(rows_slab_sum((gcol * tile).abs()))
        pb.append(rows_slab_sum(gcol))
        bb.append(rows_slab_sum(gcol.abs()))
    part = torch.cat([torch.cat(pw, 1), torch.cat(pb, 1)], 1)                    # [slabs, NG 256 + NG]
    bound = k * torch.cat([torch.cat(bw, 1), torch.cat(bb, 1)], 1) + TINY
    r['part'] = check(o['part'], part, bound, n + ' part')
    return r


def emulate_heads(c, t, fault=None):
    assert fault is None or fault in FAULTS_HEADS, fault
    L, B, Qp, C1, CA = c['L'], c['B'], c['Qp'], c['C1'], c['CA']
    NC = C1 + CA
    x = _f(t['x'])
    w1, w2 = _f(bfw(t['w1'])), _f(bfw(t['w2']))
    o = {}
    o['h1'] = _bf(torch.relu(x @ w1.t() + _f(t['b1'])))
    o['h2'] = _bf(torch.relu(o['h1'] @ w2.t() + _f(t['b2'])))
    o['cls'] = x @ _f(t['wc']).t() + _f(t['bc'])
    if fault == 'cls_bias_32':
        o['cls'][32:] = (x @ _f(t['wc']).t())[32:]
    o['box'] = torch.sigmoid(o['h2'] @ _f(t['w3']).t() + _f(t['b3']))
    if CA:
        o['at'] = torch.sigmoid(x[at_rows(L, B, Qp, fault == 'at_first_layer')] @ _f(t['wa']).t() + _f(t['ba']))
    G = _f(_folded(c, t, o))
    o['g_h2'] = _bf(torch.where(o['h2'] > 0, G[:, NC:NC + 1] * _f(t['w3'])[0][None, :] + G[:, NC + 1:NC + 2] * _f(t['w3'])[1][None, :],
                                torch.zeros_like(x)))
    o['g_h1'] = _bf(torch.where(o['h1'] > 0, o['g_h2'] @ w2, torch.zeros_like(x)))
    wn = _f(t['wc']) if not CA else torch.cat([_f(t['wc']), _f(t['wa'])], 0)
    o['dhs'] = _bf(o['g_h1'] @ w1 + G[:, :NC] @ wn)
    Gw = G.clone()
    if fault == 'part_row31':
        Gw[31::32] = 0
    pw = [rows_slab_sum(Gw[:, i:i + 1] * (x if i < NC else o['h2'])) for i in range(NC + 2)]
    pb = [rows_slab_sum(G[:, i:i + 1]) for i in range(NC + 2)]
    o['part'] = torch.cat(pw + pb, 1)
    return o


def check_heads_all(c, t, o):
    r = {f'heads_fwd {k}': v for k, v in check_heads_fwd(c, t, o).items()}
    r.update({f'heads_bwd {k}': v for k, v in check_heads_bwd(c, t, o).items()})
    return r
