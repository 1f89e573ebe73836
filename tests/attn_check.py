"""Float64 references, element-wise error bounds and exact dropout-mask probes for the stand-alone attention and LayerNorm kernels
(csrc/attn_mfma.hip, csrc/attn_f32_mfma.hip, csrc/norm_attn.hip).  A helper of tests/test_attn_ln_envelope_gpu.py and
tests/test_attn_check_cpu.py, not a conftest; the slab kernels' tests are meant to reuse it.  Everything is torch float64 on the device
of its arguments.

Unit roundoffs: u_acc = 2^-24 (f32 arithmetic), u_bf16 = 2^-8, c = 2 as in tests/gemm_check.py: a result whose only error is its own
bf16 rounding sits at ratio 0.5.  u_p = u_bf16 for the kernels that hand probabilities (and dS) to a bf16 MFMA (attn_*_mfma_kernel), 0
otherwise; u_out = u_bf16 for bf16 tensors, 0 for f32.

Attention forward, from the dtype-rounded operands [B, H, L, 32]:

    s_ij = scale q_i . k_j (+ amask_ij; -inf where kpm),  lse_i,  P_ij = exp(s_ij - lse_i),  Pd = keep P / (1 - p),  o = Pd V

    eps_ij = sqrt(32) u_acc scale sum_d |q_id| |k_jd| + 2^-22 (2 + |s_ij - lse_i|)          (0 where s_ij = -inf)
             f32 accumulation of the score;  argument and result rounding of the fast exponential
    |o - ref|   <= c [ sum_j Pd_ij |V_jd| (u_p + eps_ij + sqrt(Lk) u_acc) + (sum_j Pd_ij |V_jd|) max_j eps_ij + u_out |ref| ] + tiny
    |lse - ref| <= c ( max_j eps_ij + 2^-23 (1 + |ref|) )

(the max_j eps term is the error of the row sum, which every probability of the row shares).

Attention backward.  The reference reads the kernel's own lse and o (as the backbone test reads the stage before), so the forward's
error is not charged twice:

    P = exp(s - lse_k),  delta_i = dO_i . o_k,i,  dP = keep (dO V^T) / (1 - p),  dS = P (dP - delta)
    E(dS) = P (|dP| + |delta|) (u_p + eps) + P sqrt(32) u_acc ( |dO| |V|^T keep / (1 - p) + sum_d |o_k| |dO| )
    |dq - ref| <= c [ scale E(dS) |K| + sqrt(Lk) u_acc scale |dS| |K| + u_out |ref| ] + tiny         (dk: with Q, sqrt(Lq), transposed)
    |dv - ref| <= c [ (Pd (u_p + eps))^T |dO| + sqrt(Lq) u_acc Pd^T |dO| + u_out |ref| ] + tiny

LayerNorm, Lg = log2(D) + 2, e_mu = Lg u_acc mean|x|, xh = (x - mu) rstd:

    |y - ref|    <= c [ u_out |ref| + u_acc (8 |xh g| + |b|) + rstd |g| e_mu + 2 |xh g| e_mu mean|x - mu| rstd^2 ] + tiny
    |y2 - ref|   <= the same with ref = y + add in the first term, + c u_acc |ref|
    |mean - ref| <= c e_mu + tiny,   |rstd - ref| <= c rstd (2 e_mu mean|x - mu| rstd^2 + (e_mu rstd)^2 / 2 + 8 u_acc)
    (the variance around the kernel's mean is var + (mu_k - mu)^2 exactly: the squared term is all that moves rstd of a constant row)
    backward (reads the kernel's own mean and rstd), a = (dy + dy2) g:
    |dx - ref|   <= c [ u_out |ref| + Lg u_acc rstd (|a| + mean|a| + |xh| mean|a xh|) + u_acc (|dres| + |dres2|) ] + tiny
    |dgamma - ref| <= c (sqrt(rows) + 4) u_acc sum_rows |dy xh| + tiny,   dbeta: sum_rows |dy|

Dropout masks are not bounded but checked exactly: keep_mask() restates drop_keep / drop_threshold of csrc/common.h in numpy on
tests/noise_views_ref.rng32, and the probe_* builders make inputs through which a kernel exposes one 32-wide block of one of its four
draws (forward; backward pass A; backward pass B for Pd and for dS) as the zero pattern of an output.
"""
import math
import zlib

import numpy as np
import torch

from gemm_check import TINY, U_ACC, U_BF16, _ranges
from noise_views_ref import rng32

C_ = 2.0
DH = 32
SCALE = 1.0 / math.sqrt(DH)
NEG = float('-inf')


# ------------------------------------------------------------------------------------------------ dropout decisions
def drop_threshold(p):
    """csrc/common.h drop_threshold: p arrives as a C float"""
    t = float(np.float32(p)) * 65536.0 + 0.5
    return 0xffff if t >= 65535.0 else int(t)


def drop_keep(seed, idx, thresh):
    """csrc/common.h drop_keep for an array of uint64 element indices -> bool array"""
    idx = np.asarray(idx, np.uint64)
    h = rng32(seed & 0xffffffff, idx >> np.uint64(1))
    bits = np.where((idx & np.uint64(1)).astype(bool), h >> np.uint32(16), h & np.uint32(0xffff))
    return bits >= np.uint32(thresh)


def keep_mask(seed, B, H, Lq, Lk, p):
    """the attention kernels' keep decisions [B, H, Lq, Lk] (bool): element index ((b H + h) Lq + i) Lk + j"""
    if p <= 0:
        return np.ones((B, H, Lq, Lk), bool)
    idx = np.arange(B * H * Lq * Lk, dtype=np.uint64)
    return drop_keep(seed, idx, drop_threshold(p)).reshape(B, H, Lq, Lk)


def inv_keep(p):
    """the kernels' 1 / (1 - p) factor: f32 arithmetic on the C float p"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------ layout
def heads(t, B, H, L):
    """[B L, >= H 32] row-major (any row stride) -> float64 [B, H, L, 32]"""
    return t[:, :H * DH].double().reshape(B, L, H, DH).permute(0, 2, 1, 3)


def rows(t):
    """[B, H, L, 32] -> [B L, H 32]"""
    B, H, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * DH)


# ------------------------------------------------------------------------------------------------ checker
def check(got, ref, bound, what=''):
    """every element of got finite and within bound of ref (same shapes, any leading dims; the last two are reported as rows / cols).
    Returns the largest error / bound ratio."""
    got = got.detach().double().cpu()
    ref, bound = ref.detach().double().cpu(), bound.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    if got.dim() == 1:
        got, ref, bound = got[:, None], ref[:, None], bound[:, None]
    g2, r2, b2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, got.shape[-1]), bound.reshape(-1, got.shape[-1])
    bad = ~torch.isfinite(g2)
    if bad.any():
        rr, cc = bad.nonzero(as_tuple=True)
        raise AssertionError(f'{what}: {int(bad.sum())} non-finite (unwritten?) elements, rows {_ranges(rr.tolist())}, cols {_ranges(cc.tolist())}')
    assert torch.isfinite(r2).all() and torch.isfinite(b2).all(), f'{what}: the reference is not finite (a fully masked row?)'
    ratio = (g2 - r2).abs() / b2
    worst = float(ratio.max())
    if worst > 1.0:
        bad = ratio > 1.0
        rr, cc = bad.nonzero(as_tuple=True)
        i, j = np.unravel_index(int(ratio.argmax()), tuple(ratio.shape))
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements over the bound (worst ratio {worst:.3g} at row {i} col {j}: '
                             f'got {float(g2[i, j]):.6g} ref {float(r2[i, j]):.6g}); rows {_ranges(rr.tolist())}; cols {_ranges(cc.tolist())}')
    return worst


# ------------------------------------------------------------------------------------------------ attention references
def _scores(q, k, kpm, amask):
    """q [B,H,Lq,32], k [B,H,Lk,32] float64; kpm bool [B,Lk] or None; amask float64 [Lq,Lk] or None -> s, sum_d |q||k| scale"""
    s = SCALE * (q @ k.transpose(-1, -2))
    if amask is not None:
        s = s + amask
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], NEG)
    return s, SCALE * (q.abs() @ k.abs().transpose(-1, -2))


def _eps(s, lse, absqk):
    live = torch.isfinite(s)
    d = torch.where(live, (s - lse[..., None]).abs(), torch.zeros_like(s))
    e = math.sqrt(DH) * U_ACC * absqk + 2.0 ** -22 * (2.0 + d)
    return torch.where(live, e, torch.zeros_like(e))


def attention_fwd_ref(q, k, v, kpm, amask, keep, p, u_p, u_out):
    """-> dict(o, lse, bound_o, bound_lse), [B,H,Lq,32] / [B,H,Lq].  keep: bool tensor [B,H,Lq,Lk]"""
    Lk = k.shape[2]
    s, absqk = _scores(q, k, kpm, amask)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    Pd = P * keep.double() / (1.0 - p)
    o = Pd @ v
    eps = _eps(s, lse, absqk)
    emax = eps.max(-1).values
    av = v.abs()
    bo = C_ * ((Pd * (u_p + eps + math.sqrt(Lk) * U_ACC)) @ av + (Pd @ av) * emax[..., None] + u_out * o.abs()) + TINY
    bl = C_ * (emax + 2.0 ** -23 * (1.0 + lse.abs()))
    return dict(o=o, lse=lse, bound_o=bo, bound_lse=bl, P=P, Pd=Pd)


def attention_bwd_ref(q, k, v, do, o_k, lse_k, kpm, amask, keep, p, u_p, u_out):
    """the kernel's own o_k [B,H,Lq,32] and lse_k [B,H,Lq] (float64) -> dict(dq, dk, dv, bound_dq, bound_dk, bound_dv, dP)"""
    Lq, Lk = q.shape[2], k.shape[2]
    s, absqk = _scores(q, k, kpm, amask)
    P = torch.exp(s - lse_k[..., None])
    kf = keep.double() / (1.0 - p)
    Pd = P * kf
    delta = (do * o_k).sum(-1)
    dP = kf * (do @ v.transpose(-1, -2))
    dS = P * (dP - delta[..., None])
    eps = _eps(s, lse_k, absqk)
    E = P * (dP.abs() + delta.abs()[..., None]) * (u_p + eps) + \
        P * math.sqrt(DH) * U_ACC * ((do.abs() @ v.abs().transpose(-1, -2)) * kf + (o_k.abs() * do.abs()).sum(-1)[..., None])
    dq = SCALE * (dS @ k)
    dk = SCALE * (dS.transpose(-1, -2) @ q)
    dv = Pd.transpose(-1, -2) @ do
    bq = C_ * (SCALE * (E @ k.abs()) + math.sqrt(Lk) * U_ACC * SCALE * (dS.abs() @ k.abs()) + u_out * dq.abs()) + TINY
    bk = C_ * (SCALE * (E.transpose(-1, -2) @ q.abs()) + math.sqrt(Lq) * U_ACC * SCALE * (dS.abs().transpose(-1, -2) @ q.abs()) +
               u_out * dk.abs()) + TINY
    bv = C_ * ((Pd * (u_p + eps)).transpose(-1, -2) @ do.abs() + math.sqrt(Lq) * U_ACC * (Pd.transpose(-1, -2) @ do.abs()) +
               u_out * dv.abs()) + TINY
    return dict(dq=dq, dk=dk, dv=dv, bound_dq=bq, bound_dk=bk, bound_dv=bv, dP=dP, P=P, dPraw=do @ v.transpose(-1, -2))


# ------------------------------------------------------------------------------------------------ attention emulation (torch, f32)
def _bf(t):
    return t.to(torch.bfloat16).float()


def attention_emulate(q, k, v, do, kpm, amask, keep, p, mfma_bf16, out_bf16, fault=None, mfma_bwd=None, o_in=None):
    """The kernels' rounding decisions in torch on any device: f32 scores / exponentials / accumulation, P and dS rounded to bf16 in
    front of the bf16 MFMA kernels' second products, outputs rounded to bf16.  Operands float64 [B,H,L,32] (already dtype-rounded).
    fault plants a numerics-only defect: 'last_key' (every clip's last live key is left out), 'scale' (1 / sqrt(33)), 'kpm' (the next clip's
    padding mask), 'heads' (V's heads 0 and 1 swapped).  mfma_bwd: the backward's family when it differs from the forward's
    (a generic backward behind an MFMA forward); o_in: the o handed to the backward instead of the forward's own (the dS probes
    pass zeros).  -> dict(o, lse, dq, dk, dv) float64"""
    f = torch.float32
    q, k, v, do = q.to(f), k.to(f), v.to(f), do.to(f)
    sc = np.float32(1.0 / math.sqrt(33.0 if fault == 'scale' else 32.0))
    if fault == 'kpm' and kpm is not None:
        kpm = torch.roll(kpm, 1, 0)
    if fault == 'heads':
        v = v.clone()
        v[:, [0, 1]] = v[:, [1, 0]]
    s = (q @ k.transpose(-1, -2)) * sc
    if amask is not None:
        s = s + amask.to(f)
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], NEG)
    if fault == 'last_key':                                          # each clip's last LIVE key
        s = s.clone()
        for b in range(s.shape[0]):
            s[b, ..., s.shape[-1] - 1 if kpm is None else int((~kpm[b]).nonzero()[-1])] = NEG
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    ssum = e.sum(-1, keepdim=True)
    lse = (m + torch.log(ssum)).squeeze(-1)
    kf = keep.to(f) * np.float32(inv_keep(p)) if p > 0 else keep.to(f)
    rnd = _bf if mfma_bf16 else (lambda t: t)
    o = (rnd(e * kf) @ v) / ssum                                     # the bf16 MFMA forward normalises the accumulator
    o_k = _bf(o) if out_bf16 else o
    if mfma_bwd is not None:
        rnd = _bf if mfma_bwd else (lambda t: t)
    P = torch.exp(s - lse[..., None])
    delta = (do * (o_k if o_in is None else o_in.to(f))).sum(-1, keepdim=True)
    dP = (do @ v.transpose(-1, -2)) * kf
    dS = P * (dP - delta)
    dq = (rnd(dS) @ k) * sc
    dk = (rnd(dS).transpose(-1, -2) @ q) * sc
    dv = rnd(P * kf).transpose(-1, -2) @ do
    ob = _bf if out_bf16 else (lambda t: t)
    return dict(o=o_k.double(), lse=lse.double(), dq=ob(dq).double(), dk=ob(dk).double(), dv=ob(dv).double())


# ------------------------------------------------------------------------------------------------ seeded inputs of a case row
def case_inputs(c):
    """the operands of a row of attn_cases.ATTN, on the CPU: float64 [B,H,L,32] tensors holding dtype-rounded values, the padding mask
    (bool [B,Lk] or None), the additive mask (float32 [Lq,Lk] or None), the dropout seed as (host seed, device word) and the keep
    mask.  Every (clip, head) has its own magnitude on v and dO (powers of 1.5 over a 7-cycle that neighbours never share), so a
    head or clip read from its neighbour is wrong by at least a third of the value."""
    import attn_cases
    B, H, Lq, Lk = c['B'], c['H'], c['Lq'], c['Lk']
    g = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    td = torch.bfloat16 if c['dt'] == 'bf16' else torch.float32

    def rnd(t):
        return t.to(td).double()
    bh = torch.arange(B)[:, None] * 3 + torch.arange(H)[None, :] * 5
    mag_v = (1.5 ** ((bh % 7) - 3).double())[:, :, None, None]
    mag_d = (1.5 ** (((bh + 4) % 7) - 3).double())[:, :, None, None]
    q = rnd(torch.randn(B, H, Lq, DH, generator=g, dtype=torch.float64) * c['gain'])
    k = rnd(torch.randn(B, H, Lk, DH, generator=g, dtype=torch.float64) * c['gain'])
    v = rnd(torch.randn(B, H, Lk, DH, generator=g, dtype=torch.float64) * mag_v)
    do = rnd(torch.randn(B, H, Lq, DH, generator=g, dtype=torch.float64) * mag_d)
    kpm = torch.tensor(attn_cases.kpm_pattern(c['kpm'], B, Lk)) if c['kpm'] else None
    amask = None
    if c['amask']:
        amask = (torch.rand(Lq, Lk, generator=g) * 6 - 3).float()
        dead = torch.rand(Lq, Lk, generator=g) < 0.25
        for b in range(B):                                  # every (clip, query) row keeps a live key: the clip's first unpadded one
            dead[:, 0 if kpm is None else int((~kpm[b]).nonzero()[0])] = False
        amask = amask.masked_fill(dead, NEG)
    seed = zlib.crc32(c['name'].encode()[::-1]) & 0x7fffffff
    word = 0x9e3779b1 ^ (seed >> 3)                          # the device word: host seed + word wraps past 2^32 for some rows
    keep = torch.from_numpy(keep_mask((seed + word) & 0xffffffff, B, H, Lq, Lk, c['p']))
    return dict(q=q, k=k, v=v, do=do, kpm=kpm, amask=amask, seed=seed, word=word, keep=keep)


# ------------------------------------------------------------------------------------------------ exact keep-mask probes
def probe_inputs(kind, B, H, Lq, Lk, t, gen):
    """float64 [B,H,L,32] operands (bf16-exact values) through which a kernel exposes block t of one keep draw:
      'fwd':  V = identity on keys [32t, 32t+32)         -> o[i][d]  = Pd[i][32t+d]
      'pd':   dO = identity on queries [32t, 32t+32)     -> dv[j][d] = Pd[32t+d][j]
      'passA': K = block identity, o = 0 (delta = 0)     -> dq[i][d] = scale P keep dP / (1-p) at key 32t+d
      'ds':   Q = block identity, o = 0                  -> dk[j][d] = the same at query 32t+d
    Magnitudes are small: |q_d|, |k_d| <= 1/2, so |s| <= 1.5 and every P >= e^-3 / Lk > 2^-20; in the two dS probes dO and V share a
    unit component in dimension 0 and are +-1/64 noise elsewhere, so every dP = dO . V lies in 1 +- 31/4096.  All values are
    bf16-exact."""
    def noise(L, amp):
        return (torch.randint(-8, 9, (B, H, L, DH), generator=gen).double() / 8.0) * amp      # multiples of amp / 8: bf16-exact
    def eye(L):
        m = torch.zeros(B, H, L, DH, dtype=torch.float64)
        for d in range(DH):
            if 32 * t + d < L:
                m[:, :, 32 * t + d, d] = 1.0
        return m
    q, k = noise(Lq, 0.5), noise(Lk, 0.5)
    v, do = noise(Lk, 1.0 / 64), noise(Lq, 1.0 / 64)
    if kind == 'fwd':
        v = eye(Lk)
    elif kind == 'pd':
        do = eye(Lq)
    else:
        # dP_ij = dO_i . V_j = 1 + noise: unit component in dimension 0, |noise terms| <= 31 / 64^2 + 2 / 64
        v[..., 0], do[..., 0] = 1.0, 1.0
        if kind == 'passA':
            k = eye(Lk)
        else:
            q = eye(Lq)
    return q, k, v, do


def probe_expected(kind, ref_f, ref_b, keep, t, Lq, Lk):
    """(float64 reference of the probed quantity [B,H,Lq,Lk block], the slice of keep it must reproduce) for the output the probe
    reads; block = columns (keys) [32t, 32t+32) for 'fwd' / 'passA', rows (queries) for 'pd' / 'ds'"""
    if kind in ('fwd', 'passA'):
        sl = slice(32 * t, min(32 * t + 32, Lk))
        val = ref_f['P'][..., sl] if kind == 'fwd' else (ref_f['P'] * ref_b['dPraw'])[..., sl]
        return val, keep[..., sl]
    sl = slice(32 * t, min(32 * t + 32, Lq))
    val = ref_f['P'][..., sl, :] if kind == 'pd' else (ref_f['P'] * ref_b['dPraw'])[..., sl, :]
    return val, keep[..., sl, :]


def probe_check(kind, got, keep_blk, val_blk, what=''):
    """got: the kernel output read as the probed block (same shape as keep_blk, float64); val_blk: the float64 value an element has
    when kept.  Every element of val_blk must be non-zero (so that no element is left out of the probe), then the zero pattern of
    got must equal the mask."""
    assert bool((val_blk != 0).all()), f'{what}: the probe has zero reference elements: they could not show their keep bit'
    nz = (got != 0).cpu().numpy()
    want = np.asarray(keep_blk, bool)
    assert nz.shape == want.shape, (what, nz.shape, want.shape)
    if (nz != want).any():
        bad = np.argwhere(nz != want)
        raise AssertionError(f'{what} [{kind}]: {len(bad)} keep decisions differ from drop_keep, first (b, h, i, j) = {bad[:4].tolist()}')


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd_ref(x, gamma, beta, add, u_out):
    """x [rows, D], gamma / beta [D], add or None (float64) -> dict(y, y2, mean, rstd, bound_*)"""
    D = x.shape[1]
    Lg = math.log2(D) + 2
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + 1e-5)
    xh = xc * rstd
    y = xh * gamma + beta
    e_mu = Lg * U_ACC * x.abs().mean(1, keepdim=True)
    madev = xc.abs().mean(1, keepdim=True)
    core = U_ACC * (8 * (xh * gamma).abs() + beta.abs()) + rstd * gamma.abs() * e_mu + 2 * (xh * gamma).abs() * e_mu * madev * rstd ** 2
    out = dict(y=y, mean=mu[:, 0], rstd=rstd[:, 0], bound_y=C_ * (u_out * y.abs() + core) + TINY, bound_mean=C_ * e_mu[:, 0] + TINY,
               bound_rstd=(C_ * rstd * (2 * e_mu * madev * rstd ** 2 + 0.5 * (e_mu * rstd) ** 2 + 8 * U_ACC))[:, 0], y2=None, bound_y2=None)
    if add is not None:
        out['y2'] = y + add
        out['bound_y2'] = C_ * (u_out * out['y2'].abs() + core + U_ACC * out['y2'].abs()) + TINY
    return out


def layernorm_bwd_ref(dy, dy2, x, gamma, mean_k, rstd_k, dres, dres2, u_out):
    """the kernel's own mean_k / rstd_k [rows] (float64) -> dict(dx, dgamma, dbeta, bound_*)"""
    n, D = x.shape
    Lg = math.log2(D) + 2
    rs = rstd_k[:, None]
    xh = (x - mean_k[:, None]) * rs
    dyt = dy if dy2 is None else dy + dy2
    a = dyt * gamma
    c1, c2 = a.mean(1, keepdim=True), (a * xh).mean(1, keepdim=True)
    dx = rs * (a - c1 - xh * c2)
    res = torch.zeros_like(dx)
    for r in (dres, dres2):
        if r is not None:
            dx = dx + r
            res = res + r.abs()
    bdx = C_ * (u_out * dx.abs() + Lg * U_ACC * rs * (a.abs() + a.abs().mean(1, keepdim=True) + xh.abs() * (a * xh).abs().mean(1, keepdim=True)) +
                U_ACC * res) + TINY
    k = C_ * (math.sqrt(n) + 4) * U_ACC
    return dict(dx=dx, dgamma=(dyt * xh).sum(0), dbeta=dyt.sum(0), bound_dx=bdx, bound_dgamma=k * (dyt * xh).abs().sum(0) + TINY,
                bound_dbeta=k * dyt.abs().sum(0) + TINY)


def layernorm_emulate(x, gamma, beta, add, dy, out_bf16):
    """torch f32 emulation of ln_fwd_kernel / ln_bwd_kernel (no residuals): -> dict(y, y2, mean, rstd, dx, dgamma, dbeta) float64"""
    f = torch.float32
    D = x.shape[1]
    x32, g, b, d = x.to(f), gamma.to(f), beta.to(f), dy.to(f)
    mu = x32.sum(1, keepdim=True) * np.float32(1.0 / D)
    xc = x32 - mu
    rs = torch.rsqrt((xc * xc).sum(1, keepdim=True) * np.float32(1.0 / D) + np.float32(1e-5))
    o = xc * rs * g + b
    ob = _bf if out_bf16 else (lambda t: t)
    xh = xc * rs
    a = d * g
    c1, c2 = a.sum(1, keepdim=True) * np.float32(1.0 / D), (a * xh).sum(1, keepdim=True) * np.float32(1.0 / D)
    dx = rs * (a - c1 - xh * c2)
    return dict(y=ob(o).double(), y2=None if add is None else ob(o + add.to(f)).double(), mean=mu[:, 0].double(), rstd=rs[:, 0].double(),
                dx=ob(dx).double(), dgamma=(d * xh).sum(0).double(), dbeta=d.sum(0).double())
