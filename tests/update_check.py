"""Float64 references, derived error bounds, exact checks and float32 restatements for the kernels that write the trained weights
(csrc/misc.hip: multi_sumsq / sumsq_final, multi_adamw, multi_ema, multi_gather, and the single-tensor sumsq_partial / adamw_clip).
A helper of tests/test_update_envelope_gpu.py and tests/test_update_check_cpu.py, not a conftest.  Everything here is numpy on the
host; the rows are in tests/update_cases.py.

A row lives in ONE byte image (Layout): every tensor of every chunk, the partial sums, sumsq[0] and the step / guard / seed words are
slots of a NaN-filled buffer, each with GUARD elements before and after and at the byte offset from a 16-byte boundary that the row
asks for.  The GPU module uploads the image, launches, and reads it back; the CPU module lets the float32 restatements below write into
it.  The checker sees only the image before and the image after, so a store outside a tensor, an unwritten tail or a NaN left inside
shows whatever made it.

All references are float64 on the exact float32 / bf16 operand values; hyper-parameters enter as the float32 values the ABI carries,
the 1e-6 of the clip coefficient as float32(1e-6).  u = 2^-24 is the unit roundoff of one correctly rounded f32 operation; a division
or a square root is charged 2 u (one ulp: the bounds do not rely on the compiler's correctly-rounded option).  Every bound is
c k u (sum of the magnitudes of the terms) + TINY; k counts the roundings without any multiply-add contraction, and contraction only
removes roundings, so the count holds either way; c = 2 as in tests/gemm_check.py, so that a result whose roundings all fall the same
way sits at ratio 0.5 and an honest float32 restatement cannot come nearer its bound than that.  The formulas below are written
without c; the bias-correction term d1 + d2 / 2 is taken as it stands.

sumsq        a sum of n non-negative squares.  Whatever the order, a term's error is at most (number of additions it passes through
             + 1 for its own product) u times the total, to first order.  One chunk: a lane serially adds at most ceil(n / 256) scalar
             terms, or - vector paths - at most 8 products per 16-byte load over ceil(n / 2048) loads, 3 additions inside a float4's
             expression, 2 to combine the four accumulators of the loads-in-flight loop, 1 tail element: never more than
             ceil(n / 256) + 8; then 6 steps of the wave reduction and 3 additions of the four wave partials:
                 k_part(n) = ceil(n / 256) + 8 + 6 + 3 + 1 = ceil(n / 256) + 18          |partial_i - S_i| <= k_part(n_i) u S_i
             The final pass adds ceil(nparts / 256) partials per lane, then 6 + 3:  k_final = ceil(nparts / 256) + 9 and
                 |sumsq[0] - S| <= sum_i k_part(n_i) u S_i + k_final u S
             sedt_sumsq: parts = min(1024, ceil(n / 2048)) workgroups grid-stride, ceil(n / (256 parts)) terms per lane:
                 k = ceil(n / (256 parts)) + 10 + k_final(parts);  accumulate adds u |old + S| for its one addition.
clip coef    coef = min(1, max_norm / (sqrt(s) + 1e-6f)) from the KERNEL'S OWN s = sumsq[0]: sqrt 2 u, add 1 u, divide 2 u:
             relative error 5 u; the clamp is exact.  A row whose norm is below max_norm must equal the unclipped launch bit for bit.
AdamW, by stage (the slab suite's way): m' and v' from the inputs and coef, p' from the kernel's own m' and v'.
             gr = g coef: 6 u |gr|.
             m' = m + (gr - m)(1 - b1): the subtraction u (|gr| + |m|), the product with 1 - b1 (itself one rounding) 2 u, the
             addition u |m'|, and 6 u |gr| carried in:  |m' - ref| <= 9 u (|m| + (1 - b1)(|gr| + |m|))
             v' = v b2 + gr gr (1 - b2): v b2 1 u; gr gr carries 12 u and rounds once, times (1 - b2) two more (15 u), the addition 1 u:
                 |v' - ref| <= 16 u (v b2 + gr^2 (1 - b2))
             p' = p (1 - lr wd) - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps)) = A - B.  A: lr wd, the subtraction from 1 and the
             product: 3 u max(1, |decay|) |p|.  B: with d1, d2 the relative errors of bc1 = 1 - powf(b1, t), bc2 = 1 - powf(b2, t),
                 d(b) = (POW_ULP b^t + 1) u / (1 - b^t)             (powf within POW_ULP units of u of b^t, one rounding of 1 - x)
             lr / bc1: d1 + 2 u; sqrt(v') 2 u, sqrt(bc2) d2 / 2 + 2 u, their quotient 2 u, + eps 1 u, m' / denominator 2 u, the
             product 1 u: B carries d1 + d2 / 2 + 12 u; the final subtraction u |p'| <= u (|A| + |B|):
                 |p' - ref| <= 4 u max(1, |decay|) |p| + (13 u + d1 + d2 / 2) |B|
             lr = 0 makes B exactly 0 and decay exactly 1: p must keep its bits, which is asserted apart from the bound.
             POW_ULP = 2: ROCm's installed documentation states no accuracy for device powf (searched for under the ROCm tree, not
             found), so the fallback of 2 is used; a float32 restatement on the CPU stays below 1.
             sedt_adamw_clip forms the two corrections on the host with the C library's powf: the same bound.
EMA          shadow' = (1 - d) p + d shadow: 1 - d one rounding, two products, one addition:
                 |shadow' - ref| <= 3 u (|(1 - d) p| + |d shadow|)
gather       no bound: modes 0 / 1 are an f32 copy / one f32 addition, modes 2 / 3 round src / float(old) + src (one f32 addition) to
             bf16, nearest even: every one of them has exactly one IEEE result, compared bit for bit.

The float32 restatements (emulate_*) redo each kernel in numpy float32 and can plant the faults of FAULTS; tests/test_update_check_cpu.py
shows that the honest ones stay at or below half of every bound and that each fault fails the checker.
"""
import math
import zlib

import numpy as np

U = 2.0 ** -24
TINY = 1e-30
POW_ULP = 2.0
C_ = 2.0
GUARD = 32                      # guard elements on each side of every slot (>= 16; a multiple of 16 bytes for either element size)
F = np.float32
EPS_CLIP = float(F(1e-6))

FAULTS = ('tail_unwritten', 'past_n', 'wd_after', 'coef_unclamped', 'eps_inside', 'step_minus_1', 'swap_mv', 'lr_next',
          'bf16_wrong_half', 'ema_swapped', 'gather_trunc', 'gather_overwrite', 'sumsq_drop_tail')

WORDS = ('partial', 'sumsq', 'step', 'guard', 'seed')


# ------------------------------------------------------------------------------------------------ bf16
def bf2f(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f2bf(x):
    """round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def f2bf_trunc(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ layout
def fields(case):
    """{field: (element size of chunk ch, written by the kernel)}"""
    k = case['kind']
    if k == 'adamw':
        return {'p': (lambda ch: 4, True), 'g': (lambda ch: 2 if ch['bf'] else 4, False), 'm': (lambda ch: 4, True), 'v': (lambda ch: 4, True)}
    if k == 'sumsq':
        return {'g': (lambda ch: 2 if ch['bf'] else 4, False)}
    if k == 'ema':
        return {'p': (lambda ch: 4, False), 'm': (lambda ch: 4, True)}
    if k == 'gather':
        return {'p': (lambda ch: 2 if ch['bf'] else 4, True), 'g': (lambda ch: 4, False)}
    raise KeyError(k)


_OFF = {'p': 0, 'g': 1, 'm': 2, 'v': 3}


class Layout(object):
    """where every slot of a row lives in its image: slots[(chunk index or word name, field)] = (first byte, elements, element size)"""

    def __init__(self, case):
        self.case, self.slots, self.nbytes = case, {}, 0
        fl = fields(case)
        for ci, ch in enumerate(case['chunks']):
            for f, (es, _) in fl.items():
                self._add((ci, f), ch['n'], es(ch), ch['off'][_OFF[f]])
        for w in WORDS:
            self._add((w, 'w'), len(case['chunks']) if w == 'partial' else 1, 4, 0)
        self.writable = [(ci, f) for ci in range(len(case['chunks'])) for f, (_, wr) in fl.items() if wr]
        self.readonly = [(ci, f) for ci in range(len(case['chunks'])) for f, (_, wr) in fl.items() if not wr]

    def _add(self, key, n, es, off):
        assert off % es == 0 and 0 <= off < 16
        base = (self.nbytes + 15) // 16 * 16
        start = base + GUARD * es + off
        self.slots[key] = (start, n, es, base)
        self.nbytes = start + (n + GUARD) * es

    def blank(self):
        """the NaN fill: 0x7fc00000 over f32 regions, 0x7fc0 over bf16 regions"""
        img = np.zeros((self.nbytes + 15) // 16 * 16, np.uint8)
        for (start, n, es, base) in self.slots.values():
            end = start + (n + GUARD) * es
            lo = base + (start - base) % es
            if es == 4:
                img[lo:lo + (end - lo) // 4 * 4].view(np.uint32)[:] = 0x7fc00000
            else:
                img[lo:lo + (end - lo) // 2 * 2].view(np.uint16)[:] = 0x7fc0
        return img

    def addr(self, key):
        return self.slots[key][0]

    def bits(self, img, key):
        start, n, es, _ = self.slots[key]
        return img[start:start + n * es].view(np.uint32 if es == 4 else np.uint16)

    def get(self, img, key):
        """the slot's values as float32 (a copy)"""
        start, n, es, _ = self.slots[key]
        b = self.bits(img, key)
        return b.view(np.float32).copy() if es == 4 else bf2f(b)

    def put(self, img, key, arr):
        """float32 values (rounded to nearest even into a bf16 slot) or raw integer bits"""
        start, n, es, _ = self.slots[key]
        arr = np.asarray(arr)
        if arr.dtype.kind in 'ui':
            self.bits(img, key)[:] = arr.astype(np.uint32 if es == 4 else np.uint16)
        elif es == 4:
            self.bits(img, key)[:] = np.ascontiguousarray(arr, np.float32).view(np.uint32)
        else:
            self.bits(img, key)[:] = f2bf(arr)

    def word(self, img, name):
        return self.bits(img, (name, 'w')).view(np.int32 if name in ('step', 'guard') else np.uint32 if name == 'seed' else np.float32)

    def data_mask(self, keys):
        m = np.zeros((self.nbytes + 15) // 16 * 16, bool)
        for k in keys:
            start, n, es, _ = self.slots[k]
            m[start:start + n * es] = True
        return m


# ------------------------------------------------------------------------------------------------ inputs
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_image(case, lay, step_before=None, guard=0, seed=0x12345678):
    """the row's operands written into a blank image.  Gradients: gscale N(0, 1) with the LAST element of every chunk at 4 gscale, so
    that a lost tail moves the norm; moments: zero or of the gradients' scale; partial and sumsq[0] keep their NaN fill (the kernels
    must write them before anyone reads them)"""
    rng, img, k = _rng(case['name']), lay.blank(), case['kind']
    for ci, ch in enumerate(case['chunks']):
        n = ch['n']
        if k in ('adamw', 'sumsq'):
            gs = case['gscale']
            g = (gs * rng.standard_normal(n)).astype(F)
            g[-1] = F(4 * gs)
            lay.put(img, (ci, 'g'), g)
        if k == 'adamw':
            ms = case['gscale'] if case['gscale'] > 0 else 1.0
            p = rng.standard_normal(n).astype(F)
            p[::7] *= F(1e-3)                                   # some weights near zero: the update term shows there
            lay.put(img, (ci, 'p'), p)
            nz = case['moments'] == 'nonzero'
            lay.put(img, (ci, 'm'), (0.1 * ms * rng.standard_normal(n)).astype(F) if nz else np.zeros(n, F))
            lay.put(img, (ci, 'v'), ((0.1 * ms * rng.standard_normal(n)) ** 2).astype(F) if nz else np.zeros(n, F))
        if k == 'ema':
            lay.put(img, (ci, 'p'), rng.standard_normal(n).astype(F))
            lay.put(img, (ci, 'm'), rng.standard_normal(n).astype(F))
        if k == 'gather':
            src = rng.standard_normal(n).astype(F)
            hb = src[::5].view(np.uint32)                        # every fifth value lies exactly halfway between two bf16 numbers,
            src[::5] = ((hb & np.uint32(0xffff0000)) | np.uint32(0x8000)).view(F)       # with either parity of the kept mantissa
            lay.put(img, (ci, 'g'), src)
            old = rng.standard_normal(n).astype(F)
            old[::10] = 0                                       # ... and stays halfway after the accumulate modes' addition
            lay.put(img, (ci, 'p'), old)
    if step_before is None:
        step_before = case.get('step', 1) - (1 if case.get('max_norm') is not None else 0)
    lay.word(img, 'step')[0] = step_before
    lay.word(img, 'guard')[0] = guard
    lay.word(img, 'seed')[0] = seed
    return img


def hyper32(case):
    from update_cases import BETAS, EPS
    return dict(b1=F(BETAS[0]), b2=F(BETAS[1]), eps=F(EPS))


# ------------------------------------------------------------------------------------------------ float64 references and bounds
def ratio(got, ref, bound, what):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), f'{what}: a non-finite element inside the tensor'
    err = np.abs(got - ref)
    r = err / bound
    worst = float(r.max()) if r.size else 0.0
    assert worst <= 1.0, f'{what}: error / bound = {worst:.3g} at element {int(r.argmax())} (got {got.ravel()[r.argmax()]!r}, ' \
                         f'reference {np.asarray(ref).ravel()[r.argmax()]!r}, bound {np.asarray(bound).ravel()[r.argmax()]:.3g})'
    return worst


def k_part(n):
    return -(-n // 256) + 18


def k_final(nparts):
    return -(-nparts // 256) + 9


def sumsq_check(gs, partial, sumsq, what):
    """gs: the chunks' gradients (float32 values); partial [nchunks] and sumsq (scalar) as the kernels wrote them"""
    S = np.array([np.sum(np.asarray(g, np.float64) ** 2) for g in gs])
    kp = np.array([k_part(len(g)) for g in gs], np.float64)
    out = {}
    if partial is not None:
        out['multi_sumsq partial'] = ratio(partial, S, C_ * kp * U * S + TINY, f'{what} partial')
    out['multi_sumsq sumsq'] = ratio([sumsq], [S.sum()], [C_ * (np.sum(kp * U * S) + k_final(len(gs)) * U * S.sum()) + TINY], f'{what} sumsq[0]')
    return out


def sumsq1_check(g, got, old, accumulate, what):
    n = len(g)
    parts = min(1024, max(1, -(-n // 2048)))
    S = float(np.sum(np.asarray(g, np.float64) ** 2))
    ref = S + (float(old) if accumulate else 0.0)
    k = -(-n // (256 * parts)) + 10 + k_final(parts)
    return {'sumsq' + (' accumulate' if accumulate else ''): ratio([got], [ref], [C_ * (k * U * S + (U * abs(ref) if accumulate else 0.0)) + TINY], what)}


def clip_coef(sumsq, max_norm):
    """(float64 coefficient from the kernel's own float32 sumsq[0], its relative error)"""
    if max_norm is None or not float(F(max_norm)) > 0.0:
        return 1.0, 0.0
    c = float(F(max_norm)) / (math.sqrt(float(F(sumsq))) + EPS_CLIP)
    return min(c, 1.0), 5 * U


def pow_term(b, t):
    bt = float(b) ** t
    return (POW_ULP * bt + 1.0) * U / (1.0 - bt)


def adamw_check(x, got, lr, wd, hp, coef, step, what):
    """x / got: dicts of float32 arrays p, g, m, v before and p, m, v after; returns the three ratios"""
    lr, wd, b1, b2, eps = (float(F(a)) for a in (lr, wd, hp['b1'], hp['b2'], hp['eps']))
    cf, _ = coef
    p, g, m, v = (np.asarray(x[k], np.float64) for k in 'pgmv')
    gr = g * cf
    ob1, ob2 = 1.0 - b1, 1.0 - b2
    m_ref = m + (gr - m) * ob1
    v_ref = v * b2 + gr * gr * ob2
    out = {}
    out['m'] = ratio(got['m'], m_ref, C_ * 9 * U * (np.abs(m) + ob1 * (np.abs(gr) + np.abs(m))) + TINY, f'{what} m')
    out['v'] = ratio(got['v'], v_ref, C_ * 16 * U * (v * b2 + gr * gr * ob2) + TINY, f'{what} v')
    mk, vk = np.asarray(got['m'], np.float64), np.asarray(got['v'], np.float64)
    assert np.all(vk >= 0), f'{what}: a negative second moment'
    decay = 1.0 - lr * wd
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    B = (lr / bc1) * (mk / (np.sqrt(vk) / math.sqrt(bc2) + eps))
    p_ref = p * decay - B
    d = pow_term(b1, step) + 0.5 * pow_term(b2, step)
    out['p'] = ratio(got['p'], p_ref, C_ * 4 * U * max(1.0, abs(decay)) * np.abs(p) + (C_ * 13 * U + d) * np.abs(B) + TINY, f'{what} p')
    if lr == 0.0:
        assert np.array_equal(np.asarray(got['p'], F).view(np.uint32), np.asarray(x['p'], F).view(np.uint32)), f'{what}: lr = 0 changed p'
    return out


def ema_check(p, sh, got, decay, what):
    d = float(F(decay))
    p, sh = np.asarray(p, np.float64), np.asarray(sh, np.float64)
    a, b = (1.0 - d) * p, d * sh
    return ratio(got, a + b, C_ * 3 * U * (np.abs(a) + np.abs(b)) + TINY, what)


def gather_ref_bits(src, old_bits, mode):
    """the one IEEE result of every mode, as bits (uint32 for an f32 destination, uint16 for bf16)"""
    src = np.ascontiguousarray(src, F)
    if mode == 0:
        return src.view(np.uint32)
    if mode == 1:
        return (old_bits.view(F) + src).view(np.uint32)
    if mode == 2:
        return f2bf(src)
    return f2bf(bf2f(old_bits) + src)


# ------------------------------------------------------------------------------------------------ whole-row checks on images
def check_image_frame(lay, before, after, what, untouched=()):
    """the exact checks every row shares: nothing outside the written tensors changed (guards, read-only operands, words the launch
    does not own); `untouched`: further keys that must keep their bits"""
    own = list(lay.writable) + [(w, 'w') for w in WORDS if w not in untouched]
    own = [k for k in own if k not in untouched]
    mask = lay.data_mask(own)
    bad = np.flatnonzero((before != after) & ~mask)
    if bad.size:
        b = int(bad[0])
        near = [k for k, (s, n, es, base) in lay.slots.items() if base <= b < s + (n + GUARD) * es]
        raise AssertionError(f'{what}: byte {b} outside the written tensors changed (slot {near}, tensor bytes '
                             f'{lay.slots[near[0]][0] if near else None}..)')


def check_row(case, lay, before, after):
    """every check of one row: returns {kernel output: largest error / bound}"""
    k, what, out = case['kind'], case['name'], {}
    chunks = case['chunks']
    if k == 'sumsq' or (k == 'adamw' and case['max_norm'] is not None):
        gs = [lay.get(before, (ci, 'g')) for ci in range(len(chunks))]
        out.update(sumsq_check(gs, lay.word(after, 'partial'), lay.word(after, 'sumsq')[0], what))
    if k == 'sumsq':
        check_image_frame(lay, before, after, what)
    elif k == 'adamw':
        clipped = case['max_norm'] is not None
        check_image_frame(lay, before, after, what, untouched=() if clipped else WORDS)
        assert lay.word(after, 'step')[0] == case['step'], f'{what}: step word'
        coef = clip_coef(lay.word(after, 'sumsq')[0], case['max_norm']) if clipped else (1.0, 0.0)
        hp = hyper32(case)
        for ci, ch in enumerate(chunks):
            x = {f: lay.get(before, (ci, f)) for f in 'pgmv'}
            got = {f: lay.get(after, (ci, f)) for f in 'pmv'}
            for f, r in adamw_check(x, got, ch['lr'], ch['wd'], hp, coef, case['step'], f"{what} {ch['tag']}").items():
                out['multi_adamw ' + f] = max(out.get('multi_adamw ' + f, 0.0), r)
    elif k == 'ema':
        check_image_frame(lay, before, after, what, untouched=WORDS)
        r = 0.0
        for ci, ch in enumerate(chunks):
            r = max(r, ema_check(lay.get(before, (ci, 'p')), lay.get(before, (ci, 'm')), lay.get(after, (ci, 'm')), case['decay'],
                                 f"{what} {ch['tag']}"))
        out['multi_ema shadow'] = r
    elif k == 'gather':
        check_image_frame(lay, before, after, what, untouched=WORDS)
        for ci, ch in enumerate(chunks):
            got = lay.bits(after, (ci, 'p'))
            assert np.all(np.isfinite(lay.get(after, (ci, 'p')))), f"{what} {ch['tag']}: a non-finite element inside the tensor"
            ref = gather_ref_bits(lay.get(before, (ci, 'g')), lay.bits(before, (ci, 'p')), case['mode'])
            bad = np.flatnonzero(got != ref)
            assert bad.size == 0, f"{what} {ch['tag']}: element {int(bad[0]) if bad.size else -1} differs from the exact result " \
                                  f"({bad.size} of {ch['n']})"
        out[f"multi_gather mode {case['mode']} (exact)"] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ float32 restatements
def _lanes_sum(terms):
    """256 lanes take the terms in strides and add serially; a 64-lane butterfly; the four wave partials in order"""
    t = np.zeros(-(-max(len(terms), 1) // 256) * 256, F)
    t[:len(terms)] = terms
    acc = np.zeros(256, F)
    for row in t.reshape(-1, 256):
        acc = acc + row
    w = acc.reshape(4, 64)
    s = 32
    while s:
        w = w[:, :s] + w[:, s:2 * s]
        s //= 2
    return F(F(F(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def _f32_sum(terms, order):
    terms = np.asarray(terms, F)
    if order == 'lanes':
        return _lanes_sum(terms)
    return F(np.sum(terms, dtype=F)) if len(terms) else F(0)          # numpy's pairwise order


def emulate_sumsq(case, lay, img, order='lanes', fault=None):
    """multi_sumsq + sumsq_final on the image (the step / guard / seed words included)"""
    out = img.copy()
    parts = []
    for ci, ch in enumerate(case['chunks']):
        g = lay.get(img, (ci, 'g'))
        if fault == 'sumsq_drop_tail':
            g = g[:len(g) & ~3]
        parts.append(_f32_sum(g * g, order))
    parts = np.asarray(parts, F)
    lay.word(out, 'partial')[:] = parts
    tot = _f32_sum(parts, order)
    lay.word(out, 'sumsq')[0] = tot
    if not tot <= F(3.0e38):
        lay.word(out, 'guard')[0] = 1
    if not lay.word(out, 'guard')[0]:
        lay.word(out, 'step')[0] += 1
    lay.word(out, 'seed')[0] += 1
    return out


def _adamw_f32(p, g, m, v, lr, wd, hp, coef, step, fault=None):
    one = F(1)
    lr, wd, b1, b2, eps, coef = F(lr), F(wd), hp['b1'], hp['b2'], hp['eps'], F(coef)
    st = F(step - 1 if fault == 'step_minus_1' else step)
    with np.errstate(all='ignore'):
        bc1 = one - np.power(b1, st)
        bc2s = np.sqrt(one - np.power(b2, st))
        decay, slr = one - lr * wd, lr / bc1
        gr = g * coef
        m2 = m + (gr - m) * (one - b1)
        v2 = v * b2 + gr * gr * (one - b2)
        den = np.sqrt(v2 + eps) / bc2s if fault == 'eps_inside' else np.sqrt(v2) / bc2s + eps
        if fault == 'wd_after':
            p2 = (p - slr * (m2 / den)) * decay
        else:
            p2 = p * decay - slr * (m2 / den)
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return p2, m2, v2


def emulate_adamw(case, lay, img, order='lanes', fault=None):
    """(multi_sumsq when the row clips, then) multi_adamw on the image"""
    clipped = case['max_norm'] is not None
    out = emulate_sumsq(case, lay, img, order) if clipped else img.copy()
    coef = F(1)
    if clipped:
        coef = F(case['max_norm']) / (np.sqrt(lay.word(out, 'sumsq')[0]) + F(1e-6))
        if fault != 'coef_unclamped':
            coef = min(coef, F(1))
    hp, chunks = hyper32(case), case['chunks']
    step = int(lay.word(out, 'step')[0])
    victim = next((ci for ci, ch in enumerate(chunks) if ch['n'] > 8), 0)
    for ci, ch in enumerate(chunks):
        p, g, m, v = (lay.get(img, (ci, f)) for f in 'pgmv')
        lr = chunks[(ci + 1) % len(chunks)]['lr'] if fault == 'lr_next' else ch['lr']
        if fault == 'bf16_wrong_half' and ch['bf']:
            g = g[np.minimum(np.arange(len(g)) ^ 1, len(g) - 1)]
        if fault == 'swap_mv' and ci == victim:
            m, v = v, m
        p2, m2, v2 = _adamw_f32(p, g, m, v, lr, ch['wd'], hp, coef, step, fault)
        if fault == 'swap_mv' and ci == victim:
            m2, v2 = v2, m2
        for f, a in (('p', p2), ('m', m2), ('v', v2)):
            lay.put(out, (ci, f), a)
    return out


def emulate_ema(case, lay, img, fma=False, fault=None):
    out = img.copy()
    d = F(case['decay'])
    om = F(1) - d
    if fault == 'ema_swapped':
        d, om = om, d
    for ci in range(len(case['chunks'])):
        p, sh = lay.get(img, (ci, 'p')), lay.get(img, (ci, 'm'))
        if fma:                     # om * p + (d * sh) contracted: the first product enters the addition unrounded
            r = (np.float64(om) * p.astype(np.float64) + (d * sh).astype(np.float64)).astype(F)
        else:
            r = om * p + d * sh
        lay.put(out, (ci, 'm'), r)
    return out


def emulate_gather(case, lay, img, fault=None):
    out, mode = img.copy(), case['mode']
    for ci in range(len(case['chunks'])):
        src, old = lay.get(img, (ci, 'g')), lay.get(img, (ci, 'p'))
        acc = bool(mode & 1) and fault != 'gather_overwrite'
        val = (old + src) if acc else src
        if mode & 2:
            lay.put(out, (ci, 'p'), f2bf_trunc(val) if fault == 'gather_trunc' else f2bf(val))
        else:
            lay.put(out, (ci, 'p'), val)
    return out


def emulate(case, lay, img, fault=None, **kw):
    fn = {'adamw': emulate_adamw, 'sumsq': emulate_sumsq, 'ema': emulate_ema, 'gather': emulate_gather}[case['kind']]
    out = fn(case, lay, img, fault=fault if fault not in ('tail_unwritten', 'past_n') else None, **kw)
    if fault in ('tail_unwritten', 'past_n'):
        chunks = case['chunks']
        ci = next(i for i, ch in enumerate(chunks) if ch['n'] & 3 and ch['n'] > 4)
        for key in (k for k in lay.writable if k[0] == ci):
            start, n, es, _ = lay.slots[key]
            if fault == 'tail_unwritten':
                lo = start + (n & ~3) * es
                out[lo:start + n * es] = img[lo:start + n * es]
            else:
                out[start + n * es:start + (n + 1) * es] = out[start:start + es]          # one element past n
    return out
