"""References, bounds, np.float32 restatements and planted faults for the weight-preparation kernels and the split-K finishing pass
(csrc/misc.hip: multi_pack_kernel / pack_tile / pack_tile_vec, pack_conv_kernel, bn_fold_kernel / multi_bn_fold_kernel, stem_prep_kernel,
stem_conv0_grad_kernel, multi_wgrad_reduce_kernel; csrc/enc_slab.hip: pack_frag_kernel).  A helper of tests/test_prep_envelope_gpu.py and
tests/test_prep_check_cpu.py, not a conftest; the rows are in tests/prep_cases.py.  The guard frames, exact(), bounded(), k_measure(), the
bf16 conversions, gain() / sign() and the Kernel / register / restated(fault=...) pattern are those of tests/glue_check.py; this module
keeps its own registry (KERNELS) so that each CPU module's table test sees its own keys.

Exact kernels (compared on bits with the restatement, and with float64 under the bound, so that a mistake in the restatement shows):
  * pack (sedt_multi_pack, sedt_pack_conv): the forward image is T(w), the dgrad image T(float32(w * bnscale[co])), T the conversion to
    the compute dtype (round to nearest even for bf16): a transposition, at most one f32 multiply and one rounding.  Planted in every
    scaled row: products whose f32 rounding lands on a bf16 tie, so that the image differs from a single rounding of the float64 product
    (double_rounding_w()): a fused or reordered rounding shows.
  * frag (sedt_pack_frag): a permutation, and for an f32 master one rounding to bf16.
  * reduce (sedt_multi_wgrad_reduce, sedt_wgrad_reduce, sedt_wgrad_reduce_bias): the summation order of every mode is fixed by the code -
    mode 0: four sums over the slices 1.., s0 started from slice 0 and taking the tail, (s0 + s1) + (s2 + s3); mode 3: four thread groups
    z = g, g + 8, .. and g + 4, g + 12, .., per group s0 + s1, then (g0 + g1) + (g2 + g3); mode 1: v from slice 0 over the odd slices and
    the tail, u over the even ones, (v + u) * scale; mode 2: one chain from 0.f; the riding column sums: four groups x four sums, tail
    into the first - and one multiply by the row scale follows the sum.  Against float64: c sqrt(splitk) 2^-24 sum|slices| (|row scale|).
Bounded kernels (rsqrtf, and sums the compiler may contract into FMAs):
  * bn_fold (sedt_bn_fold, sedt_multi_bn_fold): scale within c (k_rsqrt 2^-24) |ref|, bias within c 2^-24 (|b| + (2 + k_rsqrt) |rm sc|);
    the reference adds float64(float32(1e-5)), the constant the kernel adds.
  * stem_prep: columns 0..48 and 64..112 under the house form with K = 3 (+ u_out |ref|), the other columns exactly +0.
  * stem_conv0_grad: K = 64 * 49.
K_FN['rsqrt']: the largest |scale - ref| / (2^-24 |ref|) measured on the device (glue_check.k_measure over the bn_fold rows; the figure
books the add's and the multiply's roundings on the function as well), times four, rounded up to a power of two.
Measured on MI355X (gfx950, ROCm 7 hipcc): 1.88 (the np.float32 restatement, with numpy's sqrt and a division, sits at 1.67) -> 8.
"""
import functools

import numpy as np

import glue_check as G
from glue_check import F, Frame, Kernel, bits, bounded, exact, from_bf16, gain, k_measure, rng_of, sign, store, to_bf16, val

K_FN = dict(rsqrt=8.0)          # measured on MI355X: 1.88; four times that, rounded up to a power of two
KERNELS = {}
register = functools.partial(G.register, table=KERNELS)
EPS32 = np.float32(1e-5)


def restated(key, c, fault=None):
    return G.restated(key, c, fault, table=KERNELS)


def verify_row(key, c, inp, fr, imgs):
    return G.verify_row(key, c, inp, fr, imgs, table=KERNELS)


def finite_specials():
    """glue_check.cast_specials() without the infinities and the NaN (their products' payloads are not the kernels' business): both kinds
    of bf16 tie, +-0, an f32 subnormal, the largest finite f32 (rounds to bf16 infinity), one f32 ulp on either side of a tie"""
    sp = G.cast_specials()
    return sp[np.isfinite(sp)]


def bf16_once(x):
    """a float64 scalar -> bf16 bits with ONE rounding to nearest even"""
    b = int(to_bf16(np.array([x], F))[0])
    return min((b - 1, b, b + 1), key=lambda u: (abs(float(from_bf16(np.array([u], np.uint16))[0]) - float(x)), u & 1))


def double_rounding_w(s):
    """an f32 w whose product with the f32 s rounds (in f32) onto a bf16 tie from the far side: bf16(f32(w s)) differs from bf16(w s)"""
    s = F(s)
    for k in range(64):
        tie = np.array([0x3F808000 + (k << 16)], np.uint32).view(F)[0]          # upper halves alternate even / odd
        w0 = np.array([np.float64(tie) / np.float64(s)], np.float64).astype(F)
        for d in (0, 1, -1, 2, -2, 3, -3):
            w = (w0.view(np.int32) + d).view(F)[0]
            if int(to_bf16(np.array([w * s], F))[0]) != bf16_once(np.float64(w) * np.float64(s)):
                return w
    raise AssertionError(f'no double-rounding product found for scale {s}')


# ================================================================================================ pack
@register
class Pack(Kernel):
    key = 'pack'
    nonfinite_ok = True                                     # (the largest finite f32 becomes a bf16 infinity; unwritten elements fail the bit compare)
    faults = ('neighbour_scale', 'truncate', 'fwd_scaled', 'bwd_unscaled', 'past_n')

    def planted(self, c):
        """(co, ci, tap) of the planted double-rounding products"""
        if not c['scale'] or c['Co'] < 4 or c['Ci'] * c['taps'] < 8:
            return []
        return [(co, c['Ci'] - 1, c['taps'] - 1) for co in (2, 3)]

    def make(self, c):
        r = rng_of(c)
        Co, Ci, t = c['Co'], c['Ci'], c['taps']
        # a magnitude per output row, a sign per column
        w = (0.5 + r.random((Co, Ci, t))).astype(F) * gain(np.arange(Co))[:, None, None] * sign(np.arange(Ci * t)).reshape(1, Ci, t)
        scale = ((0.75 + 0.5 * r.random(Co)) * gain(np.arange(Co) + 1) * sign(np.arange(Co) + 3)).astype(F)
        sp = finite_specials()
        if w.size >= 64:
            w.reshape(-1)[:len(sp)] = sp
            w.reshape(-1)[w.size - len(sp):] = sp[::-1]
        for co, ci, tap in self.planted(c):
            w[co, ci, tap] = double_rounding_w(scale[co])
        return dict(w=w, scale=scale)

    def frames(self, c, inp):
        fr = {}
        if c['wf']:
            fr['wf'] = Frame(c['dt'], c['Co'], c['taps'] * c['Ci'], pad=1 if c['mis'] == 'wf' else 0)
        if c['wb']:
            fr['wb'] = Frame(c['dt'], c['Ci'], c['taps'] * c['Co'], pad=1 if c['mis'] == 'wb' else 0)
        return fr

    def images(self, c, inp, fault=None):
        w, s, dt = inp['w'], inp['scale'], c['dt']
        Co, Ci, t = c['Co'], c['Ci'], c['taps']
        st = (lambda a: (bits(np.ascontiguousarray(a, F)) >> 16).astype(np.uint16)) if (fault == 'truncate' and dt == 'bf16') else (lambda a: store(dt, a))
        with np.errstate(over='ignore'):
            sc = np.roll(s, 1) if fault == 'neighbour_scale' else s
            wf_src = w * s[:, None, None] if (fault == 'fwd_scaled' and c['scale']) else w
            wb_src = w * sc[:, None, None] if (c['scale'] and fault != 'bwd_unscaled') else w          # one f32 multiply
        return dict(wf=st(wf_src.transpose(0, 2, 1)).reshape(Co, t * Ci), wb=st(wb_src.transpose(1, 2, 0)).reshape(Ci, t * Co))

    def restate(self, c, inp, fr, fault=None):
        img = self.images(c, inp, fault)
        for n, f in fr.items():
            f.region()[:] = img[n]

    def verify(self, c, inp, got):
        ref = self.images(c, inp)
        w64, s64 = inp['w'].astype(np.float64), inp['scale'].astype(np.float64)
        ref64 = dict(wf=w64.transpose(0, 2, 1), wb=(w64 * s64[:, None, None] if c['scale'] else w64).transpose(1, 2, 0))
        out = {}
        for n, g in got.items():
            exact(g, ref[n], f'{c["name"]}.{n}')
            r64 = ref64[n].reshape(g.shape)
            m = np.isfinite(val(c['dt'], ref[n]))            # (overflow to infinity is the restatement's to judge)
            out[f'pack {n}'] = bounded(np.where(m, val(c['dt'], g), 0), np.where(m, r64, 0), np.where(m, np.abs(r64), 0), 1, c['dt'], f'{c["name"]}.{n}')
        return out


# ================================================================================================ pack_frag
def frag_layout(b, fault=None):
    """[N][K] bf16 bits -> fragment-major (include/sedt_hip.h: SedtFragJob): block (n / 32, k / 16) of 1 KB, lane 32 ((k % 16) / 8) + n % 32
    owns 8 consecutive k"""
    N, K_ = b.shape
    v = b.reshape(N // 32, 32, K_ // 16, 2, 8).transpose(0, 2, 3, 1, 4)
    if fault == 'halves_swapped':
        v = v[:, :, ::-1]
    return np.ascontiguousarray(v).reshape(1, N * K_)


@register
class Frag(Kernel):
    key = 'frag'
    nonfinite_ok = True                                     # (a bf16 source is a packed operand with its specials)
    faults = ('halves_swapped', 'past_n')

    def make(self, c):
        if c['src'] == 'bf16':                               # the forward image of a pack row of the same shape
            pc = dict(Co=c['N'], Ci=c['K'], taps=1, dt='bf16', scale=1, wf=1, wb=1, mis='none', name=c['name'])
            pk = KERNELS['pack']
            return dict(w=pk.images(pc, pk.make(pc))['wf'])
        return dict(w=G.data(rng_of(c), c['N'], c['K']))

    def frames(self, c, inp):
        return {n: Frame('bf16', 1, c['N'] * c['K']) for n in ('wf', 'wb') if c[n]}

    def images(self, c, inp, fault=None):
        b = inp['w'] if c['src'] == 'bf16' else to_bf16(inp['w'])
        return dict(wf=frag_layout(b, fault), wb=frag_layout(np.ascontiguousarray(b.T), fault))

    def restate(self, c, inp, fr, fault=None):
        img = self.images(c, inp, fault)
        for n, f in fr.items():
            f.region()[:] = img[n]

    def verify(self, c, inp, got):
        ref = self.images(c, inp)
        w64 = val(c['src'], inp['w']).astype(np.float64)
        out = {}
        for n, g in got.items():
            exact(g, ref[n], f'{c["name"]}.{n}')
            # float64: the source's values through the same permutation (a permutation of float64 is exact; their bf16 rounding is not)
            src = w64 if n == 'wf' else np.ascontiguousarray(w64.T)
            N, K_ = src.shape
            r64 = np.ascontiguousarray(src.reshape(N // 32, 32, K_ // 16, 2, 8).transpose(0, 2, 3, 1, 4)).reshape(1, -1)
            m = np.isfinite(r64) & np.isfinite(from_bf16(ref[n]))
            out[f'frag {n}'] = bounded(np.where(m, from_bf16(g), 0), np.where(m, r64, 0), np.where(m, np.abs(r64), 0), 1, 'bf16', f'{c["name"]}.{n}')
        return out


# ================================================================================================ FrozenBN fold
@register
class BnFold(Kernel):
    key = 'bn_fold'
    faults = ('eps_dropped', 'past_n')
    RV = np.array([0.0, 1e-5, 1.0, 1e4], F)                  # eps dominant, comparable, negligible

    def make(self, c):
        r = rng_of(c)
        n = c['n']
        i = np.arange(n)
        rv = self.RV[i % 4] * (1.0 + 0.5 * (i // 4 % 3)).astype(F)
        return dict(w=((0.5 + r.random(n)) * sign(i)).astype(F), b=r.standard_normal(n).astype(F),
                    rm=((0.5 + r.random(n)) * gain(i) * sign(i + 1)).astype(F), rv=rv.astype(F))

    def frames(self, c, inp):
        return dict(scale=Frame('f32', 1 if c['n'] else 0, c['n']), bias=Frame('f32', 1 if c['n'] else 0, c['n']))

    def restate(self, c, inp, fr, fault=None):
        if not c['n']:
            return
        with np.errstate(divide='ignore'):
            sc = inp['w'] * (F(1) / np.sqrt(inp['rv'] + (F(0) if fault == 'eps_dropped' else EPS32)))
        sc = np.where(np.isfinite(sc), sc, F(3e38)).astype(F)
        fr['scale'].region()[0] = sc
        fr['bias'].region()[0] = inp['b'] - inp['rm'] * sc

    def verify(self, c, inp, got):
        if not c['n']:
            return {}
        w, b, rm, rv = (inp[n].astype(np.float64) for n in ('w', 'b', 'rm', 'rv'))
        sc = w / np.sqrt(rv + np.float64(EPS32))
        k = K_FN['rsqrt']
        return {'bn_fold scale': bounded(got['scale'][0], sc, k * np.abs(sc), 1, 'f32', c['name'] + '.scale'),
                'bn_fold bias': bounded(got['bias'][0], b - rm * sc, np.abs(b) + (2 + k) * np.abs(rm * sc), 1, 'f32', c['name'] + '.bias'),
                'k:rsqrt(bn_fold)': k_measure(got['scale'][0], sc, np.abs(sc), np.abs(sc))}


# ================================================================================================ stem
def stem_weights(r):
    """w0, b0 [3], w1 [64][3][49]: w0, b0 and every colour channel of w1 at gains of their own"""
    w0 = ((0.5 + r.random(3)) * 4.0 * np.array([1, -1, 1])).astype(F)
    b0 = ((0.5 + r.random(3)) / 16.0 * np.array([-1, -1, 1])).astype(F)
    w1 = ((0.5 + r.random((64, 3, 49))) * np.array([1.0, 8.0, 0.125])[None, :, None] * sign(np.arange(49))[None, None, :]
          * gain(np.arange(64))[:, None, None]).astype(F)
    return w0, b0, w1


@register
class StemPrep(Kernel):
    key = 'stem_prep'
    faults = ('b0_for_w0', 'channel_swapped', 'past_n')

    def make(self, c):
        w0, b0, w1 = stem_weights(rng_of(c))
        return dict(w0=w0, b0=b0, w1=w1)

    def frames(self, c, inp):
        return dict(wcat=Frame(c['dt'], 64, 128))

    def restate(self, c, inp, fr, fault=None):
        w1 = inp['w1'][:, ::-1] if fault == 'channel_swapped' else inp['w1']
        out = np.zeros((64, 128), F)
        for half, src in ((0, inp['b0'] if fault == 'b0_for_w0' else inp['w0']), (64, inp['b0'])):
            v = np.zeros((64, 49), F)
            for ch in range(3):
                v = v + w1[:, ch, :] * src[ch]
            out[:, half:half + 49] = v
        fr['wcat'].region()[:] = store(c['dt'], out)

    def verify(self, c, inp, got):
        w1 = inp['w1'].astype(np.float64)
        g = got['wcat']
        out = {}
        for half, src in ((0, inp['w0']), (64, inp['b0'])):
            p = w1 * src.astype(np.float64)[None, :, None]
            out['stem_prep'] = max(out.get('stem_prep', 0.0), bounded(val(c['dt'], g[:, half:half + 49]), p.sum(1), np.abs(p).sum(1), 3, c['dt'],
                                                                      f'{c["name"]}.cols{half}'))
            assert not bits(g[:, half + 49:half + 64]).any(), f'{c["name"]}: columns {half + 49}..{half + 63} are not +0'
        return out


@register
class StemConv0Grad(Kernel):
    key = 'stem_conv0_grad'
    faults = ('halves_swapped', 'past_n')

    def make(self, c):
        r = rng_of(c)
        _, _, w1 = stem_weights(r)
        Gm = np.full((64, 128), np.nan, F)                   # the kernel must not read columns 49..63 of either half
        Gm[:, :49] = G.data(r, 64, 49) * F(4.0)
        Gm[:, 64:113] = G.data(r, 64, 49) * F(1.0 / 16)
        return dict(G=Gm, w1=w1)

    def frames(self, c, inp):
        return dict(dw0=Frame('f32', 1, 3), db0=Frame('f32', 1, 3))

    def restate(self, c, inp, fr, fault=None):
        gx, gb = inp['G'][:, :49], inp['G'][:, 64:113]
        if fault == 'halves_swapped':
            gx, gb = gb, gx
        fr['dw0'].region()[0] = (inp['w1'] * gx[:, None, :]).astype(F).sum(axis=(0, 2), dtype=F)
        fr['db0'].region()[0] = (inp['w1'] * gb[:, None, :]).astype(F).sum(axis=(0, 2), dtype=F)

    def verify(self, c, inp, got):
        w1, Gm = inp['w1'].astype(np.float64), inp['G'].astype(np.float64)
        out = {}
        for n, g in (('dw0', Gm[:, :49]), ('db0', Gm[:, 64:113])):
            p = w1 * g[:, None, :]
            out[f'stem_conv0_grad {n}'] = bounded(got[n][0], p.sum(axis=(0, 2)), np.abs(p).sum(axis=(0, 2)), 64 * 49, 'f32', f'{c["name"]}.{n}')
        return out


# ================================================================================================ split-K reduce
def sum_mode0(s):
    s0, s1, s2, s3 = s[0].copy(), np.zeros_like(s[0]), np.zeros_like(s[0]), np.zeros_like(s[0])
    z = 1
    while z + 4 <= len(s):
        s0, s1, s2, s3 = s0 + s[z], s1 + s[z + 1], s2 + s[z + 2], s3 + s[z + 3]
        z += 4
    while z < len(s):
        s0 = s0 + s[z]
        z += 1
    return (s0 + s1) + (s2 + s3)


def sum_mode1(s):
    v, u = s[0].copy(), np.zeros_like(s[0])
    z = 1
    while z + 2 <= len(s):
        v, u = v + s[z], u + s[z + 1]
        z += 2
    if z < len(s):
        v = v + s[z]
    return v + u


def sum_mode2(s):
    a = np.zeros_like(s[0])
    for z in range(len(s)):
        a = a + s[z]
    return a


def sum_mode3(s):
    g = []
    for zg in range(4):
        s0, s1 = np.zeros_like(s[0]), np.zeros_like(s[0])
        z = zg
        while z + 4 < len(s):
            s0, s1 = s0 + s[z], s1 + s[z + 4]
            z += 8
        if z < len(s):
            s0 = s0 + s[z]
        g.append(s0 + s1)
    return (g[0] + g[1]) + (g[2] + g[3])


def sum_colsum(s):
    g = []
    for zg in range(4):
        b = [np.zeros_like(s[0]) for _ in range(4)]
        z = zg
        while z + 12 < len(s):
            for i in range(4):
                b[i] = b[i] + s[z + 4 * i]
            z += 16
        while z < len(s):
            b[0] = b[0] + s[z]
            z += 4
        g.append((b[0] + b[1]) + (b[2] + b[3]))
    return (g[0] + g[1]) + (g[2] + g[3])


SUM = {0: sum_mode0, 1: sum_mode1, 2: sum_mode2, 3: sum_mode3}


def _tail(s, fault, which):
    if fault == which + 'tail_dropped' and len(s) > 1:
        return s[:-1]
    if fault == which + 'tail_twice':
        return np.concatenate([s, s[-1:]])
    return s


@register
class Reduce(Kernel):
    key = 'reduce'
    faults = ('tail_dropped', 'tail_twice', 'cs_tail_dropped', 'cs_tail_twice', 'tap_channel_swapped', 'neighbour_rowscale', 'past_n')

    def make(self, c):
        import prep_cases as PC
        r = rng_of(c)
        sk, R, t, Ci = c['splitk'], c['R'], c['taps'], c['Ci']
        # every slice at a magnitude of its own, every row at a row scale of its own, a sign per column: no cancellation inside a sum
        slab = (0.5 + r.random((sk, R, t, Ci))).astype(F) * gain(np.arange(sk))[:, None, None, None] * sign(np.arange(t * Ci)).reshape(1, 1, t, Ci)
        inp = dict(slab=slab.astype(F), rowscale=(gain(np.arange(R) + 1) * (1.0 + 0.125 * (np.arange(R) % 5)) * sign(np.arange(R) + 1)).astype(F))
        n = PC.cs_slices(c)
        if n is not None:
            inp['cs'] = ((0.5 + r.random((n, R))).astype(F) * gain(np.arange(n))[:, None] * sign(np.arange(R))[None, :]).astype(F)
        return inp

    def frames(self, c, inp):
        fr = {}
        if c['R'] * c['taps'] * c['Ci']:
            fr['out'] = Frame('f32', c['R'], c['Ci'] * c['taps'], pad=1 if c['mis'] == 'out' else 0)
        if c['cs'] is not None:
            fr['bias'] = Frame('f32', 1, c['R'])
        return fr

    def images(self, c, inp, fault=None):
        import prep_cases as PC
        out = {}
        R, t, Ci = c['R'], c['taps'], c['Ci']
        if R * t * Ci:
            mode = PC.reduce_mode(c)
            s = SUM[mode](_tail(inp['slab'], fault, ''))                                  # [R][taps][Ci]
            rs = np.roll(inp['rowscale'], 1) if fault == 'neighbour_rowscale' else inp['rowscale']
            if c['scale']:
                s = s * rs[:, None, None]
            elif mode == 1:
                s = s * F(1)
            if not (fault == 'tap_channel_swapped' and mode == 1):
                s = s.transpose(0, 2, 1)                                                  # -> [R][Ci][taps]
            out['out'] = np.ascontiguousarray(s, F).reshape(R, Ci * t)
        if c['cs'] is not None:
            out['bias'] = sum_colsum(_tail(inp['cs'], fault, 'cs_'))[None, :]
        return out

    def restate(self, c, inp, fr, fault=None):
        img = self.images(c, inp, fault)
        for n, f in fr.items():
            f.region()[:] = img[n]

    def verify(self, c, inp, got):
        ref = self.images(c, inp)
        out = {}
        if 'out' in got:
            exact(got['out'], ref['out'], c['name'] + '.out')
            s64 = inp['slab'].astype(np.float64)
            rs = inp['rowscale'].astype(np.float64)[:, None, None] if c['scale'] else 1.0
            r64 = (s64.sum(0) * rs).transpose(0, 2, 1).reshape(got['out'].shape)
            t64 = (np.abs(s64).sum(0) * np.abs(rs)).transpose(0, 2, 1).reshape(got['out'].shape)
            out['reduce out'] = bounded(got['out'], r64, t64, c['splitk'], 'f32', c['name'] + '.out')
        if 'bias' in got:
            exact(got['bias'], ref['bias'], c['name'] + '.bias')
            c64 = inp['cs'].astype(np.float64)
            out['reduce colsum'] = bounded(got['bias'][0], c64.sum(0), np.abs(c64).sum(0), len(c64), 'f32', c['name'] + '.bias')
        return out


# kernel, fault: each must fail at least one row (tests/test_prep_check_cpu.py names the rows)
FAULTS = [(k.key, f) for k in KERNELS.values() for f in k.faults]
