"""References, bounds, guard frames and numpy restatements for the glue, pooling and skinny-head kernels (csrc/misc.hip,
csrc/split3.hip, csrc/skinny.hip).  A helper of tests/test_glue_envelope_gpu.py and tests/test_glue_check_cpu.py, not a conftest;
the rows are in tests/glue_cases.py.

One Kernel object per kernel key: make(row) -> the inputs (numpy, in their stored form: f32 as float32, bf16 as uint16 bit patterns,
bytes as uint8), frames(row, inputs) -> the outputs as Frames, restate(row, inputs, frames, fault) -> the kernel restated in
np.float32 writing into the frames' host images, verify(row, inputs, got) -> the checks on the owned elements, returning the largest
error / bound ratios.  The GPU module uploads the same inputs and frame images, launches the C entry point on pointers into the
frames, reads the images back and calls verify_row(): the device result and the restatement go through the same checks.

Inputs.  Every clip, row, source or job has its own magnitude (gain(): x1/16 and x4 alternating, times an offset factor) and every
column its own sign (sign()): a value taken from the neighbouring row, clip, column or source is off by a large factor.

Guard frame.  A Frame is one buffer filled with 0xFF bytes (a NaN in f32 and in bf16; 0xA5 for integer outputs) that holds the output
GUARD = 32 elements from either end; a strided output also has its gap columns inside.  After a launch no byte outside the owned
elements may differ from the fill (check_guard) and every owned float must be finite.

Exact kernels (exact()): compared on bits with the np.float32 restatement - a copy, a cast, a compare, one f32 operation and one
rounding, or a fixed-order f32 sum restated in the same order (np.cumsum over float32 adds in index order).  They are ALSO compared with
float64 under the bound below, so that a mistake in the restatement shows.

Bounded kernels (bounded() -> gemm_check.check): |got - ref| <= c (sqrt(K) 2^-24 sum|terms| + u_out |ref|), c = 2, u_out = 2^-8 for a
bf16 output and 0 for f32, K the number of summed terms (or of roundings on the way, where the kernel is a chain of them).

Transcendental terms.  The error of erff, expf, __expf, sinf / cosf, powf cannot be derived from the code: the bound gets
k_fn 2^-24 s on top, s the magnitude the function value enters the result with:
  * sinf / cosf (posenc): s = 1 + |argument|; powf (posenc, the argument's divisor): s = |argument|;
  * __expf in the skinny sigmoid: s = sigma'(z) (1 + |z|), sigma' the float64 derivative at the pre-activation z;
  * erff and expf in the GELU: |ref| cancels where 1 + erf -> 0 (x = -10: ref ~ 1e-22, erff's absolute error ~ 6e-8), so s is the term
    the function value sits in: 0.5 |x| |erf| (forward), |g| 0.5 |erf| and |g| |x| phi(x) (backward), times 1 / (1 - p).
K_FN holds k_fn per function: four times the largest |got - ref64| / (2^-24 s) measured on the device over the rows' inputs (f32 output
rows, the elements where s is at least a quarter of sum|terms|; all of the element's error booked on the function: k_measure()),
rounded up to a power of two - the inputs are seeded, the factor four is for a
compiler update.  Measured on MI355X (gfx950, ROCm 7 hipcc), largest quotient -> k_fn:
    erf   (erff)     6.1 in gelu_fwd, 8.8 in gelu_bwd (erf and exp booked together there)  -> 64
    exp   (expf)     8.8 in gelu_bwd                                                       -> 64
    nexp  (__expf)   4.5 in the skinny sigmoid                                             -> 32
    sin   (sinf / cosf) and pow (powf)   1.04 in posenc (booked together)                  -> 8 each
The quotients include the plain roundings of the same elements (the np.float32 restatements, which use numpy's functions, sit at 6.1,
8.8, 4.5 and 1.28), so the k_fn are upper estimates of the functions' own error.

Skinny forward above 64 KB of LDS ((N + 16)(K + 4) 4 bytes: 66,048 B at N = 16, K = 512; 131,584 B at K = 1024): the entry point now
raises the kernel's dynamic-LDS limit before the launch.  Nobody measured whether those launches would have failed without the
attribute: the rows were added after the fix and never run against the old code.
"""
import math
import zlib

import numpy as np
import torch

from attn_check import drop_keep, drop_threshold, inv_keep
from conv_check import q as q_bf16
from gemm_check import U_ACC, U_BF16, _ranges, check

F = np.float32
GUARD = 32
NP = dict(f32=np.float32, bf16=np.uint16, u8=np.uint8, u32=np.uint32)
FILL = dict(f32=0xFF, bf16=0xFF, u8=0xA5, u32=0xA5)
ACT = dict(none=0, relu=1, sigmoid=2)
K_FN = dict(erf=64.0, exp=64.0, nexp=32.0, sin=8.0, pow=8.0)
SEED = 0x5EED1234


# ------------------------------------------------------------------------------------------------ number formats
def to_bf16(a):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even: torch's CPU conversion"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def from_bf16(u):
    return (np.asarray(u, np.uint16).astype(np.uint32) << 16).view(np.float32)


def store(dt, a):
    """f32 values -> stored form of dt (one rounding for bf16)"""
    return to_bf16(a) if dt == 'bf16' else np.ascontiguousarray(a, dtype=np.float32)


def val(dt, s):
    """stored form -> f32 values"""
    return from_bf16(s) if dt == 'bf16' else np.asarray(s, np.float32)


def quant(dt, a):
    """f32 values rounded to dt, stored (conv_check.q for bf16: the rounding the other envelope modules use)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == 'bf16':
        return to_bf16(q_bf16(torch.from_numpy(a)).numpy().astype(np.float32))
    return a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def rng_of(c, salt=0):
    return np.random.default_rng(zlib.crc32(c['name'].encode()) + salt)


def gain(i):
    """magnitude of clip / row / source / job i: x1/16 and x4 alternating, times 1, 1.25, 1.5 (period 3)"""
    i = np.asarray(i)
    return (np.where(i % 2 == 1, 4.0, 1.0 / 16) * (1.0 + 0.25 * (i % 3))).astype(F)


def sign(j):
    """sign pattern of column / channel j"""
    j = np.asarray(j, np.int64)
    return np.where(((j * 2654435761) >> 5) & 1, -1.0, 1.0).astype(F)


def data(r, rows, cols, dt='f32', signed=True):
    """[rows, cols] values (stored in dt): row i at gain(i), column j at sign(j), magnitudes in [0.5, 1.5) of the gain"""
    a = (0.5 + r.random((rows, cols))).astype(F) * gain(np.arange(rows))[:, None]
    if signed:
        a = a * sign(np.arange(cols))[None, :]
    return quant(dt, a)


# ------------------------------------------------------------------------------------------------ guard frames
class Frame(object):
    """an output of `rows` x `cols` elements of dt, rows `ld` elements apart, inside one filled buffer: GUARD (+ pad) elements in
    front, GUARD behind.  buf is the host image; the device copy is made from it."""

    def __init__(self, dt, rows, cols, ld=None, pad=0):
        self.dt, self.rows, self.cols, self.ld, self.off = dt, rows, cols, ld or cols, GUARD + pad
        self.span = (rows - 1) * self.ld + cols if rows > 0 and cols > 0 else 0
        self.buf = np.full((self.off + self.span + GUARD) * NP[dt]().itemsize, FILL[dt], np.uint8).view(NP[dt])
        self.own = np.zeros(self.buf.shape, bool)
        if self.span:
            self.region(self.own)[:] = True

    def region(self, img=None):
        """the owned [rows, cols] elements as a strided view of an image"""
        img = self.buf if img is None else img
        return np.lib.stride_tricks.as_strided(img[self.off:], (self.rows, self.cols), (self.ld * img.itemsize, img.itemsize))

    def owned(self, img):
        return self.region(img).copy() if self.span else np.zeros((self.rows, self.cols), NP[self.dt])

    def check_guard(self, img, what):
        fill = np.full(1, FILL[self.dt], np.uint8).repeat(img.itemsize).view(img.dtype)[0]
        bad = (bits(img) != bits(np.asarray([fill]))[0]) & ~self.own
        if bad.any():
            idx = np.nonzero(bad)[0] - self.off
            raise AssertionError(f'{what}: {int(bad.sum())} elements outside the output changed, at offsets {_ranges(idx.tolist())} '
                                 f'from its first element (output spans {self.span})')

    def check_finite(self, img, what):
        if self.dt in ('f32', 'bf16') and self.span:
            v = val(self.dt, self.owned(img))
            bad = ~np.isfinite(v)
            if bad.any():
                rr, cc = np.nonzero(bad)
                raise AssertionError(f'{what}: {int(bad.sum())} non-finite (unwritten?) elements, rows {_ranges(rr.tolist())}, '
                                     f'cols {_ranges(cc.tolist())}')


def exact(got, ref, what):
    """bit equality of two stored arrays, with the failing rows / columns as ranges"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape and got.dtype.itemsize == ref.dtype.itemsize, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = bits(got) != bits(ref)
    if bad.any():
        rr, cc = np.nonzero(bad)
        i, j = rr[0], cc[0]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ in bits (first at row {i} col {j}: got '
                             f'{bits(got)[i, j]:#x} want {bits(ref)[i, j]:#x}); rows {_ranges(rr.tolist())}; cols {_ranges(cc.tolist())}')
    return 0.0


def bounded(got, ref, terms, K, dt_out, what, extra=None):
    """gemm_check.check on numpy arrays: got (f32 values), ref and terms float64; extra = sum of k_fn * s, which enters as
    extra * 2^-24 (not multiplied by c sqrt(K))"""
    got, ref, terms = (np.atleast_2d(np.asarray(a, np.float64)) for a in (got, ref, terms))
    if got.size == 0:
        return 0.0
    if extra is not None:
        terms = terms + np.atleast_2d(extra) / (2.0 * math.sqrt(K))
    return check(torch.from_numpy(got), torch.from_numpy(ref), torch.from_numpy(np.broadcast_to(terms, ref.shape).copy()), K,
                 U_BF16 if dt_out == 'bf16' else 0.0, what=what)


def k_measure(got, ref, s, terms):
    """largest |got - ref| / (2^-24 s) over the elements where the function's term is at least a quarter of sum|terms|: what a device
    run books on a transcendental function (f32 outputs; all of the element's error goes to the function, so the figure includes the
    plain roundings and is an over-estimate).  Elsewhere - a saturated sigmoid, erf(x) near 0 - s tends to 0 while the plain
    roundings stay, and the quotient says nothing about the function.  0 when no element qualifies."""
    got, ref, s, terms = (np.asarray(a, np.float64) for a in (got, ref, s, terms))
    m = (s > 0) & (s >= 0.25 * terms)
    return float((np.abs(got - ref)[m] / (U_ACC * s[m])).max()) if m.any() else 0.0


class Kernel(object):
    nonfinite_ok = False
    faults = ()

    def frames(self, c, inp):
        raise NotImplementedError


KERNELS = {}


def register(cls, table=None):
    """table: another module's registry (tests/prep_check.py keeps its own, so that each CPU module's table-coverage test sees its own keys)"""
    (KERNELS if table is None else table)[cls.key] = cls()
    return cls


def verify_row(key, c, inp, fr, imgs, table=None):
    """guards, finiteness and the kernel's own checks on the images (name -> array of the frame's dtype) after a launch or a restatement"""
    k = (KERNELS if table is None else table)[key]
    got = {}
    for n, f in fr.items():
        f.check_guard(imgs[n], f'{c["name"]}.{n}')
        if not k.nonfinite_ok:
            f.check_finite(imgs[n], f'{c["name"]}.{n}')
        got[n] = f.owned(imgs[n])
    return k.verify(c, inp, got)


def ratio_key(name, c):
    """the row of the ratio tables a result goes to: kernel output and the row's dtype (a bf16 output's ratio is its own rounding's)"""
    return name if name.startswith('k:') else f'{name} [{c.get("dt", "f32")}]'


def restated(key, c, fault=None, table=None):
    """the row through the numpy restatement (with an injected fault, if any) and the same verification as a device result"""
    k = (KERNELS if table is None else table)[key]
    inp = k.make(c)
    fr = k.frames(c, inp)
    k.restate(c, inp, fr, fault)
    _generic_fault(fr, fault)
    return verify_row(key, c, inp, fr, {n: f.buf for n, f in fr.items()}, table)


def _generic_fault(fr, fault):
    f = next(iter(fr.values()))
    if fault == 'last_vector' and f.span:                   # the last vector (up to four elements) of the output stays unwritten
        flat = f.region()
        n = min(4, f.cols)
        flat[-1, f.cols - n:] = np.full(1, FILL[f.dt], np.uint8).repeat(f.buf.itemsize).view(f.buf.dtype)[0]
    if fault == 'past_n':                                   # one element past the end written
        f.buf[f.off + f.span] = 0


# ================================================================================================ elementwise
@register
class Add(Kernel):
    key = 'add'
    faults = ('last_vector', 'past_n', 'b_mod_ignored')

    def make(self, c):
        r = rng_of(c)
        rb = c['b_mod'] if c['b_mod'] > 0 else c['rows']
        return dict(a=data(r, c['rows'], c['cols'], c['dt']), b=data(r, rb, c['cols'], c['dt'])[::-1].copy())

    def frames(self, c, inp):
        return dict(out=Frame(c['dt'], c['rows'], c['cols']))

    def _rb(self, c, fault=None):
        r = np.arange(c['rows'])
        if c['b_mod'] > 0 and fault != 'b_mod_ignored':
            return r % c['b_mod']
        return np.minimum(r, (c['b_mod'] if c['b_mod'] > 0 else c['rows']) - 1) if c['rows'] else r

    def restate(self, c, inp, fr, fault=None):
        if c['rows']:
            fr['out'].region()[:] = store(c['dt'], val(c['dt'], inp['a']) + val(c['dt'], inp['b'])[self._rb(c, fault)])

    def verify(self, c, inp, got):
        if not c['rows']:
            return {}
        a, b = val(c['dt'], inp['a']), val(c['dt'], inp['b'])[self._rb(c)]
        exact(got['out'], store(c['dt'], a + b), c['name'])
        return {'add': bounded(val(c['dt'], got['out']), a.astype(np.float64) + b, np.abs(a).astype(np.float64) + np.abs(b), 1, c['dt'], c['name'])}


def cast_specials():
    """f32 bit patterns: both kinds of f32 -> bf16 tie (low half 0x8000 under an even and an odd upper half), +-0, a subnormal, +-inf,
    the largest finite f32 (rounds to inf in bf16), a NaN"""
    return np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x00012345, 0x7F800000, 0xFF800000, 0x7F7FFFFF,
                     0x7FC00000, 0x3F807FFF, 0x3F808001], np.uint32).view(np.float32)


@register
class Cast(Kernel):
    key = 'cast'
    nonfinite_ok = True
    faults = ('last_vector', 'past_n')

    def make(self, c):
        r = rng_of(c)
        n = c['n']
        x = (r.standard_normal(n) * gain(np.arange(n))).astype(F)
        sp = cast_specials()
        if n >= 255:
            x[:len(sp)] = sp
            x[n - len(sp):] = sp[::-1]
        elif n:
            x[0] = sp[1]
        return dict(x=store(c['src'], x) if c['src'] == 'bf16' else x)

    def frames(self, c, inp):
        return dict(out=Frame(c['dst'], 1 if c['n'] else 0, c['n']))

    def ref(self, c, inp):
        """torch's CPU conversion"""
        tdt = dict(f32=torch.float32, bf16=torch.bfloat16)
        x = torch.from_numpy(inp['x'].view(np.int16) if c['src'] == 'bf16' else inp['x'])
        x = x.view(torch.bfloat16) if c['src'] == 'bf16' else x
        y = x.to(tdt[c['dst']])
        return y.view(torch.int16).numpy().view(np.uint16) if c['dst'] == 'bf16' else y.numpy()

    def restate(self, c, inp, fr, fault=None):
        if c['n']:
            fr['out'].region()[0] = store(c['dst'], val(c['src'], inp['x']))

    def verify(self, c, inp, got):
        if not c['n']:
            return {}
        ref, g = self.ref(c, inp)[None, :], got['out']
        nan = np.isnan(val(c['dst'], ref))
        assert np.isnan(val(c['dst'], g))[nan].all(), f'{c["name"]}: a NaN did not stay a NaN'
        exact(np.where(nan, 0, bits(g)).astype(bits(g).dtype), np.where(nan, 0, bits(ref)).astype(bits(g).dtype), c['name'])
        return {}


@register
class ReluMask(Kernel):
    key = 'relu_mask'
    faults = ('last_vector', 'past_n')

    def make(self, c):
        r = rng_of(c)
        n, dt = c['n'], c['dt']
        g = data(r, 1, n, dt)[0] if n else store(dt, np.zeros(0, F))
        y = store(dt, (r.standard_normal(n) * gain(np.arange(n))).astype(F))
        sub = np.uint16(1) if dt == 'bf16' else np.array([1], np.uint32).view(F)[0]      # the smallest positive subnormal
        sp = [store(dt, np.array([-0.0], F))[0], store(dt, np.array([0.0], F))[0], sub, store(dt, np.array([-3.0], F))[0]]
        for i in range(min(n, 4)):
            y[(i * 97) % n if n >= 255 else i] = sp[i]
        if n >= 255:
            y[n - 1] = sub
        return dict(g=g, y=y)

    def frames(self, c, inp):
        return dict(out=Frame(c['dt'], 1 if c['n'] else 0, c['n']))

    def ref(self, c, inp):
        return np.where(val(c['dt'], inp['y']) > 0, inp['g'], np.zeros_like(inp['g']))[None, :]

    def restate(self, c, inp, fr, fault=None):
        if c['n']:
            fr['out'].region()[:] = self.ref(c, inp)

    def verify(self, c, inp, got):
        if c['n']:
            exact(got['out'], self.ref(c, inp), c['name'])
        return {}


@register
class SigmoidGrad(Kernel):
    key = 'sigmoid_grad'
    faults = ('last_vector', 'past_n')

    def make(self, c):
        r = rng_of(c)
        n = c['n']
        g = data(r, 1, n)[0] if n else np.zeros(0, F)
        s = r.random(n).astype(F)
        for i, v in enumerate((0.0, 0.5, 1.0)[:n]):
            s[(i * 101) % n if n >= 255 else i] = v
        return dict(g=g, s=s)

    def frames(self, c, inp):
        return dict(out=Frame('f32', 1 if c['n'] else 0, c['n']))

    def restate(self, c, inp, fr, fault=None):
        if c['n']:
            fr['out'].region()[0] = inp['g'] * inp['s'] * (F(1) - inp['s'])

    def verify(self, c, inp, got):
        if not c['n']:
            return {}
        g, s = inp['g'].astype(np.float64), inp['s'].astype(np.float64)
        ref = g * s * (1 - s)
        # three roundings: g s, 1 - s, their product (K = 9: sqrt(K) = 3)
        return {'sigmoid_grad': bounded(got['out'][0], ref, np.abs(ref), 9, 'f32', c['name'])}


@register
class AddN(Kernel):
    key = 'add_n'
    faults = ('source_dropped',)

    def make(self, c):
        return dict(src=self._src(c, rng_of(c)))

    def _src(self, c, r):
        # source j at gain(j): a dropped or doubled source moves every element by a large factor
        k, n, dt = c['k'], c['n'], c['dt']
        a = (0.5 + r.random((k, n))).astype(F) * gain(np.arange(k))[:, None] * sign(np.arange(n))[None, :]
        return quant(dt, a)

    def frames(self, c, inp):
        return dict(out=Frame(c['dt'], 1 if c['n'] else 0, c['n']))

    def sum32(self, c, inp, fault=None):
        v = val(c['dt'], inp['src'])
        k = c['k'] - (1 if fault == 'source_dropped' and c['k'] > 1 else 0)
        if fault == 'source_dropped' and c['k'] == 1:
            return store(c['dt'], np.zeros(c['n'], F))
        acc = np.cumsum(v[:min(k, 8)], axis=0, dtype=F)[-1]
        if k > 8:                                           # ops.add_n: the first eight rounded to the compute dtype, then the rest
            acc = np.cumsum(np.concatenate([val(c['dt'], store(c['dt'], acc))[None], v[8:k]]), axis=0, dtype=F)[-1]
        return store(c['dt'], acc)

    def restate(self, c, inp, fr, fault=None):
        if c['n']:
            fr['out'].region()[0] = self.sum32(c, inp, fault)

    def verify(self, c, inp, got):
        if not c['n']:
            return {}
        exact(got['out'][0], self.sum32(c, inp), c['name'])
        v = val(c['dt'], inp['src']).astype(np.float64)
        extra = None
        if c['k'] > 8:                                      # the intermediate rounding to the compute dtype
            extra = (U_BF16 if c['dt'] == 'bf16' else 0.0) / U_ACC * np.abs(v[:8].sum(0))
        return {'add_n': bounded(val(c['dt'], got['out'][0]), v.sum(0), np.abs(v).sum(0), c['k'], c['dt'], c['name'], extra)}


def seed_parts(mode):
    """(seed passed by value, word behind seed_ptr or None); the kernel adds them"""
    return dict(val=(SEED, None), ptr=(0, SEED ^ 0x1111), both=(SEED, 0x00C0FFEE))[mode]


def eff_seed(mode):
    v, p = seed_parts(mode)
    return (v + (p or 0)) & 0xffffffff


@register
class DropoutGrad(Kernel):
    key = 'dropout_grad'
    faults = ('index_from_ld',)
    LDI, LDO = 8, 16

    def make(self, c):
        r = rng_of(c)
        wide = data(r, c['rows'], c['cols'] + self.LDI, c['dt'])
        return dict(x=wide)                                # the input is the column view [:, :cols] of this

    def frames(self, c, inp):
        return dict(out=Frame(c['dt'], c['rows'], c['cols'], c['cols'] + self.LDO))

    def keep(self, c, fault=None):
        rows, cols = c['rows'], c['cols']
        rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
        idx = rr * (cols + self.LDI if fault == 'index_from_ld' else cols) + cc
        return drop_keep(eff_seed(c['seed']), idx.astype(np.uint64), drop_threshold(c['p']))

    def ref(self, c, inp, fault=None):
        x = val(c['dt'], inp['x'])[:, :c['cols']]
        return store(c['dt'], np.where(self.keep(c, fault), x * F(inv_keep(c['p'])), F(0)))

    def restate(self, c, inp, fr, fault=None):
        if c['rows']:
            fr['out'].region()[:] = self.ref(c, inp, fault)

    def verify(self, c, inp, got):
        if not c['rows']:
            return {}
        g = got['out']
        keep = self.keep(c)
        assert np.array_equal(bits(g) != 0, keep), f'{c["name"]}: keep pattern differs at {int((( bits(g) != 0) != keep).sum())} elements'
        exact(g, self.ref(c, inp), c['name'])
        if c['p'] == 0.0:
            exact(g, inp['x'][:, :c['cols']], c['name'] + ' (p = 0 returns the input bits)')
        return {}


def _erf(x):
    return torch.erf(torch.from_numpy(np.asarray(x, np.float64))).numpy()


@register
class Gelu(Kernel):
    key = 'gelu'
    faults = ('last_vector', 'past_n')

    def make(self, c):
        r = rng_of(c)
        n, dt = c['n'], c['dt']
        h = np.linspace(-10, 10, n).astype(F) if n else np.zeros(0, F)
        if n >= 8:
            h[1:5] = (0.0, -0.0, 1e-4, -1e-4)
        g = data(r, 1, n, dt)[0] if n else store(dt, np.zeros(0, F))
        return dict(h=quant(dt, h), g=g)

    def frames(self, c, inp):
        n = c['n']
        return dict(a=Frame(c['dt'], 1 if n else 0, n), gh=Frame(c['dt'], 1 if n else 0, n))

    def keep(self, c):
        if c['p'] == 0.0:
            return np.ones(c['n'], bool)
        return drop_keep(SEED, np.arange(c['n'], dtype=np.uint64), drop_threshold(c['p']))

    def ref64(self, c, inp):
        x, g = val(c['dt'], inp['h']).astype(np.float64), val(c['dt'], inp['g']).astype(np.float64)
        ik = float(inv_keep(c['p']))
        erf, phi = _erf(x / math.sqrt(2.0)), np.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        keep = self.keep(c)
        fwd = dict(ref=np.where(keep, 0.5 * x * (1 + erf) * ik, 0.0), terms=0.5 * np.abs(x) * (1 + np.abs(erf)) * ik,
                   s_erf=0.5 * np.abs(x) * np.abs(erf) * ik)
        bwd = dict(ref=np.where(keep, g * (0.5 * (1 + erf) + x * phi) * ik, 0.0), terms=np.abs(g) * (0.5 * (1 + np.abs(erf)) + np.abs(x) * phi) * ik,
                   s_erf=np.abs(g) * 0.5 * np.abs(erf) * ik, s_exp=np.abs(g) * np.abs(x) * phi * ik)
        return fwd, bwd, keep

    def restate(self, c, inp, fr, fault=None):
        if not c['n']:
            return
        x, g, ik = val(c['dt'], inp['h']), val(c['dt'], inp['g']), F(inv_keep(c['p']))
        erf = _erf(x.astype(np.float64) * float(F(0.70710678118654752))).astype(F)
        keep = self.keep(c)
        y = F(0.5) * x * (F(1) + erf)
        d = F(0.5) * (F(1) + erf) + x * F(0.39894228040143268) * np.exp(F(-0.5) * x * x).astype(F)
        fr['a'].region()[0] = store(c['dt'], np.where(keep, y * ik, F(0)))
        fr['gh'].region()[0] = store(c['dt'], np.where(keep, g * d * ik, F(0)))

    def verify(self, c, inp, got):
        if not c['n']:
            return {}
        fwd, bwd, keep = self.ref64(c, inp)
        out = {}
        for name, R, key in (('a', fwd, 'gelu_fwd'), ('gh', bwd, 'gelu_bwd')):
            gv = val(c['dt'], got[name][0])
            # the zero pattern is exact: a dropped element is +0 in bits; a kept one is non-zero wherever its reference is not tiny
            dropped = ~keep
            assert (bits(got[name][0])[dropped] == 0).all(), f'{c["name"]}.{name}: a dropped element is not +0'
            big = keep & (np.abs(R['ref']) > 1e-6 * R['terms']) & (R['terms'] > 0)     # (1 + erff(x) is 0 in f32 below x ~ -5.4)
            assert (gv[big] != 0).all(), f'{c["name"]}.{name}: a kept element is zero'
            extra = K_FN['erf'] * R['s_erf'] + (K_FN['exp'] * R['s_exp'] if 's_exp' in R else 0.0)
            out[key] = bounded(gv, R['ref'], R['terms'], 4, c['dt'], f'{c["name"]}.{name}', extra)
            if c['dt'] == 'f32':
                out['k:erf+exp(' + key + ')'] = k_measure(gv, R['ref'], R['s_erf'] + R.get('s_exp', 0.0), R['terms'])
        return out


# ================================================================================================ copies
@register
class Copy2d(Kernel):
    key = 'copy2d'
    SGAP, DGAP = 16, 32                                     # bytes between items on the source / destination side

    def make(self, c):
        r = rng_of(c)
        srcs = []
        for j, (outer, inner) in enumerate(c['jobs']):
            w = (inner + self.SGAP) // 4
            srcs.append((r.integers(0, 1 << 32, outer * w, dtype=np.uint64).astype(np.uint32) & np.uint32(0x00FFFFFF)) | np.uint32((j + 1) << 24))
        return {f'src{j}': s for j, s in enumerate(srcs)}

    def frames(self, c, inp):
        return {f'dst{j}': Frame('u32', outer, inner // 4, (inner + self.DGAP) // 4) for j, (outer, inner) in enumerate(c['jobs'])}

    def ref(self, c, inp, j):
        outer, inner = c['jobs'][j]
        return inp[f'src{j}'].reshape(outer, (inner + self.SGAP) // 4)[:, :inner // 4]

    def restate(self, c, inp, fr, fault=None):
        for j in range(len(c['jobs'])):
            fr[f'dst{j}'].region()[:] = self.ref(c, inp, j)

    def verify(self, c, inp, got):
        for j in range(len(c['jobs'])):
            exact(got[f'dst{j}'], self.ref(c, inp, j), f'{c["name"]} job {j}')
        return {}


def split_values(r, rows, cols):
    """|x| <= 1e30 over ten decades and more, +-0 and subnormals, each row at its own magnitude"""
    x = (r.standard_normal((rows, cols)) * 10.0 ** r.uniform(-10, 10, (rows, cols))).astype(F) * gain(np.arange(rows))[:, None]
    flat = x.reshape(-1)
    sp = np.array([0.0, -0.0, 1e-40, -1e-40, 1e30, -1e30, 1.0, 1.00390625], F)
    flat[:min(len(sp), flat.size)] = sp[:flat.size]
    flat[flat.size - 1] = F(-1e-42) if flat.size > 8 else flat[flat.size - 1]
    return x


def split_hi_lo(x):
    """hi = RNE bf16(x), lo = RNE bf16(x - hi); the subtraction is exact in f32 (tests/test_glue_check_cpu.py checks 1e5 samples)"""
    hi = to_bf16(x)
    lo = to_bf16(x - from_bf16(hi))
    return hi, lo


@register
class Split3(Kernel):
    key = 'split3'
    faults = ('hi_lo_hi',)

    def make(self, c):
        r = rng_of(c)
        return {f'src{j}': split_values(r, rows, cols + pad) for j, (rows, cols, pad, pat) in enumerate(c['jobs'])}

    def frames(self, c, inp):
        return {f'dst{j}': Frame('bf16', rows, (3 if pat else 2) * cols) for j, (rows, cols, pad, pat) in enumerate(c['jobs'])}

    def ref(self, c, inp, j, fault=None):
        rows, cols, pad, pat = c['jobs'][j]
        hi, lo = split_hi_lo(inp[f'src{j}'][:, :cols])
        if pat:
            return np.concatenate([hi, lo, hi] if fault == 'hi_lo_hi' else [hi, hi, lo], axis=1)
        return np.concatenate([hi, lo], axis=1)

    def restate(self, c, inp, fr, fault=None):
        for j in range(len(c['jobs'])):
            fr[f'dst{j}'].region()[:] = self.ref(c, inp, j, fault)

    def verify(self, c, inp, got):
        r = 0.0
        for j, (rows, cols, pad, pat) in enumerate(c['jobs']):
            exact(got[f'dst{j}'], self.ref(c, inp, j), f'{c["name"]} job {j}')
            g = from_bf16(got[f'dst{j}']).astype(np.float64)
            x = inp[f'src{j}'][:, :cols].astype(np.float64)
            # hi + lo carries 16 mantissa bits of x: |x - hi - lo| <= 2^-17 |x| + the smallest bf16 subnormal's half
            err = np.abs(x - g[:, :cols] - g[:, -cols:])
            bound = 2.0 ** -16 * np.abs(x) + 2.0 ** -134
            assert (err <= bound).all(), f'{c["name"]} job {j}: hi + lo is not x to 2^-16'
            r = max(r, float((err / bound).max()))
        return {'split3 hi+lo': r}


# ================================================================================================ SP-SEDT decoder input
@register
class DecIn(Kernel):
    key = 'dec_in'
    faults = ('keep_index_bQ',)

    def make(self, c):
        r = rng_of(c)
        B, Q, P, D = c['B'], c['Q'], c['P'], c['D']
        # patch rows at their own magnitude; query rows at another scale, so that a wrong patch (q / qpp) or clip shows
        patch = data(r, B * P, D, c['dt'])
        query = data(r, Q, D)[::-1].copy() * F(3.0)
        keep = (r.random((Q, B)) < 0.6).astype(F)
        return dict(patch=patch, query=query, keep=keep)

    def frames(self, c, inp):
        fr = dict(out=Frame(c['dt'], c['B'] * c['Q'], c['D']))
        if c['mode'] != 'eval':
            fr['keep_out'] = Frame('f32', c['Q'], c['B'])
        return fr

    def keep(self, c, inp, fault=None):
        B, Q = c['B'], c['Q']
        if c['mode'] == 'eval':
            return np.ones((Q, B), F)
        if c['mode'] == 'given':
            return inp['keep']
        if not c['ratio'] > 0:
            return np.ones((Q, B), F)
        th = drop_threshold(c['ratio'] if c['ratio'] < 1.0 else 0.99999)
        qq, bb = np.meshgrid(np.arange(Q), np.arange(B), indexing='ij')
        idx = bb * Q + qq if fault == 'keep_index_bQ' else qq * B + bb
        return drop_keep(SEED, idx.astype(np.uint64), th).astype(F)

    def ref(self, c, inp, keep):
        B, Q, P, qpp, D = c['B'], c['Q'], c['P'], c['qpp'], c['D']
        pv = val(c['dt'], inp['patch']).reshape(B, P, D)[:, np.arange(Q) // qpp]           # [B, Q, D]
        qs = F(1.0) if c['mode'] == 'eval' else F(2.0)
        return store(c['dt'], (qs * inp['query'][None] + keep.T[:, :, None] * pv).reshape(B * Q, D))

    def restate(self, c, inp, fr, fault=None):
        k = self.keep(c, inp, fault)
        fr['out'].region()[:] = self.ref(c, inp, k)
        if 'keep_out' in fr:
            fr['keep_out'].region()[:] = k

    def verify(self, c, inp, got):
        k = self.keep(c, inp)
        if 'keep_out' in got:
            exact(got['keep_out'], k, c['name'] + '.keep_out')
            k = got['keep_out']                             # ... and it is what the output used
        exact(got['out'], self.ref(c, inp, k), c['name'])
        B, Q, P, qpp, D = c['B'], c['Q'], c['P'], c['qpp'], c['D']
        pv = val(c['dt'], inp['patch']).astype(np.float64).reshape(B, P, D)[:, np.arange(Q) // qpp]
        qs = 1.0 if c['mode'] == 'eval' else 2.0
        qv = inp['query'].astype(np.float64)[None]
        kk = k.T[:, :, None].astype(np.float64)
        return {'dec_in': bounded(val(c['dt'], got['out']), (qs * qv + kk * pv).reshape(B * Q, D), (qs * np.abs(qv) + kk * np.abs(pv)).reshape(B * Q, D),
                                  1, c['dt'], c['name'])}


@register
class DecInBwd(Kernel):
    key = 'dec_in_bwd'
    faults = ('clip_tail_dropped',)

    def make(self, c):
        r = rng_of(c)
        B, Q, D = c['B'], c['Q'], c['D']
        # clip b at gain(b): rows are b * Q + q
        g = (0.5 + r.random((B, Q, D))).astype(F) * gain(np.arange(B))[:, None, None] * sign(np.arange(D))[None, None, :]
        g = g * (1 + np.arange(Q, dtype=F))[None, :, None]
        return dict(g=quant(c['dt'], g.reshape(B * Q, D)), keep=(r.random((Q, B)) < 0.6).astype(F))

    def frames(self, c, inp):
        fr = dict(d_query=Frame('f32', c['Q'], c['D']))
        if c['need_patch']:
            fr['d_patch'] = Frame(c['dt'], c['B'] * c['P'], c['D'])
        return fr

    def sums(self, c, inp, fault=None):
        B, Q, P, qpp, D = c['B'], c['Q'], c['P'], c['qpp'], c['D']
        g = val(c['dt'], inp['g']).reshape(B, Q, D)
        dp = np.zeros((B, P, D), F)
        for p in range(P):
            for r in range(qpp):
                qq = p * qpp + r
                if qq < Q:
                    dp[:, p] = dp[:, p] + inp['keep'][qq][:, None] * g[:, qq]
        per = (B + 3) // 4
        parts = []
        for grp in range(4):                                # four thread groups own consecutive quarters of the clips, in clip order
            b0, b1 = grp * per, min(B, grp * per + per)
            if fault == 'clip_tail_dropped' and b1 > b0:
                b1 = b0 + (b1 - b0) // 8 * 8                # the tail behind the eight-wide unroll
            parts.append(np.cumsum(g[b0:b1], axis=0, dtype=F)[-1] if b1 > b0 else np.zeros((Q, D), F))
        dq = F(2.0) * (((parts[0] + parts[1]) + parts[2]) + parts[3])
        return store(c['dt'], dp.reshape(B * P, D)), dq

    def restate(self, c, inp, fr, fault=None):
        dp, dq = self.sums(c, inp, fault)
        fr['d_query'].region()[:] = dq
        if 'd_patch' in fr:
            fr['d_patch'].region()[:] = dp

    def verify(self, c, inp, got):
        B, Q, P, qpp, D = c['B'], c['Q'], c['P'], c['qpp'], c['D']
        dp, dq = self.sums(c, inp)
        exact(got['d_query'], dq, c['name'] + '.d_query')
        g = val(c['dt'], inp['g']).astype(np.float64).reshape(B, Q, D)
        out = {'dec_in_bwd d_query': bounded(got['d_query'], 2 * g.sum(0), 2 * np.abs(g).sum(0), B, 'f32', c['name'] + '.d_query')}
        if 'd_patch' in got:
            exact(got['d_patch'], dp, c['name'] + '.d_patch')
            kg = inp['keep'].T[:, :, None].astype(np.float64) * g                        # [B, Q, D]
            pad = np.zeros((B, P * qpp - Q, D))
            ref = np.concatenate([kg, pad], 1).reshape(B, P, qpp, D).sum(2).reshape(B * P, D)
            ab = np.concatenate([np.abs(kg), pad], 1).reshape(B, P, qpp, D).sum(2).reshape(B * P, D)
            out['dec_in_bwd d_patch'] = bounded(val(c['dt'], got['d_patch']), ref, ab, qpp, c['dt'], c['name'] + '.d_patch')
        return out


# ================================================================================================ reductions and pooling
def colsum32(x, rows, cols, fault=None):
    """csrc/misc.hip colsum_kernel in np.float32: chunks of rows, four row groups per chunk (rows r0 + ty, step 4, in order), the four
    partials added left to right; a second pass of the same kernel over the chunk sums"""
    def one(x, rows, rpc, nch):
        out = np.zeros((nch, cols), F)
        for ch in range(nch):
            r0, r1 = ch * rpc, min(rows, ch * rpc + rpc)
            red = [np.cumsum(x[r0 + ty:r1:4], axis=0, dtype=F)[-1] if r0 + ty < r1 else np.zeros(cols, F) for ty in range(4)]
            out[ch] = ((red[0] + red[1]) + red[2]) + red[3]
        return out
    nch = min(max((rows + 255) // 256, 1), 256)
    rpc = (rows + nch - 1) // nch
    st1 = one(x, rows, rpc, nch)
    if nch == 1:
        return st1[0]
    if fault == 'last_chunk_dropped':
        st1, nch = st1[:-1], nch - 1
    return one(st1, nch, nch, 1)[0]


@register
class Colsum(Kernel):
    key = 'colsum'
    faults = ('last_chunk_dropped',)

    def in_dt(self, c):
        return 'f32' if c['in_f32'] else c['dt']

    def make(self, c):
        r = rng_of(c)
        return dict(x=data(r, c['rows'], c['cols'] + c['view'], self.in_dt(c)))

    def frames(self, c, inp):
        return dict(out=Frame('f32', 1, c['cols']))

    def restate(self, c, inp, fr, fault=None):
        x = val(self.in_dt(c), inp['x'])[:, :c['cols']]
        fr['out'].region()[0] = colsum32(x, c['rows'], c['cols'], fault)

    def verify(self, c, inp, got):
        x = val(self.in_dt(c), inp['x'])[:, :c['cols']]
        exact(got['out'][0], colsum32(x, c['rows'], c['cols']), c['name'])
        x = x.astype(np.float64)
        return {'colsum': bounded(got['out'][0], x.sum(0), np.abs(x).sum(0), c['rows'], 'f32', c['name'])}


@register
class Avgpool(Kernel):
    key = 'avgpool'
    faults = ('p_tail_dropped',)

    def make(self, c):
        r = rng_of(c)
        B, P, C = c['B'], c['P'], c['C']
        # position q of clip b at gain(b * P + q): a dropped or repeated position moves the mean
        return dict(x=data(r, B * P, C, c['dt']))

    def frames(self, c, inp):
        return dict(out=Frame('f32', 1 if c['B'] else 0, c['B'] * c['C']))

    def mean32(self, c, inp, fault=None):
        B, P, C = c['B'], c['P'], c['C']
        x = val(c['dt'], inp['x']).reshape(B, P, C)
        if fault == 'p_tail_dropped':
            x = x[:, :max(P // 4 * 4, 0)]
        s = np.cumsum(x, axis=1, dtype=F)[:, -1] if x.shape[1] else np.zeros((B, C), F)
        return (s / F(P)).reshape(-1)

    def restate(self, c, inp, fr, fault=None):
        if c['B']:
            fr['out'].region()[0] = self.mean32(c, inp, fault)

    def verify(self, c, inp, got):
        if not c['B']:
            return {}
        B, P, C = c['B'], c['P'], c['C']
        exact(got['out'][0], self.mean32(c, inp), c['name'])       # both kernels: positions ascending, one division
        x = val(c['dt'], inp['x']).astype(np.float64).reshape(B, P, C)
        return {'avgpool': bounded(got['out'][0], x.mean(1).reshape(-1), np.abs(x).mean(1).reshape(-1), P + 1, 'f32', c['name'])}


MP_VALUES = np.array([-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0], F)      # all bf16 values: most 3x3 windows hold a tie


def maxpool_fwd32(x, fault=None):
    """[B, H, W, C] f32 -> (pooled [B, Ho, Wo, C], argmax bytes): 3x3 stride 2 pad 1, the first maximum in scan order (kh, kw) wins"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = np.full((B, Ho, Wo, C), -np.inf, F)
    bi = np.zeros((B, Ho, Wo, C), np.uint8)
    first = np.ones((1, Ho, Wo, 1), bool)
    order = [(kh, kw) for kh in range(3) for kw in range(3)]
    if fault == 'kw_kh_order':
        order = [(kh, kw) for kw in range(3) for kh in range(3)]
    for kh, kw in order:
        hi, wi = 2 * np.arange(Ho) - 1 + kh, 2 * np.arange(Wo) - 1 + kw
        valid = ((hi >= 0) & (hi < H))[:, None] & ((wi >= 0) & (wi < W))[None, :]
        f = x[:, np.clip(hi, 0, H - 1)][:, :, np.clip(wi, 0, W - 1)]
        v4 = valid[None, :, :, None]
        if fault == 'not_clipped':                          # the border taps take part, as zeros
            f, v4 = np.where(v4, f, F(0)), np.ones_like(v4)
        upd = v4 & (first | ((f >= best) if fault == 'last_max_wins' else (f > best)))
        best = np.where(upd, f, best)
        bi = np.where(upd, np.uint8(kh * 3 + kw), bi)
        first = first & ~v4
    return best, bi


def maxpool_bwd32(dy, idx, relu_src, y, H, W):
    B, Ho, Wo, C = dy.shape
    dx = np.zeros((B, H, W, C), F)
    for ho in range(Ho):
        for wo in range(Wo):
            for kh in range(3):
                for kw in range(3):
                    hi, wi = 2 * ho - 1 + kh, 2 * wo - 1 + kw
                    if 0 <= hi < H and 0 <= wi < W:
                        m = idx[:, ho, wo] == kh * 3 + kw
                        if y is not None:
                            m = m & (y[:, ho, wo] > 0)
                        dx[:, hi, wi] += np.where(m, dy[:, ho, wo], F(0))
    if relu_src is not None:
        dx = np.where(relu_src > 0, dx, F(0))
    return dx


@register
class Maxpool(Kernel):
    key = 'maxpool'
    faults = ('last_max_wins', 'kw_kh_order', 'not_clipped')

    def make(self, c):
        r = rng_of(c)
        B, H, W, C, dt = c['B'], c['H'], c['W'], c['C'], c['dt']
        x = MP_VALUES[r.integers(0, len(MP_VALUES), (B, H, W, C))]
        x[0, ..., 0] = -1.0                                  # one channel all negative and all tied: the clipped border must not win
        y, idx = maxpool_fwd32(x)
        # gradients k / 8, |k| <= 16: a sum of up to four is exact in f32 and in bf16
        dy = (r.integers(-16, 17, y.shape) / 8.0).astype(F)
        relu_src = MP_VALUES[r.integers(0, len(MP_VALUES), x.shape)]
        return dict(x=store(dt, x), y=store(dt, y), idx=idx, dy=store(dt, dy), relu_src=store(dt, relu_src))

    def frames(self, c, inp):
        B, H, W, C, dt = c['B'], c['H'], c['W'], c['C'], c['dt']
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return dict(y=Frame(dt, B * Ho * Wo, C), idx=Frame('u8', B * Ho * Wo, C), dx_relu=Frame(dt, B * H * W, C), dx_y=Frame(dt, B * H * W, C),
                    dx_plain=Frame(dt, B * H * W, C))

    def ref(self, c, inp, fault=None):
        B, H, W, C, dt = c['B'], c['H'], c['W'], c['C'], c['dt']
        y, idx = maxpool_fwd32(val(dt, inp['x']), fault)
        dy, rs = val(dt, inp['dy']), val(dt, inp['relu_src'])
        yin, iin = val(dt, inp['y']), inp['idx']            # the backward reads the (reference) forward results
        f2 = lambda a: store(dt, a.reshape(-1, C))
        return dict(y=f2(y), idx=idx.reshape(-1, C), dx_relu=f2(maxpool_bwd32(dy, iin, rs, None, H, W)),
                    dx_y=f2(maxpool_bwd32(dy, iin, None, yin, H, W)), dx_plain=f2(maxpool_bwd32(dy, iin, None, None, H, W)))

    def restate(self, c, inp, fr, fault=None):
        for n, a in self.ref(c, inp, fault).items():
            fr[n].region()[:] = a

    def verify(self, c, inp, got):
        ref = self.ref(c, inp)
        for n in ('y', 'idx', 'dx_relu', 'dx_y', 'dx_plain'):
            exact(got[n], ref[n], f'{c["name"]}.{n}')       # every element: no mismatch fraction
        return {}


# ================================================================================================ positional and layout
def resize_index(n_in, n_out, fault=None):
    """the kernel's source index: min(int(floor(i * (n_in / n_out))), n_in - 1) in f32"""
    s = F(n_in) / F(n_out)
    t = np.arange(n_out, dtype=F) * s
    t = np.rint(t) if fault == 'floor_to_round' else np.floor(t)
    return np.minimum(t.astype(np.int64), n_in - 1)


@register
class MaskResize(Kernel):
    key = 'mask_resize'
    faults = ('floor_to_round', 'last_vector', 'past_n')

    def make(self, c):
        return dict(m=rng_of(c).integers(0, 2, (c['B'], c['Hin'], c['Win'])).astype(np.uint8))

    def frames(self, c, inp):
        return dict(out=Frame('u8', c['B'] * c['Hout'], c['Wout']))

    def restate(self, c, inp, fr, fault=None):
        if c['B']:
            hi, wi = resize_index(c['Hin'], c['Hout'], fault), resize_index(c['Win'], c['Wout'], fault)
            fr['out'].region()[:] = inp['m'][:, hi][:, :, wi].reshape(-1, c['Wout'])

    def verify(self, c, inp, got):
        if not c['B']:
            return {}
        ref = torch.nn.functional.interpolate(torch.from_numpy(inp['m'])[None].float(), size=(c['Hout'], c['Wout']))[0].to(torch.uint8).numpy()
        exact(got['out'], ref.reshape(-1, c['Wout']), c['name'])
        return {}


def posenc_mask(c):
    B, H, W = c['B'], c['H'], c['W']
    m = np.zeros((B, H, W), np.uint8)
    if c['mask'] == 'suffix':
        for b in range(B):
            m[b, H - (b * 7 + 3) % H:] = 1                  # a suffix of its own length per clip (never the whole clip)
    elif c['mask'] == 'column':
        m[:, :, W - 1] = 1                                   # a fully masked column: tot = 0
        m[0, H // 2:, 0] = 1
    elif c['mask'] == 'holes':
        m[:, 1::3, :] = 1
        m[B - 1, 0, 0] = 1
    return m


@register
class Posenc(Kernel):
    key = 'posenc'
    faults = ('cum_not_stopping',)

    def make(self, c):
        return dict(m=posenc_mask(c))

    def frames(self, c, inp):
        return dict(pos=Frame(c['dt'], c['B'] * c['H'] * c['W'], c['D']))

    def arg(self, c, inp, T, fault=None):
        """the sine / cosine argument [B, H, W, D] in the float type T (np.float32: the restatement; np.float64: the reference, which
        takes the kernel's f32 constants as they are)"""
        D = c['D']
        nm = (inp['m'] == 0).astype(T)
        cum, tot = np.cumsum(nm, axis=1, dtype=T), nm.sum(1, keepdims=True, dtype=T)
        if fault == 'cum_not_stopping':
            cum = np.broadcast_to(tot, cum.shape)
        y = cum / (tot + T(F(1e-6))) * T(F(6.283185307179586))
        ch = np.arange(D) // 2 * 2
        dim_t = np.power(T(10000.0), ch.astype(T) / T(D)).astype(T)
        return (y[..., None] / dim_t).astype(T)

    def restate(self, c, inp, fr, fault=None):
        a = self.arg(c, inp, F, fault)
        out = np.where(np.arange(c['D']) % 2 == 0, np.sin(a), np.cos(a)).astype(F)
        fr['pos'].region()[:] = store(c['dt'], out.reshape(-1, c['D']))

    def ref64(self, c, inp):
        a = self.arg(c, inp, np.float64)
        return np.where(np.arange(c['D']) % 2 == 0, np.sin(a), np.cos(a)).reshape(-1, c['D']), np.abs(a).reshape(-1, c['D'])

    def verify(self, c, inp, got):
        ref, a = self.ref64(c, inp)
        gv = val(c['dt'], got['pos'])
        # the argument: cum / (tot + eps) * 2 pi / dim_t - four roundings, and the exponent's rounding, which powf amplifies by
        # ln(10000) c / D <= 9.3; |d sin| <= |d argument|
        extra = K_FN['sin'] * (1 + a) + K_FN['pow'] * a
        out = {'posenc': bounded(gv, ref, 10.0 * a, 4, c['dt'], c['name'], extra + 1.0)}        # (+ 1: the result's own f32 rounding, <= 2^-24)
        if c['dt'] == 'f32':
            out['k:sin+pow(posenc)'] = k_measure(gv, ref, 1 + 2 * a, 10.0 * a)
        return out


def im2col32(x, fault=None):
    """[B, H, W] f32 -> [B * Ho * Wo, 128]: columns [0, 49) the 7x7 stride-2 pad-3 taps, [64, 113) the in-bounds indicators"""
    B, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((B, H + 6, W + 6), F)
    xp[:, 3:3 + H, 3:3 + W] = x
    ip = np.zeros((H + 6, W + 6), F)
    ip[3:3 + H, 3:3 + W] = 1
    col = np.zeros((B, Ho, Wo, 128), F)
    for kh in range(7):
        for kw in range(7):
            col[..., kh * 7 + kw] = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            col[..., 64 + kh * 7 + kw] = ip[kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2][None]
    return col.reshape(-1, 128)


@register
class StemIm2col(Kernel):
    key = 'stem_im2col'

    def make(self, c):
        r = rng_of(c)
        B, H, W = c['B'], c['H'], c['W']
        # pixel row h of clip b at gain(b * H + h), pixel column w at sign(w): a tap from the neighbouring row or column shows
        return dict(x=data(r, B * H, W).reshape(B, H, W))

    def frames(self, c, inp):
        B, H, W = c['B'], c['H'], c['W']
        return dict(col=Frame(c['dt'], B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), 128))

    def restate(self, c, inp, fr, fault=None):
        fr['col'].region()[:] = store(c['dt'], im2col32(inp['x']))

    def verify(self, c, inp, got):
        ref = store(c['dt'], im2col32(inp['x']))
        exact(got['col'], ref, c['name'])
        g = val(c['dt'], got['col'])
        assert (g[:, 49:64] == 0).all() and (g[:, 113:] == 0).all(), f'{c["name"]}: columns 49-63 / 113-127 are not zero'
        assert np.isin(g[:, 64:113], (0.0, 1.0)).all()
        return {}


# ================================================================================================ skinny heads
def _act64(z, act):
    if act == 'relu':
        return np.maximum(z, 0.0)
    if act == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-z))
    return z


def _gprime(g, ys, act, T):
    g, ys = g.astype(T), ys.astype(T)
    if act == 'sigmoid':
        return (g * (ys * (T(1) - ys))).astype(T)
    if act == 'relu':
        return np.where(ys > 0, g, T(0)).astype(T)
    return g


@register
class SkinnyFwd(Kernel):
    key = 'skinny_fwd'
    faults = ('row_tail', 'bias_after_act')
    XOFF, XPAD = 8, 12                                      # the column view: 8 elements in, rows K + 12 apart (no 16-byte row alignment)

    def make(self, c):
        r = rng_of(c)
        M, N, K = c['M'], c['N'], c['K']
        x = data(r, M, K, c['dt'])
        w = data(r, N, K)[::-1].copy() / F(math.sqrt(K) / 4)        # pre-activations of a few units: the sigmoid off its plateaus
        b = (gain(np.arange(N)) * sign(np.arange(N) + 3)).astype(F)
        return dict(x=x, w=w, b=b)

    def out_dt(self, c):
        return 'f32' if c['out_f32'] else c['dt']

    def frames(self, c, inp):
        return dict(y=Frame(self.out_dt(c), c['M'], c['N']), y_view=Frame(self.out_dt(c), c['M'], c['N']))

    def y32(self, c, inp, fault=None):
        """the kernel in np.float32: four fma chains over k = 4 i + j, (a0 + a1) + (a2 + a3), bias, activation"""
        M, N, K = c['M'], c['N'], c['K']
        x, w = val(c['dt'], inp['x']).astype(np.float64), inp['w'].astype(np.float64)
        acc = np.zeros((M, N, 4), F)
        for k in range(K // 4):
            acc = (x[:, None, 4 * k:4 * k + 4] * w[None, :, 4 * k:4 * k + 4] + acc).astype(F)        # fma: one rounding
        z = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
        if c['bias'] and fault != 'bias_after_act':
            z = z + inp['b'][None]
        if c['act'] == 'relu':
            z = np.maximum(z, F(0))
        elif c['act'] == 'sigmoid':
            z = F(1) / (F(1) + np.exp(-z).astype(F))
        if c['bias'] and fault == 'bias_after_act':
            z = z + inp['b'][None]
        return store(self.out_dt(c), z.astype(F))

    def restate(self, c, inp, fr, fault=None):
        y = self.y32(c, inp, fault)
        for n in ('y', 'y_view'):
            fr[n].region()[:] = y
        if fault == 'row_tail':                             # rows M .. (the block's 16) are not cut off: written behind the output
            f = fr['y']
            extra = min((-c['M']) % 16 * c['N'], GUARD)
            f.buf[f.off + f.span:f.off + f.span + extra] = 0

    def verify(self, c, inp, got):
        x, w = val(c['dt'], inp['x']).astype(np.float64), inp['w'].astype(np.float64)
        z, ab = x @ w.T, np.abs(x) @ np.abs(w).T
        if c['bias']:
            z, ab = z + inp['b'][None], ab + np.abs(inp['b'])[None]
        ref, extra = _act64(z, c['act']), None
        if c['act'] == 'sigmoid':
            d = ref * (1 - ref)
            ab = d * ab + ref                               # the pre-activation's error through sigma', and the two roundings of 1 / (1 + e)
            extra = K_FN['nexp'] * d * (1 + np.abs(z))
        exact(got['y_view'], got['y'], c['name'] + ': the scalar loader (column view) against the vector loader')
        gv = val(self.out_dt(c), got['y'])
        key = 'skinny_fwd ' + c['act']
        out = {key: bounded(gv, ref, ab, c['K'] + 1, self.out_dt(c), c['name'], extra)}
        if c['act'] == 'sigmoid' and c['out_f32']:
            out['k:nexp(skinny sigmoid)'] = k_measure(gv, ref, ref * (1 - ref) * (1 + np.abs(z)), ab)
        return out


@register
class SkinnyDgrad(Kernel):
    key = 'skinny_dgrad'
    ACC_PAD = 8

    def make(self, c):
        r = rng_of(c)
        M, N, K, dt = c['M'], c['N'], c['K'], c['dt']
        g = data(r, M, N)
        ys = r.random((M, N)).astype(F)
        if c['act'] == 'relu':
            ys = np.where(r.random((M, N)) < 0.5, ys, F(0))
        w = data(r, N, K)[::-1].copy()
        mask = quant(dt, np.where(r.random((M, K)) < 0.5, F(1), F(-1)) * (0.5 + r.random((M, K))).astype(F))
        old = data(r, M, K + self.ACC_PAD, dt)
        return dict(g=g, ys=ys, w=w, mask=mask, old=old)

    def frames(self, c, inp):
        M, K = c['M'], c['K']
        f = Frame(c['dt'], M, K, K + self.ACC_PAD if c['acc'] else K)
        if c['acc']:
            f.region()[:] = inp['old'][:, :K]               # the running input gradient the launch adds to
        return dict(gx=f)

    def parts(self, c, inp, T):
        gp = _gprime(inp['g'], inp['ys'], c['act'], T)
        w = inp['w'].astype(T)
        old = val(c['dt'], inp['old'])[:, :c['K']].astype(T) if c['acc'] else None
        return gp, w, old

    def restate(self, c, inp, fr, fault=None):
        gp, w, old = self.parts(c, inp, F)
        acc = np.zeros((c['M'], c['K']), F)
        for n in range(c['N']):
            acc = (gp[:, n, None].astype(np.float64) * w[None, n].astype(np.float64) + acc).astype(F)
        if old is not None:
            acc = acc + old
        if c['mask']:
            acc = np.where(val(c['dt'], inp['mask']) > 0, acc, F(0))
        fr['gx'].region()[:] = store(c['dt'], acc)

    def verify(self, c, inp, got):
        gp, w, old = self.parts(c, inp, np.float64)
        ref, ab = gp @ w, np.abs(gp) @ np.abs(w)
        if old is not None:
            ref, ab = ref + old, ab + np.abs(old)
        if c['mask']:
            m = val(c['dt'], inp['mask']) > 0
            assert (bits(got['gx'])[~m] == 0).all(), f'{c["name"]}: a masked element is not +0'
            ref, ab = np.where(m, ref, 0.0), np.where(m, ab, 0.0)
        # N products, the accumulated input, and the (up to three) roundings of g' = g s (1 - s)
        return {'skinny_dgrad': bounded(val(c['dt'], got['gx']), ref, ab, c['N'] + 4, c['dt'], c['name'])}


@register
class SkinnyWgrad(Kernel):
    key = 'skinny_wgrad'

    def make(self, c):
        r = rng_of(c)
        M, N, K = c['M'], c['N'], c['K']
        g = data(r, M, N)
        ys = r.random((M, N)).astype(F)
        if c['act'] == 'relu':
            ys = np.where(r.random((M, N)) < 0.5, ys, F(0))
        return dict(g=g, ys=ys, x=data(r, M, K, c['dt']))

    def frames(self, c, inp):
        fr = dict(dw=Frame('f32', c['N'], c['K']))
        if c['db']:
            fr['db'] = Frame('f32', 1, c['N'])
        return fr

    def restate(self, c, inp, fr, fault=None):
        gp = _gprime(inp['g'], inp['ys'], c['act'], F)
        x = val(c['dt'], inp['x'])
        for n in range(c['N']):
            fr['dw'].region()[n] = self.tree32(gp[:, n, None] * x)
        if c['db']:
            fr['db'].region()[0] = self.tree32(gp)

    @staticmethod
    def tree32(t):
        """the kernels' order over the rows of t [M, cols]: 16 row slices, four sub-groups each (rows sub, sub + 4, ... in order), the four
        added left to right, the 16 slice sums added in order (the products rounded to f32 first, where the kernel has an fma)"""
        M = t.shape[0]
        per = (M + 15) // 16
        part = np.zeros((16,) + t.shape[1:], F)
        for z in range(16):
            m0, m1 = z * per, min(M, z * per + per)
            s = [np.cumsum(t[m0 + u:m1:4], axis=0, dtype=F)[-1] if m0 + u < m1 else np.zeros(t.shape[1:], F) for u in range(4)]
            part[z] = ((s[0] + s[1]) + s[2]) + s[3]
        return np.cumsum(part, axis=0, dtype=F)[-1]

    def verify(self, c, inp, got):
        gp = _gprime(inp['g'], inp['ys'], c['act'], np.float64)
        x = val(c['dt'], inp['x']).astype(np.float64)
        K = c['M'] + 3                                      # M products and the roundings of g'
        out = {'skinny_wgrad dW': bounded(got['dw'], gp.T @ x, np.abs(gp).T @ np.abs(x), K, 'f32', c['name'] + '.dw')}
        if c['db']:
            out['skinny_wgrad db'] = bounded(got['db'][0], gp.sum(0), np.abs(gp).sum(0), K, 'f32', c['name'] + '.db')
        return out


# the injected faults of tests/test_glue_check_cpu.py: (kernel key, fault) - each must fail at least one row of that kernel
FAULTS = [('add', 'last_vector'), ('gelu', 'last_vector'), ('mask_resize', 'last_vector'), ('add', 'past_n'), ('cast', 'past_n'),
          ('relu_mask', 'past_n'), ('add', 'b_mod_ignored'), ('add_n', 'source_dropped'), ('dropout_grad', 'index_from_ld'),
          ('split3', 'hi_lo_hi'), ('dec_in', 'keep_index_bQ'), ('dec_in_bwd', 'clip_tail_dropped'), ('colsum', 'last_chunk_dropped'),
          ('avgpool', 'p_tail_dropped'), ('maxpool', 'last_max_wins'), ('maxpool', 'kw_kh_order'), ('maxpool', 'not_clipped'),
          ('mask_resize', 'floor_to_round'), ('posenc', 'cum_not_stopping'), ('skinny_fwd', 'row_tail'), ('skinny_fwd', 'bias_after_act')]
