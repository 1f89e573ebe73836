"""Float64 references, bounds, guard frames and numpy restatements for the seven kernels of csrc/input.hip (box_transform,
box_transform_views, scaler_clip_stats + scaler_accumulate, mixup, mixup_targets, query_patch).  A helper of
tests/test_input_envelope_gpu.py and tests/test_input_check_cpu.py, not a conftest; the rows are in tests/input_cases.py.

One Kernel object per kernel key: make(row) -> the inputs (numpy), frames(row, inputs) -> the outputs as Frames, restate(row, inputs,
frames, fault) -> the kernel restated in np.float32 in the kernel's own summation order, writing into the frames' host images,
verify(row, inputs, images) -> the checks, returning the largest error / bound ratios.  The GPU module uploads the same inputs and frame
images, launches on pointers into the frames, reads the images back and calls verify(): the device result and the restatement go through
the same checks.  restate() takes a `fault` (FAULTS): a deliberately wrong variant that at least one row must reject.

Inputs.  amp[b, r, c] = clip gain (1e-3 .. 1e1, its own decade per clip) x band factor (1, 1e-1, 1e-2, 1e-3 by c % 4) x u[0.25, 1.25), one
element in 16 another 1e-3 lower (so that the 80 dB floor clamps something); the raw rows a PadOrTrunc drops (r >= frames) are 300 x louder,
so that the clip maximum lies in rows the output never shows.  The rows of box_transform_views have neither (|x + sd z| must stay away
from 0, below): there every fourth band lies 1e-5 down instead, under the floor.  A row or band taken from a neighbour is wrong by a
large factor.  Rows >= nframes_raw of amp and of the injected normals are poison: NaN in even clips, 1e30 in odd ones.

Guard frame.  A Frame is one buffer filled with 0xFF bytes (NaN in f32 / f64) or 0xA5 (integers) that holds the output GUARD = 32 elements
from either end.  After a launch no byte outside the owned elements may differ from the fill, and the exact kernels compare their WHOLE
image - elements past the merged totals of the label merge included - with the expected image.

References.  The chain after the dB step is oracle.transforms_oracle (pad_trunc, time_mask, freq_mask, freq_shift, normalize) on float64;
the dB step is its amplitude_to_db fed float64 amplitudes.  The label merge is utilities.mixup.plan_mixup_label_unlabel (its decisions
are also written down by hand per designed pair: EXPECT); the query patches are the body of transforms_oracle.query_patches on given rows.

Compared exactly (bits): labels, offsets, job records, ratios, copied boxes; mixup modes 1 and 2; query patches; every element whose
reference carries no rounding before the normalisation (PadOrTrunc zeros, time mask, wrapped shift bands, the constant fill, and every
element of an apply_log = 0 clean view: there expected = f32((v - mean) / std) in float64, the kernel's own expression); the guards.
The filled bands of a mean fill must hold one bit pattern per output column.

Bounds, per element, u = 2^-24, DB = 10 / ln 10, all multiplied by C = 2 (the safety constant of tests/gemm_check.py):
  * dB value v = 10 log10(max(1e-10, x x)) in f32: the square's rounding moves v by DB u, the f32 constant 1e-10f by another DB u; the
    device log10f is taken as 2 ulp (the OpenCL full-profile figure the ROCm device library states it meets; its table is not on this
    machine - an assumption), the multiply by 10 half an ulp: e(v) = 2 DB u + 5 u |v|.
  * floor: max() is 1-Lipschitz: an element within e of the floor gets max(e(own), e(clip maximum)).
  * mean fill over n = frames x f elements: the kernel adds ceil(n / 1024) terms per thread, 6 butterfly levels, 16 wave partials and
    divides once: (ceil(n / 1024) + 22) u mean|terms| + u |fill| + the largest e among its terms.
  * normalisation in float64, rounded once: e / std[c] + u |out|.
  * noisy view: sd[c] = sqrt(sum / nraw): each term fl(fl(x x) pow) has two roundings, the sum ceil(nraw / G) + G adds, one divide;
    halved by the square root, which is taken as 1 ulp (2 u): rel(sd) = ((3 + ceil(nraw / G) + G) / 2 + 2) u.  x + sd z costs two roundings:
    delta = |sd z| (rel(sd) + u) + u |x + sd z| (+ |sd| 1e-4 when the kernel draws z: the |z_dev - z_mirror| bound
    tests/test_noise_views_gpu.py derives).  d/dx 10 log10(x^2) = 2 DB / x, so e(v) += 2 DB delta / |x + sd z|; the rows keep
    |x + sd z| >= |x| / 2 (amplitudes are positive, the SNR is 30 dB), asserted on the reference.
  * scaler: mean(v): sum of e over the kept rows / frames; mean(fl32(v v)): sum of (2 |v| e + u v^2) / frames; the double accumulation
    adds 2^-50 of the sum of magnitudes.
  * mix mode 0: 2^-23 (|l p| + |m q|) exactly as derived (contracted or not), no constant on top.
The np.float32 restatements reach 0.33 - 0.5 of these bounds, mix mode 0 0.96 (tests/test_input_check_cpu.py prints them): none is
loose by more than the constant C and a factor of about two.

The h == 128 branch of query_patch_kernel copies the codes; Pillow's resampler at scale 1 gives the same bits (weights 1 and 0, see
test_resampler_at_128_rows_is_the_copy), so "copy branch replaced by the resampler" is not observable and is no fault here; the
neighbouring mistake that is - the copy taken for h >= 128 - is ('query_patches', 'copy_branch_from_128').
"""
import math
import zlib

import numpy as np
import torch

from oracle import transforms_oracle as TO
import input_cases as IC
import noise_views_ref as R

F32 = np.float32
U = 2.0 ** -24
C_SAFE = 2.0
DB = 10.0 / math.log(10.0)
K_LOG = 5.0
E_SQ = 2.0 * DB * U
Z_TOL = 1e-4
TINY = 1e-30
GUARD = 32
SNR = 30.0
NOISE_POW = float(F32(10.0 ** (-SNR / 10.0)))
LAM = 0.37
_FILL = {np.dtype(np.float32): 0xFF, np.dtype(np.float64): 0xFF, np.dtype(np.int32): 0xA5, np.dtype(np.int64): 0xA5, np.dtype(np.uint8): 0xA5}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def rng_of(c, salt=0):
    return np.random.default_rng(zlib.crc32(c['name'].split('_log')[0].encode()) + salt)


class Frame(object):
    """`n` elements of `dtype` inside one filled buffer, GUARD elements in front and behind.  buf is the host image."""

    def __init__(self, dtype, n):
        self.dtype, self.n = np.dtype(dtype), int(n)
        self.buf = np.full((self.n + 2 * GUARD) * self.dtype.itemsize, _FILL[self.dtype], np.uint8).view(self.dtype)

    def own(self, img=None):
        return (self.buf if img is None else img)[GUARD:GUARD + self.n]

    def blank(self):
        return Frame(self.dtype, self.n).buf

    def check_guard(self, img, what):
        assert img.shape == self.buf.shape and img.dtype == self.dtype, what
        b, f = bits(img), bits(self.blank())
        bad = b != f
        bad[GUARD:GUARD + self.n] = False
        assert not bad.any(), f'{what}: {int(bad.sum())} guard elements changed, first at offset {int(np.nonzero(bad)[0][0]) - GUARD} of {self.n}'


def exact(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {tuple(int(k) for k in i)}: '
                             f'got {got[tuple(i)]!r} want {want[tuple(i)]!r}')
    return 0.0


def bounded(got, ref, bound, what):
    """|got - ref| <= C bound + tiny per element; returns the largest ratio"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    if got.size == 0:
        return 0.0
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    bad = ~np.isfinite(got)
    if bad.any():
        raise AssertionError(f'{what}: {int(bad.sum())} non-finite (unwritten or poisoned) elements, first at {tuple(int(k) for k in np.argwhere(bad)[0])}')
    ratio = np.abs(got - ref) / (C_SAFE * bound + TINY)
    w = float(ratio.max())
    if w > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f'{what}: {int((ratio > 1).sum())} of {ratio.size} elements over the bound (worst ratio {w:.3g} at {tuple(int(k) for k in i)}: '
                             f'got {got[i]:.9g} ref {ref[i]:.9g} bound {C_SAFE * bound[i]:.3g})')
    return w


# ------------------------------------------------------------------------------------------------ inputs of the clip kernels
def amp_batch(c, nraws, salt=0, views=False):
    """flat [B, stride, F] f32 amplitudes of the module header, rows >= nraws[b] poisoned.  views: the form of the noisy rows (header)"""
    F, frames, stride = c['F'], c['frames'], IC.raw_stride(c)
    r = rng_of(c, salt)
    B = len(nraws)
    a = 0.25 + r.random((B, stride, F))
    if views:
        a *= (10.0 ** -np.asarray([0, 1, 2, 5])[np.arange(F) % 4])[None, None, :]
    else:
        a *= (10.0 ** -(np.arange(F) % 4))[None, None, :]
        a *= np.where(r.random((B, stride, F)) < 1.0 / 16, 1e-3, 1.0)
        a[:, frames:] *= 300.0
    a *= (10.0 ** (-3.0 + 1.3 * ((np.arange(B) + salt) % 4)))[:, None, None] * (1.0 + 0.25 * (np.arange(B) % 3))[:, None, None]
    for b in c.get('silent_clips', ()):
        a[b] = 0.0
    for b, bands in c.get('silent_bands', {}).items():
        a[b][:, list(bands)] = 0.0
    a = a.astype(F32)
    for b, n in enumerate(nraws):
        a[b, max(min(n, stride), 0):] = np.nan if b % 2 == 0 else 1e30
    return a


def scaler_vectors(c):
    r = rng_of(c, 77)
    return r.standard_normal(c['F']) * 3.0 - 30.0, r.random(c['F']) * 5.0 + 8.0


def clip_rows(flat, b, nraw, stride, F, fault=None):
    """the nraw raw rows of clip b of a flat batch"""
    base = b * (nraw if fault == 'stride_is_nraw' else stride) * F
    return flat.reshape(-1)[base:base + nraw * F].reshape(nraw, F)


def _wave_block_sum(s):
    """block_sum of csrc/input.hip on the 1024 per-thread partials: xor butterfly 32..1 per wave, then the 16 wave sums in index order"""
    v = s.reshape(16, 64).astype(F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ o]).astype(F32)
    t = F32(0)
    for w in range(16):
        t = F32(t + v[w, 0])
    return t


def chain(x, delta, rec, c, mean, std, f32mode, fault=None):
    """one clip through box_transform_kernel from its raw rows x [nraw, F] (float64 reference with bounds, or np.float32 in the kernel's
    order).  delta: float64 amplitude error of x (a noisy view) or None.  Returns (out [frames, F], E or None, exact mask or None, fill
    columns of the output)."""
    nraw, tm_t, tm_t0, fm_f, fm_f0, fm_on, sh = (int(k) for k in rec[:7])
    frames, F, log = c['frames'], c['F'], c['log']
    T = F32 if f32mode else np.float64
    x = x.astype(T)
    e = None
    if log:
        if f32mode:
            v = (F32(10) * np.log10(np.maximum(F32(1e-10), (x * x).astype(F32)))).astype(F32)
        elif nraw:
            v = TO.amplitude_to_db(x.T, top_db=None).T
            e = E_SQ + K_LOG * U * np.abs(v)
            if delta is not None:
                e = e + np.where(delta > 0, 2.0 * DB * delta / np.maximum(np.abs(x), TINY), 0.0)
        else:
            v, e = x, np.zeros_like(x)
    else:
        v = x
        e = None if f32mode else (delta if delta is not None else np.zeros_like(x))
    keep = min(nraw, frames)
    top = v[:keep] if fault == 'floor_from_kept' else v
    mx = top.max() if top.size else T(-np.inf)
    floor = T(mx - T(80))
    clip = np.zeros((frames, F), T)
    kept = v[:keep]
    if log and keep:
        if not f32mode:
            e_mx = e[v >= mx - 2.0 * e.max()].max()
            e = np.where(kept <= floor + e[:keep] + e_mx, np.maximum(e[:keep], e_mx), e[:keep])
        kept = np.maximum(kept, floor)
    clip[:keep] = kept
    E = None
    if not f32mode:
        E = np.zeros((frames, F))
        E[:keep] = e[:keep]
    t_end = tm_t0 + tm_t + (1 if fault == 'mask_end_inclusive' and tm_t > 0 else 0)
    if tm_t > 0:
        clip[max(tm_t0, 0):t_end] = 0
        if E is not None:
            E[max(tm_t0, 0):t_end] = 0
    fill_cols = []
    if fm_on and fm_f > 0:
        f_end = min(F, fm_f0 + fm_f + (1 if fault == 'mask_end_inclusive' else 0))
        reg = clip[:, fm_f0:f_end]
        if c.get('fill_mean', 1):
            n = reg.size
            if f32mode:
                flat = np.zeros(IC.trips(n) * 1024, F32)
                flat[:n] = reg.reshape(-1)
                s = np.zeros(1024, F32)
                for row in flat.reshape(-1, 1024):
                    s = (s + row).astype(F32)
                fill = F32(_wave_block_sum(s) / F32(n))
            else:
                fill = reg.mean()
                e_fill = (IC.trips(n) + 22) * U * np.abs(reg).mean() + U * abs(fill) + E[:, fm_f0:f_end].max()
        else:
            fill, e_fill = T(F32(c['fill_const'])), 0.0
        clip[:, fm_f0:f_end] = fill
        if E is not None:
            E[:, fm_f0:f_end] = e_fill
        fill_cols = [k + sh for k in range(fm_f0, f_end) if 0 <= k + sh < F]
    if fault == 'shift_off_by_one' and sh:                  # the wrapped band next to the zeroed ones keeps what np.roll brought round
        rolled = np.roll(clip, sh, axis=1)
        if sh > 0:
            rolled[:, :sh - 1] = 0
        else:
            rolled[:, F + sh + 1:] = 0
        clip = rolled
    else:
        clip = TO.freq_shift(clip, True, sh)
        if E is not None:
            E = TO.freq_shift(E, True, sh)
    ex = None if E is None else E == 0
    if mean is not None:
        if f32mode:
            clip = TO.normalize(clip.astype(np.float64), mean, std).astype(F32)
        else:
            clip = TO.normalize(clip, mean, std)
            E = E / std[None, :] + U * np.abs(clip)
    return clip, E, ex, fill_cols


def check_view(got, ref, E, ex, fill_cols, what):
    """one clip of a transform output against its reference: exact positions on bits, the rest under the bound, filled columns uniform"""
    assert np.isfinite(ref).all(), what
    exact(got[ex], ref[ex].astype(F32), what + ' (exact positions)')
    r = bounded(got[~ex], ref[~ex], E[~ex], what)
    for k in fill_cols:
        assert (bits(got[:, k]) == bits(got[:1, k])[0]).all(), f'{what}: filled column {k} is not uniform'
    return r


class Kernel(object):
    faults = ()


KERNELS = {}
_REF = {}


def register(cls):
    KERNELS[cls.key] = cls()
    return cls


def cached(key, c, fn):
    k = (key, c['name'])
    if k not in _REF:
        _REF[k] = fn()
    return _REF[k]


def images(fr):
    return {n: f.buf for n, f in fr.items()}


def restated(key, c, fault=None):
    """the row through the numpy restatement (with an injected fault, if any) and the same verification as a device result"""
    k = KERNELS[key]
    inp = k.make(c)
    fr = k.frames(c, inp)
    with np.errstate(over='ignore', invalid='ignore'):        # a fault may read the poison rows
        k.restate(c, inp, fr, fault)
    return k.verify(c, inp, fr, images(fr))


def guards(c, fr, img):
    for n, f in fr.items():
        f.check_guard(img[n], f'{c["name"]}.{n}')


# ================================================================================================ box_transform
@register
class BoxTransform(Kernel):
    key = 'box_transform'
    faults = ('shift_off_by_one', 'mask_end_inclusive', 'floor_from_kept', 'stride_is_nraw', 'unwritten_tail')

    def make(self, c):
        recs = np.zeros((len(c['recs']), 8), np.int32)
        recs[:, :7] = c['recs']
        mean, std = scaler_vectors(c) if c['norm'] else (None, None)
        return dict(amp=amp_batch(c, [r[0] for r in c['recs']]), recs=recs, mean=mean, std=std)

    def frames(self, c, inp):
        return dict(out=Frame(F32, len(c['recs']) * c['frames'] * c['F']))

    def restate(self, c, inp, fr, fault=None):
        out = fr['out'].own().reshape(len(c['recs']), c['frames'], c['F'])
        for b, r in enumerate(inp['recs']):
            x = clip_rows(inp['amp'], b, int(r[0]), IC.raw_stride(c), c['F'], fault)
            out[b] = chain(x, None, r, c, inp['mean'], inp['std'], True, fault)[0]
        if fault == 'unwritten_tail':
            fr['out'].own()[-1:] = fr['out'].blank()[:1]

    def reference(self, c, inp):
        return cached(self.key, c, lambda: [chain(clip_rows(inp['amp'], b, int(r[0]), IC.raw_stride(c), c['F']), None, r, c, inp['mean'],
                                                  inp['std'], False) for b, r in enumerate(inp['recs'])])

    def verify(self, c, inp, fr, img):
        guards(c, fr, img)
        got = fr['out'].own(img['out']).reshape(len(c['recs']), c['frames'], c['F'])
        w = 0.0
        for b, (ref, E, ex, cols) in enumerate(self.reference(c, inp)):
            w = max(w, check_view(got[b], ref, E, ex, cols, f'{c["name"]} clip {b}'))
        return {'box_transform': w}


# ================================================================================================ box_transform_views
def noise_std(x, nraw, F, f32mode, fault=None, frames=None):
    """sd[c] of the noisy view from the raw rows x [nraw, F]: kernel order in f32, or float64 with its relative bound"""
    G = IC.groups(F)
    div = frames if fault == 'sd_div_frames' else nraw
    if not f32mode:
        x = x.astype(np.float64)
        sd = np.sqrt((x * x * NOISE_POW).sum(0) / max(div, 1)) if nraw else np.zeros(F)
        return sd, ((3 + IC.trips(nraw, G) + G) / 2.0 + 2.0) * U
    part = np.zeros((G, F), F32)
    for k in range(IC.trips(nraw, G)):
        blk = x[k * G:(k + 1) * G].astype(F32)
        part[:len(blk)] = (part[:len(blk)] + ((blk * blk).astype(F32) * F32(NOISE_POW)).astype(F32)).astype(F32)
    s = np.zeros(F, F32)
    for q in range(G):
        s = (s + part[q]).astype(F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt((s / F32(div)).astype(F32)).astype(F32), None


@register
class BoxTransformViews(Kernel):
    key = 'box_transform_views'
    faults = ('sd_div_frames', 'stride_is_nraw', 'shift_off_by_one', 'mask_end_inclusive', 'view1_takes_record0')

    def make(self, c):
        B = len(c['recs'])
        recs = np.zeros((B, 18), np.int32)
        for b, (r0, r1, on) in enumerate(c['recs']):
            recs[b, 0:7], recs[b, 8:15], recs[b, 16] = r0, r1, on
        nraws = [r[0][0] for r in c['recs']]
        amp = amp_batch(c, nraws, views=True)
        F, stride = c['F'], IC.raw_stride(c)
        if c.get('drawn'):
            z = np.zeros((B, stride, F), F32)
            for b, n in enumerate(nraws):
                z[b, :n] = R.normals(c['seed'], c['offset'] + b * stride * F, n * F).reshape(n, F)
        else:
            z = rng_of(c, 5).standard_normal((B, stride, F)).astype(F32)
            for b, n in enumerate(nraws):
                z[b, n:] = np.nan if b % 2 == 0 else 1e30
        mean, std = scaler_vectors(c) if c['norm'] else (None, None)
        return dict(amp=amp, z=z, recs=recs, mean=mean, std=std)

    def frames(self, c, inp):
        n = len(c['recs']) * c['frames'] * c['F']
        return dict(out0=Frame(F32, n), out1=Frame(F32, n))

    def _views(self, c, inp, f32mode, fault=None):
        F, stride, frames = c['F'], IC.raw_stride(c), c['frames']
        res = []
        for b, row in enumerate(inp['recs']):
            r0, r1, on = row[0:8], row[8:16], int(row[16])
            if fault == 'view1_takes_record0':
                r1 = r0
            nraw = int(r0[0])
            x = clip_rows(inp['amp'], b, nraw, stride, F, fault)
            pair = [chain(x, None, r0, c, inp['mean'], inp['std'], f32mode, fault)]
            if on:
                z = clip_rows(inp['z'], b, nraw, stride, F, fault)
                sd, rel = noise_std(x, nraw, F, f32mode, fault, frames)
                if f32mode:
                    xn, delta = (x + (sd[None, :] * z).astype(F32)).astype(F32), None
                else:
                    sz = sd[None, :] * z.astype(np.float64)
                    xn = x.astype(np.float64) + sz
                    delta = np.abs(sz) * (rel + U) + U * np.abs(xn) + (np.abs(sd)[None, :] * Z_TOL if c.get('drawn') else 0.0)
                    assert (np.abs(xn) >= 0.5 * np.abs(x)).all(), (c['name'], b, 'x + sd z comes too close to 0 for a dB bound')
                pair.append(chain(xn, delta, r1, c, inp['mean'], inp['std'], f32mode, fault))
            else:
                pair.append(chain(x, None, r1, c, inp['mean'], inp['std'], f32mode, fault))
            res.append(pair)
        return res

    def restate(self, c, inp, fr, fault=None):
        B = len(c['recs'])
        o = [fr[n].own().reshape(B, c['frames'], c['F']) for n in ('out0', 'out1')]
        for b, pair in enumerate(self._views(c, inp, True, fault)):
            o[0][b], o[1][b] = pair[0][0], pair[1][0]

    def reference(self, c, inp):
        return cached(self.key, c, lambda: self._views(c, inp, False))

    def verify(self, c, inp, fr, img):
        guards(c, fr, img)
        B = len(c['recs'])
        got = [fr[n].own(img[n]).reshape(B, c['frames'], c['F']) for n in ('out0', 'out1')]
        w = {'views.clean': 0.0, 'views.noisy': 0.0}
        for b, pair in enumerate(self.reference(c, inp)):
            for k in (0, 1):
                name = 'views.noisy' if k and inp['recs'][b, 16] else 'views.clean'
                w[name] = max(w[name], check_view(got[k][b], *pair[k], f'{c["name"]} clip {b} view {k}'))
        return w

    def single_view_rows(self, c, inp):
        """(k, clips, records [n, 8]) of the views the single-view kernel must reproduce bit for bit: view 0 and each clean view 1"""
        r = inp['recs']
        clean = [b for b in range(len(r)) if not r[b, 16]]
        return [(0, list(range(len(r))), r[:, 0:8].copy()), (1, clean, r[clean, 8:16].copy())]


# ================================================================================================ scaler_update
@register
class Scaler(Kernel):
    key = 'scaler_update'
    faults = ('divisor_keep', 'stride_is_nraw', 'floor_from_kept', 'no_clamp')

    def eff(self, c, n):
        return min(max(int(n), 0), IC.raw_stride(c))

    def make(self, c):
        r = rng_of(c, 9)
        acc0 = r.standard_normal(2 * c['F']) * 100.0
        calls = [dict(nf=np.asarray(nf, np.int64).astype(np.int32), amp=amp_batch(c, [self.eff(c, n) for n in nf], salt=i))
                 for i, nf in enumerate(c['calls'])]
        return dict(calls=calls, acc0=acc0, count0=np.asarray([41], np.int64))

    def frames(self, c, inp):
        F = c['F']
        fr = {f'stats{i}': Frame(np.float64, len(k['nf']) * 2 * F) for i, k in enumerate(inp['calls'])}
        fr['stats_cat'] = Frame(np.float64, sum(len(k['nf']) for k in inp['calls']) * 2 * F)
        for n in ('acc', 'acc_cat'):
            fr[n] = Frame(np.float64, 2 * F)
            fr[n].own()[:] = inp['acc0']
        for n in ('count', 'count_cat'):
            fr[n] = Frame(np.int64, 1)
            fr[n].own()[:] = inp['count0']
        return fr

    def _clip(self, c, call, b, f32mode, fault=None):
        """[2, F] statistics of one clip (float64 reference with bound, or the kernel's order)"""
        F, frames, stride = c['F'], c['frames'], IC.raw_stride(c)
        nraw = self.eff(c, call['nf'][b])
        x = clip_rows(call['amp'], b, nraw, stride, F, fault)
        if fault == 'no_clamp' and call['nf'][b] > stride:      # rows past the batch's: whatever lies there
            x, nraw = np.concatenate([x, np.full((1, F), np.nan, F32)]), nraw + 1
        keep = min(nraw, frames)
        T = F32 if f32mode else np.float64
        x = x.astype(T)
        if c['log']:
            if f32mode:
                v = (F32(10) * np.log10(np.maximum(F32(1e-10), (x * x).astype(F32)))).astype(F32)
            else:
                v = TO.amplitude_to_db(x.T, top_db=None).T if nraw else x
                e = E_SQ + K_LOG * U * np.abs(v)
        else:
            v, e = x, np.zeros(x.shape)
        top = v[:keep] if fault == 'floor_from_kept' else v
        mx = top.max() if top.size else T(-np.inf)
        floor = T(mx - T(80))
        kept = v[:keep]
        div = float(max(keep, 1) if fault == 'divisor_keep' else frames)
        if f32mode:
            if c['log']:
                kept = np.maximum(kept, floor)
            G = IC.groups(F)
            part = np.zeros((2, G, F))
            for k in range(IC.trips(keep, G)):
                blk = kept[k * G:(k + 1) * G]
                part[0, :len(blk)] += blk.astype(np.float64)
                part[1, :len(blk)] += (blk * blk).astype(F32).astype(np.float64)      # rounded to f32 like the reference's array ** 2
            s = np.zeros((2, F))
            for q in range(G):
                s += part[:, q]
            return s / div, None
        if c['log'] and keep:
            e_mx = e[v >= mx - 2.0 * e.max()].max()
            e = np.where(kept <= floor + e[:keep] + e_mx, np.maximum(e[:keep], e_mx), e[:keep])
            kept = np.maximum(kept, floor)
        else:
            e = e[:keep]
        ref = np.stack([kept.sum(0), (kept * kept).sum(0)]) / div
        bound = np.stack([e.sum(0) + 2.0 ** -50 * np.abs(kept).sum(0), (2 * np.abs(kept) * e + (U + 2.0 ** -50) * kept * kept).sum(0)]) / div
        return ref, bound

    def restate(self, c, inp, fr, fault=None):
        F = c['F']
        allst = []
        for i, call in enumerate(inp['calls']):
            st = np.stack([self._clip(c, call, b, True, fault)[0] for b in range(len(call['nf']))])
            fr[f'stats{i}'].own()[:] = st.reshape(-1)
            allst.append(st)
            acc = fr['acc'].own()
            for s in st:                                    # scaler_accumulate_kernel: clip order
                acc += s.reshape(-1)
            fr['count'].own()[0] += len(st)
        cat = np.concatenate(allst)
        fr['stats_cat'].own()[:] = cat.reshape(-1)
        for s in cat:
            fr['acc_cat'].own()[:] += s.reshape(-1)
        fr['count_cat'].own()[0] += len(cat)

    def reference(self, c, inp):
        return cached(self.key, c, lambda: [[self._clip(c, call, b, False) for b in range(len(call['nf']))] for call in inp['calls']])

    def verify(self, c, inp, fr, img):
        guards(c, fr, img)
        F = c['F']
        ref = self.reference(c, inp)
        w = {'scaler.clip_stats': 0.0, 'scaler.acc': 0.0}
        for i, call in enumerate(ref):
            got = fr[f'stats{i}'].own(img[f'stats{i}']).reshape(len(call), 2, F)
            for b, (r, bd) in enumerate(call):
                w['scaler.clip_stats'] = max(w['scaler.clip_stats'], bounded(got[b], r, bd, f'{c["name"]} call {i} clip {b}'))
        flat = [p for call in ref for p in call]
        tot = inp['acc0'].reshape(2, F) + sum(r for r, _ in flat)
        bd = sum(b for _, b in flat) + 2.0 ** -50 * (np.abs(inp['acc0'].reshape(2, F)) + sum(np.abs(r) for r, _ in flat))
        acc = fr['acc'].own(img['acc'])
        w['scaler.acc'] = bounded(acc.reshape(2, F), tot, bd, f'{c["name"]} accumulators')
        exact(fr['acc_cat'].own(img['acc_cat']), acc, f'{c["name"]}: two calls against one call over the concatenation')
        exact(fr['stats_cat'].own(img['stats_cat']), np.concatenate([fr[f'stats{i}'].own(img[f'stats{i}']) for i in range(len(ref))]),
              f'{c["name"]}: clip statistics of the concatenation')
        for n in ('count', 'count_cat'):
            exact(fr[n].own(img[n]), inp['count0'] + len(flat), f'{c["name"]}.{n}')
        return w


# ================================================================================================ mixup
JOB = np.dtype([('src1', np.int32), ('src2', np.int32), ('mode', np.int32), ('lam', np.float32)])


@register
class Mixup(Kernel):
    key = 'mixup'
    faults = ('last_float4_dropped', 'src_is_row', 'second_trip_skipped', 'lam_swapped')

    def make(self, c):
        n = 4 * c['clip4'] + c['rem']
        r = rng_of(c)
        g = (10.0 ** (np.arange(3) - 1.0))[:, None]
        x1 = ((0.5 + r.random((3, n))) * g * np.where(np.arange(n) % 2, -1.0, 1.0)).astype(F32)
        x2 = ((0.5 + r.random((3, n))) * g[::-1] * 7.0).astype(F32)
        return dict(x1=x1, x2=x2, jobs=np.asarray(c['jobs'], JOB) if c['jobs'] else np.zeros(0, JOB))

    def frames(self, c, inp):
        return dict(out=Frame(F32, len(c['jobs']) * (4 * c['clip4'] + c['rem'])))

    def restate(self, c, inp, fr, fault=None):
        n = 4 * c['clip4']
        out = fr['out'].own().reshape(len(c['jobs']), n + c['rem'])
        for i, j in enumerate(inp['jobs']):
            s1, s2 = (i % 3, i % 3) if fault == 'src_is_row' else (j['src1'], j['src2'])
            l, m = F32(j['lam']), F32(F32(1) - F32(j['lam']))
            if fault == 'lam_swapped':
                l, m = m, l
            a, b = inp['x1'][s1], inp['x2'][s2]
            v = a if j['mode'] == 1 else b if j['mode'] == 2 else ((l * a).astype(F32) + (m * b).astype(F32)).astype(F32)
            end = n - 4 if fault == 'last_float4_dropped' else min(n, 4 * 256 * IC.mix_grid_x(c['clip4'])) if fault == 'second_trip_skipped' else n
            out[i, :end] = v[:end]

    def verify(self, c, inp, fr, img):
        guards(c, fr, img)
        got = fr['out'].own(img['out']).reshape(len(c['jobs']), 4 * c['clip4'] + c['rem'])
        w = 0.0
        for i, j in enumerate(inp['jobs']):
            a, b = inp['x1'][j['src1']], inp['x2'][j['src2']]
            if j['mode'] in (1, 2):
                exact(got[i], a if j['mode'] == 1 else b, f'{c["name"]} job {i} (copy)')
            else:
                l, m = float(F32(j['lam'])), float(F32(F32(1) - F32(j['lam'])))
                lp, mq = l * a.astype(np.float64), m * b.astype(np.float64)
                w = max(w, bounded(got[i], lp + mq, (2.0 ** -23 * (np.abs(lp) + np.abs(mq))) / C_SAFE, f'{c["name"]} job {i} (mix)'))
        return {'mixup.mode0': w}


# ================================================================================================ mixup_targets
S1 = (0.25, 0.25)                                  # the labelled event of the designed pairs: [0.125, 0.375], class 3
# design -> ((labels1, boxes1), (labels2, boxes2)); EXPECT: the decision written down by hand (0 mixed, 1 labelled clip, 2 pseudo clip)
DESIGN = {
    'touch': (([3], [S1]), ([3], [(0.5, 0.25)])),                                   # end 0.375 == onset 0.375: not separate
    'touch_reversed': (([3], [(0.5, 0.25)]), ([3], [S1])),
    'ulp_apart': (([3], [(0.25, float(F32(0.25) - F32(2.0 ** -24)))]), ([3], [(0.5, 0.25)])),      # end 0.375 - 2^-25: one f32 ulp below
    'other_class_overlap': (([3], [S1]), ([7], [(0.3125, 0.25)])),
    'overlap': (([3], [S1]), ([8, 3], [(0.75, 0.125), (0.3125, 0.25)])),
    'weak_first': (([7, 7], []), ([1, 2], [(0.5, 0.25), (0.5625, 0.25)])),          # boxes 0 and 1 read under the weak clip's labels 7, 7
    'weak_plain': (([2], []), ([6, 8], [(0.25, 0.125), (0.75, 0.125)])),
}
EXPECT = {'touch': 1, 'touch_reversed': 1, 'ulp_apart': 0, 'other_class_overlap': 0, 'overlap': 1, 'weak_first': 1, 'weak_plain': 0,
          'many': 0, 'many_clash_last': 1}


def _row_of_boxes(n, first=0):
    """n disjoint dyadic events of class 1"""
    return [1] * n, [((first + j + 0.5) / 256.0, 1.0 / 512.0) for j in range(n)]


def design_pair(d):
    if isinstance(d, str):
        return DESIGN[d]
    if d[0] == 'count':
        l1, b1 = _row_of_boxes(d[1])
        l2, b2 = _row_of_boxes(d[2], first=d[1])
        return (l1, b1), ([4] * len(l2), b2)
    l1, b1 = _row_of_boxes(2)
    l2, b2 = _row_of_boxes(d[1] - 2, first=2)
    if d[0] == 'many_clash_last':
        b2[-1] = (1.0 / 512.0, 1.0 / 512.0)            # overlaps event 0
    return (l1, b1), (l2, b2)


def expected_decision(c, i):
    if i >= c['mix_num']:
        return 2
    d = c['design'].get(i)
    if d is None:
        return 0
    if isinstance(d, str) or d[0] != 'count':
        return EXPECT[d if isinstance(d, str) else d[0]]
    return (1 if d[2] == 0 else 2) if d[1] + d[2] > c['max_events'] else 0


@register
class MixupTargets(Kernel):
    key = 'mixup_targets'
    faults = ('second_clip_skipped', 'box64_ignored', 'max_events_ge', 'touch_separate', 'split_ignored', 'offsets_kept_when_full',
              'box_label_from_own_list')

    def ns_eff(self, c):
        return c['ns1'] if c['split'] is None else min(c['split'], c['ns1'])

    def targets(self, c):
        """(y1 as the tables hold it, y1 as the reference reads it, y2): lists of (labels, boxes, ratio or None)"""
        y1t, y1r, y2 = [], [], []
        for i in range(c['B1']):
            n = 1 + i % 3
            lab, box = [(i + k) % 5 for k in range(n)], [((2 * k + 1) / 16.0, 1.0 / 32.0) for k in range(n)]
            if i in c['design'] and i < c['B2']:
                lab, box = design_pair(c['design'][i])[0]
            ratio = [float(F32(0.25 + 0.05 * i))] * len(lab) if c['ratio1'] and i % 3 == 0 else None
            y1t.append((lab, box if i < c['ns1'] else [], ratio))
            y1r.append((lab, box if i < self.ns_eff(c) else [], ratio))
        for i in range(c['B2']):
            n = i % 4
            lab, box = [5 + (i + k) % 5 for k in range(n)], [(0.5 + (2 * k + 1) / 16.0, 1.0 / 32.0) for k in range(n)]
            if i in c['design'] and i < c['B1']:
                lab, box = design_pair(c['design'][i])[1]
            y2.append((lab, box, None))
        return y1t, y1r, y2

    @staticmethod
    def _table(y, nbox_clips):
        lab = np.asarray([l for t in y for l in t[0]] + [0], np.int64)
        lab_off = np.cumsum([0] + [len(t[0]) for t in y]).astype(np.int32)
        box = np.asarray([v for t in y[:nbox_clips] for b in t[1] for v in b] + [0, 0], F32)
        box_off = np.cumsum([0] + [len(t[1]) for t in y[:nbox_clips]]).astype(np.int32)
        ratio = np.asarray([r for t in y for r in (t[2] or [1.0] * len(t[0]))] + [1.0], F32)
        return lab, lab_off, box, box_off, ratio

    def make(self, c):
        y1t, y1r, y2 = self.targets(c)
        t1, t2 = self._table(y1t, c['ns1']), self._table(y2, c['B2'])
        from sound_event_detection_transformer_amd.utilities.mixup import lam_pair
        inp = dict(lab1=t1[0], lab_off1=t1[1], box1=t1[2], box_off1=t1[3], ratio1=t1[4] if c['ratio1'] else None,
                   split1=None if c['split'] is None else np.asarray([c['split']], np.int32),
                   lab2=t2[0], lab_off2=t2[1], box2=t2[2], box_off2=t2[3], lam=lam_pair(LAM), y1r=y1r, y2=y2)
        exp = self.expected(c, inp)
        tot = max(exp['lab_off'][-1], exp['box_off'][-1])
        inp['cap'] = c['B2'] * c['max_targets'] if c['cap'] is None else int(tot) + c['cap']
        inp['bufcap'] = max(inp['cap'], int(tot), 1)
        return inp

    def frames(self, c, inp):
        n, B2 = inp['bufcap'], c['B2']
        fr = dict(lab_out=Frame(np.int64, n), lab_off_out=Frame(np.int32, B2 + 1), box_out=Frame(F32, 2 * n), box_off_out=Frame(np.int32, B2 + 1),
                  jobs=Frame(np.int32, 4 * B2))
        if c['ratio_out']:
            fr['ratio_out'] = Frame(F32, n)
        return fr

    def plan(self, c, inp):
        """utilities.mixup.plan_mixup_label_unlabel on the reference's reading of the targets -> (modes, merged targets)"""
        from sound_event_detection_transformer_amd.utilities.mixup import plan_mixup_label_unlabel

        def tg(y):
            out = []
            for lab, box, ratio in y:
                t = dict(labels=torch.tensor(lab, dtype=torch.int64), boxes=torch.tensor(box, dtype=torch.float32).reshape(-1, 2), orig_size=0)
                if ratio is not None:
                    t['ratio'] = torch.tensor(ratio, dtype=torch.float32)
                out.append(t)
            return out
        ratio = c['mix_num'] / c['B1'] if c['B1'] else 0.0
        assert int(c['B1'] * ratio) == c['mix_num']
        jobs, labels = plan_mixup_label_unlabel(tg(inp['y1r']), tg(inp['y2']), LAM, c['B1'], ratio, c['max_events'])
        return [j[2] for j in jobs], labels

    def expected(self, c, inp):
        def build():
            modes, labels = self.plan(c, inp)
            lab = [t['labels'].numpy() for t in labels]
            box = [t['boxes'].reshape(-1, 2).numpy().astype(F32) for t in labels]
            rat = [t['ratio'].float().numpy() if 'ratio' in t else np.ones(len(t['labels']), F32) for t in labels]
            return dict(modes=modes, lab=lab, box=box, ratio=rat, lab_off=np.cumsum([0] + [len(x) for x in lab]).astype(np.int32),
                        box_off=np.cumsum([0] + [len(x) for x in box]).astype(np.int32))
        return cached(self.key, c, build)

    def restate(self, c, inp, fr, fault=None):
        """mixup_targets_kernel step by step (its lanes and waves matter only through the injected faults)"""
        B2, ns1 = c['B2'], c['ns1'] if fault == 'split_ignored' else self.ns_eff(c)
        a = inp
        dec, lo, bo = np.zeros(B2, np.int32), np.zeros(B2 + 1, np.int32), np.zeros(B2 + 1, np.int32)
        half = F32(2)
        for i in range(B2):
            l2o, nl2 = a['lab_off2'][i], a['lab_off2'][i + 1] - a['lab_off2'][i]
            b2o, nb2 = a['box_off2'][i], a['box_off2'][i + 1] - a['box_off2'][i]
            d, nl, nb = 2, nl2, nb2
            if fault == 'second_clip_skipped' and i >= 16:
                pass
            elif i < c['mix_num'] and i < c['B1']:
                l1o, nl1 = a['lab_off1'][i], a['lab_off1'][i + 1] - a['lab_off1'][i]
                b1o, nb1 = (a['box_off1'][i], a['box_off1'][i + 1] - a['box_off1'][i]) if i < ns1 else (0, 0)
                over = nb1 + nb2 >= c['max_events'] if fault == 'max_events_ge' else nb1 + nb2 > c['max_events']
                if over:
                    if nb2 == 0:
                        d, nl, nb = 1, nl1, nb1
                else:
                    n = nb1 + nb2
                    bx = np.concatenate([a['box1'][2 * b1o:2 * (b1o + nb1)], a['box2'][2 * b2o:2 * (b2o + nb2)]]).reshape(-1, 2)
                    lab = np.concatenate([a['lab1'][l1o:l1o + nl1], a['lab2'][l2o:l2o + nl2]])
                    if fault == 'box_label_from_own_list':
                        lab = np.concatenate([a['lab1'][l1o:l1o + nb1], a['lab2'][l2o:l2o + nl2]])
                    s, t = (bx[:, 0] - bx[:, 1] / half).astype(F32), (bx[:, 0] + bx[:, 1] / half).astype(F32)
                    clash = False
                    for j in range(min(n, 64) if fault == 'box64_ignored' else n):
                        for k in range(j):
                            if lab[k] != lab[j]:
                                continue
                            if fault == 'touch_separate':
                                clash |= bool(not (t[j] <= s[k]) and not (t[k] <= s[j]))
                            else:
                                clash |= bool(not (t[j] < s[k]) and not (t[k] < s[j]))
                    d, nl, nb = (1, nl1, nb1) if clash else (0, nl1 + nl2, n)
            dec[i], lo[i + 1], bo[i + 1] = d, nl, nb
        lo, bo = np.cumsum(lo).astype(np.int32), np.cumsum(bo).astype(np.int32)
        fits = lo[B2] <= a['cap'] and bo[B2] <= a['cap']
        keep = fits or fault == 'offsets_kept_when_full'
        fr['lab_off_out'].own()[:] = lo if keep else 0
        fr['box_off_out'].own()[:] = bo if keep else 0
        jobs = fr['jobs'].own().reshape(B2, 4)
        for i in range(B2):
            d = dec[i]
            jobs[i, :3] = (i, i, d)
            jobs[i, 3:].view(F32)[0] = a['lam'][0] if d == 0 else 0.0
            if not fits:
                continue
            l2o, nl2 = a['lab_off2'][i], a['lab_off2'][i + 1] - a['lab_off2'][i]
            b2o, nb2 = a['box_off2'][i], a['box_off2'][i + 1] - a['box_off2'][i]
            l1o = nl1 = b1o = nb1 = 0
            if d != 2:
                l1o, nl1 = a['lab_off1'][i], a['lab_off1'][i + 1] - a['lab_off1'][i]
                if i < ns1:
                    b1o, nb1 = a['box_off1'][i], a['box_off1'][i + 1] - a['box_off1'][i]
            k1, k2 = (0 if d == 2 else nl1), (0 if d == 1 else nl2)
            fr['lab_out'].own()[lo[i]:lo[i] + k1 + k2] = np.concatenate([a['lab1'][l1o:l1o + k1], a['lab2'][l2o:l2o + k2]])
            if 'ratio_out' in fr:
                r1 = a['ratio1'][l1o:l1o + k1] if a['ratio1'] is not None else np.ones(k1, F32)
                fr['ratio_out'].own()[lo[i]:lo[i] + k1 + k2] = [a['lam'][0]] * k1 + [a['lam'][1]] * k2 if d == 0 else (r1 if d == 1 else np.ones(k2, F32))
            t1, t2 = (0 if d == 2 else nb1), (0 if d == 1 else nb2)
            fr['box_out'].own()[2 * bo[i]:2 * (bo[i] + t1 + t2)] = np.concatenate([a['box1'][2 * b1o:2 * (b1o + t1)], a['box2'][2 * b2o:2 * (b2o + t2)]])

    def want(self, c, inp, fr):
        """the expected images of every output, fill included"""
        e = self.expected(c, inp)
        B2 = c['B2']
        w = {n: f.blank() for n, f in fr.items()}
        fits = e['lab_off'][-1] <= inp['cap'] and e['box_off'][-1] <= inp['cap']
        fr['lab_off_out'].own(w['lab_off_out'])[:] = e['lab_off'] if fits else 0
        fr['box_off_out'].own(w['box_off_out'])[:] = e['box_off'] if fits else 0
        jobs = fr['jobs'].own(w['jobs']).reshape(B2, 4)
        for i in range(B2):
            jobs[i, :3] = (i, i, e['modes'][i])
            jobs[i, 3:].view(F32)[0] = inp['lam'][0] if e['modes'][i] == 0 else 0.0
        if fits:
            fr['lab_out'].own(w['lab_out'])[:e['lab_off'][-1]] = np.concatenate(e['lab'] + [np.zeros(0, np.int64)])
            fr['box_out'].own(w['box_out'])[:2 * e['box_off'][-1]] = np.concatenate([b.reshape(-1) for b in e['box']] + [np.zeros(0, F32)])
            if 'ratio_out' in fr:
                fr['ratio_out'].own(w['ratio_out'])[:e['lab_off'][-1]] = np.concatenate(e['ratio'] + [np.zeros(0, F32)])
        return w

    def verify(self, c, inp, fr, img):
        want = self.want(c, inp, fr)
        for n in fr:
            exact(img[n], want[n], f'{c["name"]}.{n}')
        return {}


# ================================================================================================ query_patches
def resample_rows(code, out_h=128, copy_branch=True):
    """Pillow's vertical bilinear pass (transforms_oracle.pil_resize_rows) with the same-size copy made optional"""
    code = np.asarray(code, np.uint8)
    h = code.shape[0]
    if h == out_h and copy_branch:
        return code.copy()
    scale = h / out_h
    fs = max(scale, 1.0)
    out = np.empty((out_h, code.shape[1]), np.uint8)
    for yy in range(out_h):
        center = (yy + 0.5) * scale
        ymin = max(int(center - fs + 0.5), 0)
        n = min(int(center + fs + 0.5), h) - ymin
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(n) + ymin - center + 0.5) * (1.0 / fs)))
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = w / ww
        kk = (0.5 + w * 4194304.0).astype(np.int64)
        acc = (1 << 21) + (code[ymin:ymin + n].astype(np.int64) * kk[:, None]).sum(0)
        out[yy] = np.clip(acc >> 22, 0, 255)
    return out


def patch_from_rows(data, s, e, fixed, resize=TO.pil_resize_rows):
    """the body of transforms_oracle.query_patches for the rows [s, e) of one clip data [T, F] f32"""
    patch = data[s:e]
    if fixed:
        return patch.astype(F32)
    mn, mx = patch.min(), patch.max()
    code = (((patch - mn) / (mx - mn)) * F32(255)).astype(np.uint8)
    back = resize(code, 128).astype(F32) / F32(255)
    return (back * (mx - mn) + mn).astype(F32)


def box_of_rows(s, e, T):
    """a (centre, length) box that transforms_oracle.patch_rows maps back to [s, e), or None"""
    box = np.asarray([(s + e) / (2.0 * T), (e - s) / float(T)], F32)
    return box if TO.patch_rows(box, T) == (s, e) else None


@register
class QueryPatches(Kernel):
    key = 'query_patches'
    faults = ('copy_branch_from_128', 'crop_from_row0', 'clip_ignored')

    def make(self, c):
        r = rng_of(c)
        data = (r.standard_normal((c['B'], c['T'], c['F'])) * 2.0 + 0.5) * (10.0 ** (np.arange(c['B']) - 1.0))[:, None, None]
        jobs = np.zeros((len(c['jobs']), 4), np.int32)
        if c['jobs']:
            jobs[:, :3] = c['jobs']
        return dict(data=data.astype(F32), jobs=jobs)

    def frames(self, c, inp):
        return dict(out=Frame(F32, len(c['jobs']) * 128 * c['F']))

    def restate(self, c, inp, fr, fault=None):
        out = fr['out'].own().reshape(len(c['jobs']), 128, c['F'])
        for i, (b, s, e, _) in enumerate(inp['jobs']):
            h = e - s
            if fault == 'crop_from_row0':
                s, e = 0, h
            d = inp['data'][0 if fault == 'clip_ignored' else b]
            if fault == 'copy_branch_from_128' and h >= 128 and not c['fixed']:
                out[i] = patch_from_rows(d, s, e, 0, lambda code, n: code[:128].copy())
            else:
                out[i] = patch_from_rows(d, s, e, c['fixed'], resample_rows)

    def reference(self, c, inp):
        return cached(self.key, c, lambda: [patch_from_rows(inp['data'][b], s, e, c['fixed']) for b, s, e, _ in inp['jobs']])

    def verify(self, c, inp, fr, img):
        guards(c, fr, img)
        got = fr['out'].own(img['out']).reshape(len(c['jobs']), 128, c['F'])
        for i, ref in enumerate(self.reference(c, inp)):
            exact(got[i], ref, f'{c["name"]} patch {i} rows {tuple(int(k) for k in inp["jobs"][i, 1:3])}')
        return {}


# (kernel key, fault): each must fail at least one row of its kernel (tests/test_input_check_cpu.py)
FAULTS = [(k, f) for k in KERNELS for f in KERNELS[k].faults]
