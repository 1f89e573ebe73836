"""GPU: the glue, pooling and skinny-head kernels (csrc/misc.hip: add, add_n, cast, relu_mask, sigmoid_grad, dropout_grad, gelu_fwd /
gelu_bwd, copy2d, spsedt_dec_in forward / backward, colsum, avgpool (both kernels), maxpool_fwd / maxpool_bwd, mask_resize, posenc,
stem_im2col; csrc/split3.hip; csrc/skinny.hip: forward, input gradient, weight gradient) at their vector, block, chunk, job-table
and LDS edges, element by element (tests/glue_check.py: references, bounds, guard frames, restatements; tests/glue_cases.py: the rows).

The C entry points are called through lib.load() with pointers into guard frames (glue_check.Frame): every output sits in one filled
buffer, 32 guard elements on either side and the gap columns of a strided output inside.  Per row: gemm_check.poison() before each
launch; no byte outside the owned elements changes; every owned float is finite; exact kernels equal their np.float32 restatement bit
for bit (and float64 under the bound), bounded kernels stay under c (sqrt(K) 2^-24 sum|terms| + u_out |ref|) plus the transcendental
terms of glue_check.K_FN; a second launch from the same inputs is bit-identical.  The rows through ops.* (nine sources of add_n, nine
copy2d jobs, the deferred skinny weight gradient) count their launches with lib.launch_log.  posenc is also compared with
oracle.sedt_oracle.PositionEmbeddingSine at the tolerance of tests/test_ops_gpu.py.  Then the refused calls: non-zero status,
sedt_last_error names the entry point, no byte of the frame changes.  No row is sampled or skipped.

The four entry-point fixes and the rows that show them: skinny forward above 64 KB of LDS (skinny_fwd_*_N16_K512_*, *_K1024_*: the
launch needs the raised dynamic-LDS limit), skinny forward K % 4 (test_refusals: K = 66), empty tensors (the n0 / B0 / rows 0 rows: the
call returns 0 and the frame is untouched), spsedt_dec_in's f32 alignment (test_refusals: patch 16 bytes behind a 32-byte boundary).

The largest error / bound ratio per kernel and output, and the k_fn measurements (glue_check.k_measure), are printed at the end of the
module with -s, with the module's run time.  On MI355X (1.9 s inside the whole suite, 4.5 s alone; [dtype] = the rows' compute dtype, a
bf16 output's ratio is mostly its own rounding: 0.5 of c u_out):
  add [bf16]                 0.498     add [f32]                  0.499     add_n [bf16]               0.586
  add_n [f32]                0.563     avgpool [bf16]             0.167     avgpool [f32]              0.653
  colsum [bf16]              0.0741    colsum [f32]               0.433     dec_in [bf16]              0.497
  dec_in [f32]               0.5       dec_in_bwd d_patch [bf16]  0.498     dec_in_bwd d_patch [f32]   0.353
  dec_in_bwd d_query [bf16]  0         dec_in_bwd d_query [f32]   0.545     gelu_bwd [bf16]            0.489
  gelu_bwd [f32]             0.541     gelu_fwd [bf16]            0.49      gelu_fwd [f32]             0.355
  posenc [bf16]              0.492     posenc [f32]               0.0553    sigmoid_grad [f32]         0.381
  skinny_dgrad [bf16]        0.496     skinny_dgrad [f32]         0.526     skinny_fwd none [bf16]     0.497
  skinny_fwd none [f32]      0.134     skinny_fwd relu [bf16]     0.498     skinny_fwd relu [f32]      0.129
  skinny_fwd sigmoid [bf16]  0.455     skinny_fwd sigmoid [f32]   0.0699    skinny_wgrad dW [bf16]     0.506
  skinny_wgrad dW [f32]      0.713     skinny_wgrad db [bf16]     0.276     skinny_wgrad db [f32]      0.496
  split3 hi+lo [f32]         0.499
  k:erf+exp(gelu_fwd) 6.1, k:erf+exp(gelu_bwd) 8.8, k:nexp(skinny sigmoid) 4.5, k:sin+pow(posenc) 1.04
The exact kernels' ratios are those of their restatements by construction; the bounded f32 rows (skinny, gelu) land on the figures of
tests/test_glue_check_cpu.py's restatements to three digits, posenc's functions differ from numpy's (1.04 against 1.28).  No kernel
failed a row; the four entry-point changes came from reading the code, before the rows were run.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import glue_cases as GC
import glue_check as K
from gemm_check import nan_buffer, poison

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)
T0 = [None]
DT = dict(f32=0, bf16=1)
TDT = dict(f32=torch.float32, bf16=torch.bfloat16)


@pytest.fixture(scope='module')
def env():
    from sound_event_detection_transformer_amd import lib as L, ops
    assert torch.cuda.is_available()
    lib = L.load()
    T0[0] = time.time()
    yield L, lib, ops
    if RATIOS:
        print('\nlargest error / bound ratio per kernel and output (k: the k_fn measurements, in units of 2^-24 s):')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - T0[0]:.1f} s')


def vp(a):
    return None if a is None else C.c_void_p(int(a))


def up(a, lead=0):
    """a numpy array as device bytes, `lead` bytes behind a 256-byte boundary; returns (tensor, address of the first element)"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.empty(lead + b.size + 64, dtype=torch.uint8, device='cuda')
    assert t.data_ptr() % 256 == 0
    t[lead:lead + b.size] = torch.from_numpy(b.copy())
    return t, t.data_ptr() + lead


def as_tensor(t, addr, shape, dt):
    """a typed view of the device bytes t from address addr on"""
    o = addr - t.data_ptr()
    n = int(np.prod(shape)) * TDT[dt].itemsize
    return t[o:o + n].view(TDT[dt]).view(*shape)


class Row(object):
    """a row's inputs and frames on the device"""

    def __init__(self, key, c):
        self.key, self.c, self.k = key, c, K.KERNELS[key]
        self.inp = self.k.make(c)
        self.fr = self.k.frames(c, self.inp)
        self.keep = []
        self.P_in, self.T_in = {}, {}                       # the inputs: addresses and the tensors that own them
        for n, a in self.inp.items():
            lead = c.get('off', 0) if (key, n) == ('avgpool', 'x') else 0
            self.T_in[n], self.P_in[n] = up(a, lead)
        self.P, self.T = dict(self.P_in), dict(self.T_in)

    def fresh_frames(self):
        """P / T: the inputs, and over them (a frame may carry an input's name) fresh copies of the frame images"""
        self.P, self.T = dict(self.P_in), dict(self.T_in)
        for n, f in self.fr.items():
            t, p = up(f.buf)
            self.T[n], self.P[n] = t, p + f.off * f.buf.itemsize
            assert self.P[n] % 32 == 0

    def images(self):
        torch.cuda.synchronize()
        out = {}
        for n, f in self.fr.items():
            b = self.T[n].cpu().numpy()
            out[n] = b[:f.buf.nbytes].view(f.buf.dtype).copy()
        return out

    def frame_tensor(self, n):
        f = self.fr[n]
        assert f.ld == f.cols
        return as_tensor(self.T[n], self.P[n], (f.rows, f.cols), f.dt)


# ================================================================================================ launchers
def l_add(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_add(vp(P['a']), vp(P['b']), vp(P['out']), c['rows'], c['cols'], c['b_mod'], DT[c['dt']], L.stream_ptr()), 'add')


def l_cast(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_cast(vp(P['x']), DT[c['src']], vp(P['out']), DT[c['dst']], c['n'], L.stream_ptr()), 'cast')


def l_relu_mask(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_relu_mask(vp(P['g']), vp(P['y']), vp(P['out']), c['n'], DT[c['dt']], L.stream_ptr()), 'relu_mask')


def l_sigmoid_grad(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_sigmoid_grad(vp(P['g']), vp(P['s']), vp(P['out']), c['n'], L.stream_ptr()), 'sigmoid_grad')


def l_add_n(L, lib, ops, r):
    c, P = r.c, r.P
    isz = 2 if c['dt'] == 'bf16' else 4
    if c['via'] == 'ops':
        srcs = [as_tensor(r.T['src'], P['src'] + j * c['n'] * isz, (c['n'],), c['dt']) for j in range(c['k'])]
        with L.launch_log() as log:
            ops.add_n(DT[c['dt']], srcs, out=r.frame_tensor('out')[0])
        assert log['add_n'] == 2, log
        return
    arr = (C.c_void_p * c['k'])(*[P['src'] + j * c['n'] * isz for j in range(c['k'])])
    with L.launch_log() as log:
        L.check(lib.sedt_add_n(arr, c['k'], vp(P['out']), c['n'], DT[c['dt']], L.stream_ptr()), 'add_n')
    assert log['add_n'] == 1


def _seed_args(r, mode):
    v, p = K.seed_parts(mode)
    if p is None:
        return v, None
    t = torch.from_numpy(np.array([p], np.uint32).view(np.int32)).cuda()
    r.keep.append(t)
    return v, t.data_ptr()


def l_dropout_grad(L, lib, ops, r):
    c, P = r.c, r.P
    v, p = _seed_args(r, c['seed'])
    L.check(lib.sedt_dropout_grad(vp(P['x']), c['cols'] + K.DropoutGrad.LDI, vp(P['out']), c['cols'] + K.DropoutGrad.LDO, c['rows'], c['cols'],
                                  float(c['p']), v, vp(p), DT[c['dt']], L.stream_ptr()), 'dropout_grad')


def l_gelu(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_gelu_fwd(vp(P['h']), vp(P['a']), c['n'], float(c['p']), K.SEED, None, DT[c['dt']], L.stream_ptr()), 'gelu_fwd')
    L.check(lib.sedt_gelu_bwd(vp(P['g']), vp(P['h']), vp(P['gh']), c['n'], float(c['p']), K.SEED, None, DT[c['dt']], L.stream_ptr()), 'gelu_bwd')


def l_copy2d(L, lib, ops, r):
    c, P = r.c, r.P
    jobs = [(P[f'src{j}'], P[f'dst{j}'], outer, inner, inner + K.Copy2d.SGAP, inner + K.Copy2d.DGAP) for j, (outer, inner) in enumerate(c['jobs'])]
    with L.launch_log() as log:
        if c['via'] == 'ops':
            ops.copy2d(jobs)
        else:
            arr = (L.SedtCopyJob * len(jobs))()
            for n, (sp, dp, outer, inner, ss, ds) in enumerate(jobs):
                arr[n].src, arr[n].dst, arr[n].outer, arr[n].inner, arr[n].src_stride, arr[n].dst_stride = sp, dp, outer, inner, ss, ds
            L.check(lib.sedt_copy2d(arr, len(jobs), L.stream_ptr()), 'copy2d')
    assert log['copy2d'] == (2 if c['via'] == 'ops' else 1)


def l_split3(L, lib, ops, r):
    c, P = r.c, r.P
    arr = (L.SedtSplitJob * len(c['jobs']))()
    for j, (rows, cols, pad, pat) in enumerate(c['jobs']):
        arr[j].src, arr[j].ld, arr[j].dst, arr[j].rows, arr[j].cols, arr[j].pattern = P[f'src{j}'], cols + pad, P[f'dst{j}'], rows, cols, pat
    L.check(lib.sedt_split3(arr, len(c['jobs']), L.stream_ptr()), 'split3')


def l_dec_in(L, lib, ops, r):
    c, P = r.c, r.P
    train = c['mode'] != 'eval'
    L.check(lib.sedt_spsedt_dec_in(vp(P['patch']), vp(P['query']), vp(P['keep']) if c['mode'] == 'given' else None, vp(P.get('keep_out')), vp(P['out']),
                                   c['B'], c['Q'], c['P'], c['qpp'], c['D'], int(train), float(c['ratio']), K.SEED, None, DT[c['dt']],
                                   L.stream_ptr()), 'spsedt_dec_in')


def l_dec_in_bwd(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_spsedt_dec_in_bwd(vp(P['g']), vp(P['keep']), vp(P.get('d_patch')), vp(P['d_query']), c['B'], c['Q'], c['P'], c['qpp'], c['D'], 1,
                                       DT[c['dt']], L.stream_ptr()), 'spsedt_dec_in_bwd')


def l_colsum(L, lib, ops, r):
    c, P = r.c, r.P
    nb = lib.sedt_colsum_scratch(c['rows'], c['cols'])
    scratch = nan_buffer(nb // 4 + 64, torch.float32)
    r.keep.append(scratch)
    L.check(lib.sedt_colsum(vp(P['x']), c['cols'] + c['view'], c['rows'], c['cols'], c['in_f32'], DT[c['dt']], vp(P['out']), vp(scratch.data_ptr()), nb,
                            L.stream_ptr()), 'colsum')


def l_avgpool(L, lib, ops, r):
    c, P = r.c, r.P
    assert P['x'] % 32 == c['off']
    L.check(lib.sedt_avgpool(vp(P['x']), vp(P['out']), c['B'], c['P'], c['C'], DT[c['dt']], L.stream_ptr()), 'avgpool')


def l_maxpool(L, lib, ops, r):
    c, P = r.c, r.P
    a = (c['B'], c['H'], c['W'], c['C'], DT[c['dt']], L.stream_ptr())
    L.check(lib.sedt_maxpool_fwd(vp(P['x']), vp(P['y']), vp(P['idx']), *a), 'maxpool_fwd')
    # (the backward launches read the reference forward results, uploaded with the inputs)
    L.check(lib.sedt_maxpool_bwd(vp(P['dy']), vp(r.P_in['idx']), vp(P['relu_src']), vp(P['dx_relu']), *a), 'maxpool_bwd')
    L.check(lib.sedt_maxpool_bwd_y(vp(P['dy']), vp(r.P_in['idx']), None, vp(r.P_in['y']), vp(P['dx_y']), *a), 'maxpool_bwd')
    L.check(lib.sedt_maxpool_bwd(vp(P['dy']), vp(r.P_in['idx']), None, vp(P['dx_plain']), *a), 'maxpool_bwd')


def l_mask_resize(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_mask_resize(vp(P['m']), vp(P['out']), c['B'], c['Hin'], c['Win'], c['Hout'], c['Wout'], L.stream_ptr()), 'mask_resize')


def l_posenc(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_posenc(vp(P['m']), vp(P['pos']), c['B'], c['H'], c['W'], c['D'], DT[c['dt']], L.stream_ptr()), 'posenc')


def l_stem_im2col(L, lib, ops, r):
    c, P = r.c, r.P
    L.check(lib.sedt_stem_im2col(vp(P['x']), vp(P['col']), c['B'], c['H'], c['W'], DT[c['dt']], L.stream_ptr()), 'stem_im2col')


def l_skinny_fwd(L, lib, ops, r):
    c, P = r.c, r.P
    M, N, Kk = c['M'], c['N'], c['K']
    a = (M, N, Kk, K.ACT[c['act']], c['out_f32'], DT[c['dt']], L.stream_ptr())
    bias = vp(P['b']) if c['bias'] else None
    assert P['x'] % 32 == 0
    L.check(lib.sedt_skinny_linear_fwd(vp(P['x']), Kk, vp(P['w']), bias, vp(P['y']), N, *a), 'skinny_linear_fwd')
    # the same rows as a column view: 8 elements into a buffer whose rows are K + 12 apart -> the scalar loader
    k = K.KERNELS['skinny_fwd']
    wide = np.zeros((M, Kk + k.XPAD), r.inp['x'].dtype)
    wide[:, k.XOFF:k.XOFF + Kk] = r.inp['x']
    t, p = up(wide)
    r.keep.append(t)
    assert (Kk + k.XPAD) % 8 != 0
    L.check(lib.sedt_skinny_linear_fwd(vp(p + k.XOFF * wide.itemsize), Kk + k.XPAD, vp(P['w']), bias, vp(P['y_view']), N, *a), 'skinny_linear_fwd')


def l_skinny_dgrad(L, lib, ops, r):
    c, P = r.c, r.P
    M, N, Kk = c['M'], c['N'], c['K']
    ldo = Kk + K.SkinnyDgrad.ACC_PAD if c['acc'] else Kk
    L.check(lib.sedt_skinny_linear_bwd(vp(P['g']), vp(P['ys']), N, vp(P['w']), vp(P['w']), Kk, vp(P['mask']) if c['mask'] else None, Kk,
                                       vp(P['gx']), ldo, None, None, None, M, N, Kk, K.ACT[c['act']], c['acc'], DT[c['dt']], L.stream_ptr()),
            'skinny_linear_bwd')


def l_skinny_wgrad(L, lib, ops, r):
    c, P = r.c, r.P
    M, N, Kk = c['M'], c['N'], c['K']
    if c['deferred']:
        g, ys = (as_tensor(r.T[n], P[n], (M, N), 'f32') for n in ('g', 'ys'))
        x = as_tensor(r.T['x'], P['x'], (M, Kk), c['dt'])
        w = torch.zeros(N, Kk, device='cuda')
        batch = ops.ReduceBatch()
        with L.launch_log() as log:
            _, dw, db = ops.skinny_linear_bwd(DT[c['dt']], g, ys, w, x, act=K.ACT[c['act']], need_gx=False, batch=batch)
            batch.flush()
        assert log['skinny_linear_bwd'] == 1, log
        r.frame_tensor('dw').copy_(dw)
        r.frame_tensor('db')[0].copy_(db)
        return
    nb = lib.sedt_skinny_linear_bwd_scratch(Kk)
    scratch = nan_buffer(nb // 4 + 64, torch.float32)
    r.keep.append(scratch)
    L.check(lib.sedt_skinny_linear_bwd(vp(P['g']), vp(P['ys']), N, vp(P['g']), vp(P['x']), Kk, None, 0, None, Kk, vp(P['dw']), vp(P.get('db')),
                                       vp(scratch.data_ptr()), M, N, Kk, K.ACT[c['act']], 0, DT[c['dt']], L.stream_ptr()), 'skinny_linear_bwd')


LAUNCH = dict(add=l_add, cast=l_cast, relu_mask=l_relu_mask, sigmoid_grad=l_sigmoid_grad, add_n=l_add_n, dropout_grad=l_dropout_grad, gelu=l_gelu,
              copy2d=l_copy2d, split3=l_split3, dec_in=l_dec_in, dec_in_bwd=l_dec_in_bwd, colsum=l_colsum, avgpool=l_avgpool, maxpool=l_maxpool,
              mask_resize=l_mask_resize, posenc=l_posenc, stem_im2col=l_stem_im2col, skinny_fwd=l_skinny_fwd, skinny_dgrad=l_skinny_dgrad,
              skinny_wgrad=l_skinny_wgrad)


def run_row(env, key, c):
    L, lib, ops = env
    r = Row(key, c)
    imgs = []
    for rep in range(2):
        r.fresh_frames()
        poison(16)
        LAUNCH[key](L, lib, ops, r)
        imgs.append(r.images())
        r.keep = []
    for k, v in K.verify_row(key, c, r.inp, r.fr, imgs[0]).items():
        RATIOS[K.ratio_key(k, c)] = max(RATIOS[K.ratio_key(k, c)], v)
    for n in r.fr:
        assert np.array_equal(K.bits(imgs[0][n]), K.bits(imgs[1][n])), f'{c["name"]}.{n}: a second launch differs'
    return r, imgs[0]


@pytest.mark.parametrize('key', [k for k in GC.CASES if k not in ('posenc', 'avgpool')])
def test_glue_envelope(env, key):
    assert set(LAUNCH) == set(GC.CASES)
    for c in GC.CASES[key]:
        run_row(env, key, c)


def test_avgpool_envelope_and_the_two_kernels_agree(env):
    """every avgpool row; the rows at a 16-byte offset (scalar kernel, by the entry point's alignment test) give the bits of the same
    data at a 32-byte boundary (eight-channel kernel), as the source comment says"""
    got = {}
    for c in GC.AVGPOOL:
        r, img = run_row(env, 'avgpool', c)
        got[(c['P'], c['C'], c['dt'], c['off'])] = (r.inp['x'], r.fr['out'].owned(img['out']))
    pairs = 0
    for (P, Cc, dt, off), (x, out) in got.items():
        if off:
            # the same values through the other kernel: inputs are seeded by the row's name, so compare through the restatement, which
            # both kernels equal bit for bit (verify_row: exact), and directly on one shared input
            c16 = next(c for c in GC.AVGPOOL if (c['P'], c['C'], c['dt'], c['off']) == (P, Cc, dt, off))
            c0 = dict(c16, off=0)                            # same name -> same inputs, at the aligned address
            assert GC.avgpool_kernel(c0) == 'vec8' and GC.avgpool_kernel(c16) == 'scalar'
            r0, img0 = run_row(env, 'avgpool', c0)
            assert np.array_equal(K.bits(r0.inp['x']), K.bits(x))
            assert np.array_equal(K.bits(r0.fr['out'].owned(img0['out'])), K.bits(out)), f'{c16["name"]}: the two avgpool kernels differ in bits'
            pairs += 1
    assert pairs == 4


def test_posenc_envelope_and_oracle(env):
    from oracle import sedt_oracle as O
    for c in GC.POSENC:
        r, img = run_row(env, 'posenc', c)
        B, H, W, D = c['B'], c['H'], c['W'], c['D']
        m = torch.from_numpy(r.inp['m']).bool()
        pe = O.PositionEmbeddingSine(D, normalize=True)(O.NestedTensor(torch.zeros(B, 1, H, W), m))           # (B, D, H, W)
        ref = pe.flatten(2).permute(0, 2, 1).reshape(-1, D).double().numpy()
        got = K.val(c['dt'], r.fr['pos'].owned(img['pos'])).astype(np.float64)
        tol = 2e-5 if c['dt'] == 'f32' else 5e-3             # tests/test_ops_gpu.py: relative to the largest element
        assert np.abs(got - ref).max() <= tol * max(np.abs(ref).max(), 1e-12), c['name']


# ================================================================================================ refused calls
def _refused(L, lib, status, name, frames):
    assert status != 0, f'{name}: accepted'
    assert name in lib.sedt_last_error().decode(), lib.sedt_last_error().decode()
    torch.cuda.synchronize()
    for t, before in frames:
        assert torch.equal(t.cpu(), before), f'{name}: a refused call changed the frame'


def _frame(dt, rows, cols):
    f = K.Frame(dt, rows, cols)
    t, p = up(f.buf)
    return t, p + f.off * f.buf.itemsize, t.cpu().clone()


def test_refusals(env):
    """each one returns from a SEDT_REQUIRE before any launch (read in csrc/): non-zero status, the error names the entry point, no
    byte of the frame changes"""
    L, lib, ops = env
    S = L.stream_ptr()
    src_t, src = up(np.ones(1 << 16, np.float32))
    # skinny weight gradient at M = 16385: the row slice does not fit the LDS buffer
    t, p, b = _frame('f32', 16, 64)
    scratch = nan_buffer(lib.sedt_skinny_linear_bwd_scratch(64) // 4, torch.float32)
    big_t, big = up(np.ones((16385, 64), np.float32))
    st = lib.sedt_skinny_linear_bwd(vp(big), None, 16, vp(src), vp(big), 64, None, 0, None, 64, vp(p), None, vp(scratch.data_ptr()), 16385, 16, 64, 0, 0,
                                    0, S)
    _refused(L, lib, st, 'skinny_linear_bwd', [(t, b)])
    assert torch.isnan(scratch).all()
    # skinny forward: K % 4 != 0 (the LDS rows are read as float4) - refused since this module's fix
    t, p, b = _frame('f32', 4, 2)
    _refused(L, lib, lib.sedt_skinny_linear_fwd(vp(src), 66, vp(src), None, vp(p), 2, 4, 2, 66, 0, 1, 0, S), 'skinny_linear_fwd', [(t, b)])
    # stem_im2col at W = 2043: wider than the row staging buffer
    t, p, b = _frame('f32', 1022, 128)
    _refused(L, lib, lib.sedt_stem_im2col(vp(src), vp(p), 1, 1, 2043, 0, S), 'stem_im2col', [(t, b)])
    # add_n: nine pointers; an element count that is no multiple of 8
    t, p, b = _frame('f32', 1, 16)
    arr = (C.c_void_p * 9)(*[src] * 9)
    _refused(L, lib, lib.sedt_add_n(arr, 9, vp(p), 16, 0, S), 'add_n', [(t, b)])
    _refused(L, lib, lib.sedt_add_n(arr, 2, vp(p), 12, 0, S), 'add_n', [(t, b)])
    # split3: cols % 4 != 0
    t, p, b = _frame('bf16', 2, 12)
    job = (L.SedtSplitJob * 1)()
    job[0].src, job[0].ld, job[0].dst, job[0].rows, job[0].cols, job[0].pattern = src, 8, p, 2, 6, 0
    _refused(L, lib, lib.sedt_split3(job, 1, S), 'split3', [(t, b)])
    # pool_at: Q (C + 1) above 4096
    t, p, b = _frame('f32', 1, 64)
    a = L.SedtPoolAt()
    a.logits, a.B, a.Qs, a.q0, a.Q, a.C, a.mode = src, 1, 64, 0, 64, 64, L.POOL_MODES['avg']
    _refused(L, lib, lib.sedt_pool_at(a, vp(p), S), 'pool_at', [(t, b)])
    # spsedt_dec_in in f32: patch / out move as 32-byte vectors - a pointer 16 bytes behind a 32-byte boundary is refused since this
    # module's fix (it passed the earlier 16-byte test)
    t, p, b = _frame('f32', 2, 64)
    assert src % 32 == 0 and p % 32 == 0
    _refused(L, lib, lib.sedt_spsedt_dec_in(vp(src + 16), vp(src), None, None, vp(p), 1, 2, 2, 1, 64, 0, 0.0, 0, None, 0, S), 'spsedt_dec_in', [(t, b)])
    _refused(L, lib, lib.sedt_spsedt_dec_in(vp(src), vp(src), None, None, vp(p + 16), 1, 1, 1, 1, 64, 0, 0.0, 0, None, 0, S), 'spsedt_dec_in', [(t, b)])
    # ... while bf16 moves 16-byte vectors: the same offset is inside its envelope (one row, inside the frame)
    t, p, b = _frame('bf16', 2, 64)
    L.check(lib.sedt_spsedt_dec_in(vp(src + 16), vp(src), None, None, vp(p), 1, 2, 2, 1, 64, 0, 0.0, 0, None, 1, S), 'spsedt_dec_in')
    torch.cuda.synchronize()
    del src_t, big_t


def test_empty_tensors_launch_nothing(env):
    """the entry points that can be handed an empty tensor return 0 without a launch (a grid of 0 blocks is a launch error): status 0,
    no pending HIP error, the frame untouched.  (The rows n0 / B0 / rows 0 of the tables run the same calls through run_row.)"""
    L, lib, ops = env
    S = L.stream_ptr()
    t, p, b = _frame('f32', 1, 8)
    src_t, src = up(np.ones(64, np.float32))
    calls = [('add', lambda: lib.sedt_add(vp(src), vp(src), vp(p), 0, 8, 0, 0, S)),
             ('cast', lambda: lib.sedt_cast(vp(src), 0, vp(p), 1, 0, S)),
             ('relu_mask', lambda: lib.sedt_relu_mask(vp(src), vp(src), vp(p), 0, 0, S)),
             ('sigmoid_grad', lambda: lib.sedt_sigmoid_grad(vp(src), vp(src), vp(p), 0, S)),
             ('avgpool', lambda: lib.sedt_avgpool(vp(src), vp(p), 0, 4, 8, 0, S)),
             ('mask_resize', lambda: lib.sedt_mask_resize(vp(src), vp(p), 0, 4, 4, 2, 2, S)),
             ('dropout_grad', lambda: lib.sedt_dropout_grad(vp(src), 8, vp(p), 8, 0, 8, 0.1, 1, None, 0, S)),
             ('gelu_fwd', lambda: lib.sedt_gelu_fwd(vp(src), vp(p), 0, 0.1, 1, None, 0, S)),
             ('gelu_bwd', lambda: lib.sedt_gelu_bwd(vp(src), vp(src), vp(p), 0, 0.1, 1, None, 0, S)),
             ('add_n', lambda: lib.sedt_add_n((C.c_void_p * 2)(src, src), 2, vp(p), 0, 0, S))]
    for name, call in calls:
        assert call() == 0, (name, lib.sedt_last_error().decode())
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), b)
    del src_t
