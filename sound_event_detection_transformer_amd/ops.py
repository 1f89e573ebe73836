"""Tensor-level wrappers over the C ABI (include/sedt_hip.h).

Every function takes torch tensors that live on the GPU, passes raw device pointers + sizes to
libsedt_hip.so on the current torch stream and returns torch tensors allocated with the caching
allocator.  No arithmetic happens in torch here; torch is device memory + streams only.
"""
import ctypes as C
from collections import namedtuple

import os
import numpy as np
import torch

from . import lib as L
from .lib import F32, BF16, ACT_NONE, ACT_RELU, ACT_SIGMOID, TORCH_DTYPE, p as _p  # noqa: F401


class ConvGeom(object):
    """geometry of one convolution over NHWC activations"""
    __slots__ = ('Hi', 'Wi', 'Ci', 'Ho', 'Wo', 'Co', 'KH', 'KW', 'sh', 'sw', 'ph', 'pw', 'dh', 'dw')

    def __init__(self, Hi, Wi, Ci, Co, k=1, stride=1, pad=0, dil=1):
        self.Hi, self.Wi, self.Ci, self.Co = Hi, Wi, Ci, Co
        self.KH = self.KW = k
        self.sh = self.sw = stride
        self.ph = self.pw = pad
        self.dh = self.dw = dil
        self.Ho = (Hi + 2 * pad - dil * (k - 1) - 1) // stride + 1
        self.Wo = (Wi + 2 * pad - dil * (k - 1) - 1) // stride + 1

    @property
    def taps(self):
        return self.KH * self.KW

    @property
    def plain(self):
        return self.KH == 1 and self.KW == 1 and self.sh == 1 and self.sw == 1 and self.ph == 0 and self.pw == 0


def _dev_env(name, default):
    """a developer A/B switch: the environment is consulted only when SEDT_DEV=1 is set as well (tools/README.md); a training job's
    behaviour never depends on a leaked variable"""
    return os.environ.get(name, default) if os.environ.get('SEDT_DEV') == '1' else default


IGEMM_BREG = _dev_env('SEDT_IGEMM_BREG', '0') != '0'   # developer A/B switch (csrc/igemm3.hip, BR = 1): weights through registers out of their fragment-major images
RELU_BITS = _dev_env('SEDT_RELU_BITS', '1') != '0'      # developer A/B switch: 0 = the backward masks with the bf16 activations
PROFILE = None   # bench.py sets this to a list: every GEMM launch then also records (argument block, dtype, shape, operands, hint)
# hint (igemm's argument): how the un-recorded step launches the problem being recorded - 'conv3x3_c64_kernel' (direct kernel), ('group', kernel
# label, share of the recorded problem's flops the grouped form executes), 'wgrad_group'; None: as recorded
PROFILE_FUSED = []     # with PROFILE on: (kernel-name prefix, algorithmic flop, algorithmic bytes) of every fused-Bottleneck launch of the recorded step


def _dev_check(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('sedt ops need GPU tensors: the HIP path has no CPU fallback')


def igemm_args(M, N, K, A, lda, B, ldb, Cout, ldc, *, trans=0, conv=None, transposed=0, out_f32=0, scale=None,
               bias=None, res=None, ldr=0, res_mod=0, mask=None, ldm=0, act=ACT_NONE, act_post_res=0, alpha=1.0, drop_p=0.0,
               seed=0, seed_ptr=None, splitk=1, slab=None, tile=(0, 0), colsum_out=None, mask_bits=False, bits_out=None, res_map=None):
    """the SedtIgemm argument block of one implicit GEMM; ``conv`` = (Hi, Wi, Ci, Ho, Wo, KH, KW, sh, sw, ph, pw, dh, dw);
    ``res_map`` = (r_Hi, r_Wi, r_sh, r_sw): ``res`` lives on the coarse grid of an r_Hi x r_Wi image (SedtIgemm.rmap)"""
    _dev_check(A, B, Cout)
    a = L.SedtIgemm()
    a.M, a.N, a.K = M, N, K
    a.A, a.B, a.lda, a.ldb = A.data_ptr(), B.data_ptr(), lda, ldb
    a.trans, a.transposed = trans, transposed
    if conv is not None:
        a.conv = 1
        (a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.KH, a.KW, a.sh, a.sw, a.ph, a.pw, a.dh, a.dw) = conv
    else:
        a.conv = 0
        a.KH = a.KW = a.sh = a.sw = a.dh = a.dw = 1
    a.C = Cout.data_ptr() if Cout is not None else None
    a.ldc, a.out_f32 = ldc, out_f32
    a.scale = scale.data_ptr() if scale is not None else None
    a.bias = bias.data_ptr() if bias is not None else None
    a.res = res.data_ptr() if res is not None else None
    a.ldr, a.res_mod = ldr, res_mod
    if res_map is not None:
        r_Hi, r_Wi, r_sh, r_sw = res_map
        assert res is not None and not res_mod and 1 <= r_Hi < 4096 and 1 <= r_Wi < 4096 and 1 <= r_sh < 16 and 1 <= r_sw < 16, res_map
        a.rmap = C.c_int32(r_Hi | r_Wi << 12 | r_sh << 24 | r_sw << 28).value
    a.mask = mask.data_ptr() if mask is not None else None
    a.ldm = ldm
    a.act, a.act_post_res, a.alpha = act, act_post_res, alpha
    a.drop_p, a.seed = drop_p, seed & 0xffffffff
    a.seed_ptr = seed_ptr.data_ptr() if seed_ptr is not None else None
    a.splitk = splitk
    a.slab = slab.data_ptr() if slab is not None else None
    a.tile_m, a.tile_n = tile
    a.colsum_out = colsum_out.data_ptr() if colsum_out is not None else None
    if mask_bits:                                   # 1-bit ReLU mask: uint8 [M, N/8] image, ldm in bytes
        assert mask is not None and mask.dtype == torch.uint8
        a.mask_bits = 1
    if bits_out is not None:                        # sign bits of the stored output, uint8 [M, N/8]
        assert bits_out.dtype == torch.uint8 and bits_out.shape == (M, N // 8) and N % 8 == 0 and bits_out.stride(1) == 1 and not trans
        a.bits_out, a.ldbits = bits_out.data_ptr(), bits_out.stride(0)
    if IGEMM_BREG and not trans and B.dtype == torch.bfloat16:
        from . import packing
        fr = packing.lookup_operand_frag(B.data_ptr())
        if fr is not None and fr.numel() == B.numel() and ldb * B.shape[0] == B.numel():
            a.bfrag = fr.data_ptr()
    return a


class WgradPool(object):
    """Weight-gradient GEMMs waiting for a ride (co-scheduling, csrc/igemm3.hip: igemm3_co_kernel).

    In the backward pass only the dgrad chain is ordered; a layer's weight gradients are needed by the optimizer alone.
    While ``coschedule()`` is active, ReduceBatch.flush() parks the layer's wgrad problems here instead of launching
    them, and every following forward/dgrad GEMM launch takes a few along in the workgroup slots it would leave idle
    (at batch 64 most GEMMs of the chain fill 2 of ~5 slots per CU).  ``drain()`` - called before anything reads the
    gradients - launches what is left and then all split-K reductions."""
    SLOTS = 1280                    # 256 CUs x 5 resident workgroups of the 32 KB-LDS GEMM kernels
    MAX_RIDERS = 10

    def __init__(self):
        self.gemms, self.reduces, self.keep, self.dtype = [], [], [], None

    def push(self, group, dtype, jobs, keep, operands):
        self.gemms.extend(group)
        self.reduces.extend(jobs)
        self.keep.append((keep, operands))
        self.dtype = dtype

    def take(self, main_tiles):
        if NO_RIDE:
            return []
        room = max(self.SLOTS - main_tiles, 512)
        out = []
        while self.gemms and len(out) < self.MAX_RIDERS:
            a = self.gemms[0][0]
            wgs = ((a.M + 63) // 64) * ((a.N + 63) // 64) * max(a.splitk, 1)
            if out and wgs > room:
                break
            out.append(self.gemms.pop(0))
            room -= wgs
        return out

    def give_back(self, items):
        self.gemms[0:0] = items

    def drain(self):
        lib = L.load()
        while self.gemms:
            chunk, self.gemms = self.gemms[:10], self.gemms[10:]
            arr = (L.SedtIgemm * len(chunk))(*[c[0] for c in chunk])
            L.check(lib.sedt_wgrad_group(arr, len(chunk), L.gemm_dtype(self.dtype), L.stream_ptr()), 'wgrad_group')
        while self.reduces:
            chunk, self.reduces = self.reduces[:L.MAX_REDUCE_JOBS], self.reduces[L.MAX_REDUCE_JOBS:]
            arr = (L.SedtReduceJob * len(chunk))(*chunk)
            L.check(lib.sedt_multi_wgrad_reduce(arr, len(chunk), None, L.stream_ptr()), 'multi_wgrad_reduce')
        self.keep = []


POOL = WgradPool()
_co = {'on': False}


class coschedule(object):
    """context manager: weight gradients computed inside are complete only after the scope exits (it drains the pool)"""

    def __init__(self, enable=True):
        self.enable = enable

    def __enter__(self):
        self.prev = _co['on']
        _co['on'] = bool(self.enable) and PROFILE is None
        return self

    def __exit__(self, *exc):
        _co['on'] = self.prev
        if not self.prev:
            POOL.drain()
        return False


# ---- the fast bf16x3 mode (csrc/split3.hip): an f32-mode GEMM whose shape fits the LDS-DMA kernels runs as ONE bf16 GEMM over a three
# times longer contraction axis, on operands split once into bf16 [hi | lo | hi] / [hi | hi | lo] images, with an f32 epilogue.
# X3_FAST = False keeps every contraction of the mode on the register-staged generic kernel (csrc/igemm.hip, the round-4 form).
X3_FAST = _dev_env('SEDT_X3_FAST', '1') != '0'


# An activation / gradient is a GEMM operand twice per step (x: its layer's forward and weight gradient; dY: input and weight gradient):
# its [hi | lo] image is kept from the first use to the second.  Keyed by (pointer, rows, cols, row stride); an entry holds the
# SOURCE tensor as well, so the caching allocator cannot hand that memory to another tensor while the entry lives, and the source's
# autograd version counter at the time the image was made: a torch in-place op on a cached operand bumps the counter and the stale
# image is dropped at the next lookup.  Writes through this library's own raw pointers do not bump it, so a GEMM that writes a tensor
# WITHOUT leaving its image (no split_out) pops that tensor's entry (igemm / _igemm_x3_fast).  Emptied when a model forward starts
# (packing.PlanSet / PackPlan) and by the optimizer step.
X3_CACHE = {}
# weight operand images [rows][3 cols] = [hi | hi | lo] of WHOLE packed operands, by base pointer: (rows, cols, ld, image, source tensor).
# A GEMM asks for its weight's image; on a miss ONE split launch makes it together with the next few operands the model consumes
# (packing.weight_neighbours), row slices of a cached operand (the q|k and v halves of an in_proj weight) are views of its image.
W3_CACHE = {}
W3_STARTS = []                      # sorted base pointers of W3_CACHE (range lookup for row slices)
X3_WGROUP = int(_dev_env('SEDT_X3_WGROUP', '3'))       # further operands prepared with the one that missed (0: one split launch per weight).
# Same-box A/B on the C2 bf16x3 step (profiles/r06_ab_x3_wgroup.txt): 0 -> 13.74-13.78 ms, 3 -> 13.69-13.72, 5 -> 13.85-13.87, 7 -> 13.83-13.93:
# an image made more than a few GEMMs ahead of its use is read back cold, which costs more than the launches it saves
X3_CACHE_ON = _dev_env('SEDT_X3_CACHE', '1') != '0'
X3_SPLIT_OUT = _dev_env('SEDT_X3_SPLIT_OUT', '1') != '0'      # GEMM epilogues write the operand image of outputs that feed GEMMs again


def x3_cache_clear():
    X3_CACHE.clear()
    W3_CACHE.clear()
    del W3_STARTS[:]


def _w3_lookup(ptr, rows, cols, ld):
    """image of the weight operand (ptr, rows, cols, ld) if it is a cached operand or a row slice of one"""
    import bisect
    k = bisect.bisect_right(W3_STARTS, ptr) - 1
    if k < 0:
        return None
    base = W3_STARTS[k]
    r_, c_, ld_, img, src = W3_CACHE[base]
    off = ptr - base
    if c_ != cols or ld_ != ld or off % (4 * ld) or off // (4 * ld) + rows > r_:
        return None
    r0 = off // (4 * ld)
    return img[r0:r0 + rows]


def _w3_plan(t, off, rows, cols, ld):
    """split jobs (tensor, 0, rows, cols, ld, 1) that make the missing weight image AND those of the operands consumed next"""
    from . import packing
    ptr = t.data_ptr() + 4 * off
    jobs = []
    if X3_WGROUP > 0 and X3_CACHE_ON:
        for wt, r_, c_ in packing.weight_neighbours(ptr, X3_WGROUP):
            if wt.data_ptr() in W3_CACHE or c_ % 64 or (wt.data_ptr() % 16):
                continue
            jobs.append((wt, 0, r_, c_, c_, 1))
    return jobs


SPLIT_MAXJ = 8                      # jobs per sedt_split3 launch (csrc/split3.hip)


def _split3(jobs):
    """jobs: (tensor, element offset of the view's first element, rows, cols, row stride, pattern); one launch for up to SPLIT_MAXJ.  Returns
    the bf16 images: [rows, 2 * cols] = [hi | lo] for pattern 0 (activations / gradients), [rows, 3 * cols] = [hi | hi | lo] for pattern 1 (weights)"""
    import bisect
    outs, todo = [None] * len(jobs), []           # todo: (job tuple, destination, index in outs or None)
    for i, (t, off, rows, cols, ld, pattern) in enumerate(jobs):
        key = (t.data_ptr() + 4 * off, rows, cols, ld)
        if pattern == 1 and X3_CACHE_ON:
            hit = _w3_lookup(key[0], rows, cols, ld)
            if hit is not None:
                outs[i] = hit
                continue
            extra = _w3_plan(t, off, rows, cols, ld)
            for wt, _, r_, c_, ld_, _ in extra[:SPLIT_MAXJ - len(jobs)]:
                d = torch.empty((r_, 3 * c_), device=wt.device, dtype=torch.bfloat16)
                todo.append(((wt, 0, r_, c_, ld_, 1), d, None))
                W3_CACHE[wt.data_ptr()] = (r_, c_, ld_, d, wt)
                bisect.insort(W3_STARTS, wt.data_ptr())
            hit = _w3_lookup(key[0], rows, cols, ld)          # (the operand itself is the first neighbour when a plan knows it)
            if hit is not None:
                outs[i] = hit
                continue
        hit = X3_CACHE.get(key) if (pattern == 0 and X3_CACHE_ON) else None
        if hit is not None and hit[2] == t._version:
            outs[i] = hit[1]
            continue
        d = torch.empty((rows, (3 if pattern else 2) * cols), device=t.device, dtype=torch.bfloat16)
        outs[i] = d
        todo.append(((t, off, rows, cols, ld, pattern), d, i))
        if pattern == 0 and X3_CACHE_ON:
            if len(X3_CACHE) >= 1024:           # (op-level callers outside a model forward never reach a clearing point: bound what is held)
                X3_CACHE.clear()
            X3_CACHE[key] = (t, d, t._version)
    for base in range(0, len(todo), SPLIT_MAXJ):
        chunk = todo[base:base + SPLIT_MAXJ]
        arr = (L.SedtSplitJob * len(chunk))()
        for n, ((t, off, rows, cols, ld, pattern), d, _) in enumerate(chunk):
            arr[n].src, arr[n].ld, arr[n].dst = t.data_ptr() + 4 * off, ld, d.data_ptr()
            arr[n].rows, arr[n].cols, arr[n].pattern = rows, cols, pattern
        L.check(L.load().sedt_split3(arr, len(chunk), L.stream_ptr()), 'split3')
    return outs


def _x3_rows(M, conv):
    """rows of the gathered operand: the pixels of the B images behind the M output rows (conv = igemm_args' geometry tuple)"""
    if conv is None:
        return M
    Hi, Wi, _, Ho, Wo = conv[:5]
    return (M // (Ho * Wo)) * Hi * Wi


def _x3_fast_ok(M, N, K, A, lda, B, ldb, Cout, ldc, kw):
    """envelope of the LDS-DMA forward / dgrad kernels on the tripled contraction (lds_plan, csrc/igemm3.hip) with f32 epilogue operands"""
    conv = kw.get('conv')
    if not X3_FAST or kw.get('trans', 0) or kw.get('splitk', 1) > 1 or kw.get('act', ACT_NONE) == ACT_SIGMOID or kw.get('slab') is not None:
        return False
    if Cout is None or Cout.dtype != torch.float32 or A.dtype != torch.float32 or B.dtype != torch.float32:
        return False
    Ci = conv[2] if conv is not None else K
    if K % 64 or Ci % 64 or N % 8 or ldc % 8 or lda % 4 or ldb % 4 or A.data_ptr() % 16 or B.data_ptr() % 16 or Cout.data_ptr() % 16:
        return False
    if conv is not None:
        taps = conv[5] * conv[6]
        if ldb != K or taps * Ci != K or taps > 32 or M % (conv[3] * conv[4]):
            return False
        if kw.get('transposed', 0) and (conv[7] != conv[8] or (2 * Ci) % conv[7]):
            return False
    res, mask = kw.get('res'), kw.get('mask')
    if res is not None and (res.dtype != torch.float32 or res.data_ptr() % 16 or kw.get('ldr', 0) % 4):
        return False
    if mask is not None and not kw.get('mask_bits') and (mask.dtype != torch.float32 or mask.data_ptr() % 16 or kw.get('ldm', 0) % 4):
        return False
    if mask is not None and kw.get('mask_bits') and (mask.data_ptr() % 4 or kw.get('ldm', 0) % 4):     # 1-bit image: ldm in BYTES (igemm3.hip envelope)
        return False
    for k_ in ('scale', 'bias'):                      # per-column epilogue operands are read as 16-byte vectors (lds_plan)
        t_ = kw.get(k_)
        if t_ is not None and t_.data_ptr() % 16:
            return False
    rows = _x3_rows(M, conv)
    return rows * 3 * Ci * 2 < (1 << 31) and N * 3 * K * 2 < (1 << 31)


def _describe(a, code, njobs=0):
    """the kernel instance sedt_igemm runs the problem `a` on, or (njobs > 0) sedt_igemm_group the njobs problems of the array `a`, as a
    profiler prints it; None when the call is refused.  Nothing is launched"""
    buf = C.create_string_buffer(160)
    if njobs:
        r = L.load().sedt_igemm_group_describe(a, njobs, code, buf, 160)
    else:
        r = L.load().sedt_igemm_describe(C.byref(a), code, 0, buf, 160)
    return buf.value.decode() if r == 0 else None


def _launch_igemm(a, code, shape, kept, hint, x3=False):
    """the tail of every single-GEMM launch: record it (the operand tensors `kept` alive, so that the launch can be replayed for timing), count
    the kernel instance the dispatcher picks in the launch log (lib.launch_log()), launch"""
    if PROFILE is not None:
        PROFILE.append((a, code, shape, kept, hint))
    if L.LAUNCH_LOG is not None:
        name = _describe(a, code)
        if name is not None:
            L.LAUNCH_LOG['igemm_x3:' + name if x3 else 'igemm:' + name.split('(')[0]] += 1
    L.check(L.load().sedt_igemm(C.byref(a), code, L.stream_ptr()), 'sedt_igemm_x3' if x3 else 'sedt_igemm')


def _igemm_x3_fast(M, N, K, A, lda, B, ldb, Cout, ldc, kw, hint):
    conv = kw.get('conv')
    Ci = conv[2] if conv is not None else K
    rows = _x3_rows(M, conv)
    wjob = (B, 0, N * (K // Ci), Ci, Ci, 1) if conv is not None else (B, 0, N, K, ldb, 1)
    A3, B3 = _split3([(A, 0, rows, Ci, lda, 0), wjob])
    kw = dict(kw)
    if conv is not None:
        kw['conv'] = (conv[0], conv[1], 3 * Ci) + tuple(conv[3:])
    kw['out_f32'] = 1
    a = igemm_args(M, N, 3 * K, A3, 2 * Ci, B3, 3 * K, Cout, ldc, **kw)
    a.f32ep, a.awrap = 1, Ci                 # (the A image is [hi | lo]: the walk over 3 Ci wraps back onto hi)
    # outputs that feed GEMMs again - a ReLU'd activation (the Bottleneck chain, the FFN's hidden layer, the box MLP) or a masked
    # gradient (the dgrad chain: the next input gradient AND a weight gradient read it) - leave their operand image from the epilogue:
    # the consumers find it in the cache instead of running a split pass (read 4 B + write 6 B per element and a launch saved)
    img = None
    if X3_CACHE_ON and X3_SPLIT_OUT and (kw.get('act', ACT_NONE) == ACT_RELU or kw.get('mask') is not None) and N % 8 == 0:
        img = torch.empty((M, 2 * N), device=Cout.device, dtype=torch.bfloat16)
        a.split_out = img.data_ptr()
        X3_CACHE[(Cout.data_ptr(), M, N, ldc)] = (Cout, img, Cout._version)
    else:
        X3_CACHE.pop((Cout.data_ptr(), M, N, ldc), None)          # (rewritten without a new image: a cached one would be stale)
    _launch_igemm(a, BF16, (M, N, 3 * K, 0, 0 if conv is None else 1), (A, B, Cout, kw, A3, B3), hint, x3=True)


def igemm(dtype, M, N, K, A, lda, B, ldb, Cout, ldc, hint=None, **kw):
    """raw implicit GEMM call (arguments as igemm_args); hint: what a recording notes beside the problem (PROFILE)"""
    if dtype == F32 and L.GEMM_X3 and _x3_fast_ok(M, N, K, A, lda, B, ldb, Cout, ldc, kw):
        return _igemm_x3_fast(M, N, K, A, lda, B, ldb, Cout, ldc, kw, hint)
    if dtype == F32 and L.GEMM_X3 and Cout is not None and X3_CACHE:
        X3_CACHE.pop((Cout.data_ptr(), M, N, ldc), None)          # the generic kernel rewrites Cout and leaves no operand image
    a = igemm_args(M, N, K, A, lda, B, ldb, Cout, ldc, **kw)
    conv, trans = kw.get('conv'), kw.get('trans', 0)
    if (dtype == BF16 and kw.get('out_f32') and not trans and kw.get('res') is None and (kw.get('mask') is None or kw.get('mask_bits'))
            and kw.get('act', ACT_NONE) != ACT_SIGMOID):
        # an f32 OUTPUT of bf16 operands (SP-SEDT's feature_align head: 12,000 x 2048 at C4): the LDS-DMA kernels write f32 through
        # their f32 epilogue (SedtIgemm.f32ep); asked for only when the dispatcher says the problem is inside their envelope
        a.f32ep = 1
        if not (_describe(a, L.gemm_dtype(dtype)) or '').startswith('igemm3'):
            a.f32ep = 0
    if _co['on'] and POOL.gemms and not trans and dtype == BF16:
        riders = POOL.take(((M + 63) // 64) * ((N + 63) // 64))
        arr = (L.SedtIgemm * len(riders))(*[r[0] for r in riders])
        taken = C.c_int(0)
        L.check(L.load().sedt_igemm_co(C.byref(a), arr, len(riders), L.gemm_dtype(dtype), L.stream_ptr(), C.byref(taken)), 'sedt_igemm_co')
        if not taken.value:
            POOL.give_back(riders)
        return
    _launch_igemm(a, L.gemm_dtype(dtype), (M, N, K, trans, 0 if conv is None else 1), (A, B, Cout, kw), hint)


def _geom_tuple(g, transposed=False):
    if transposed:   # rows run over the conv INPUT grid, gathered tensor is dY on the conv OUTPUT grid
        return (g.Ho, g.Wo, g.Co, g.Hi, g.Wi, g.KH, g.KW, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw)
    return (g.Hi, g.Wi, g.Ci, g.Ho, g.Wo, g.KH, g.KW, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw)


def linear(dtype, x, w, out=None, *, bias=None, out_f32=False, **ep):
    """y[M,N] = epilogue(x[M,K] @ w[N,K]^T); x/w may be row-strided views (last dim contiguous)"""
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_f32 else TORCH_DTYPE[dtype])
    igemm(dtype, M, N, K, x, x.stride(0), w, w.stride(0), out, out.stride(0), bias=bias, out_f32=int(out_f32), **ep)
    return out


def skinny_ok(N, K):
    """envelope of the direct small-N linear kernels (csrc/skinny.hip)"""
    return N <= 16 and K % 64 == 0 and K <= 1024


def skinny_linear_fwd(dtype, x, w, bias=None, act=ACT_NONE, out_f32=False):
    """y = act(x @ w^T + b) for N <= 16 output features straight from the f32 master weight (no packing)"""
    _dev_check(x, w)
    M, K = x.shape
    N = w.shape[0]
    assert w.dtype == torch.float32 and w.is_contiguous() and x.stride(1) == 1
    y = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_f32 else TORCH_DTYPE[dtype])
    L.check(L.load().sedt_skinny_linear_fwd(_p(x), x.stride(0), _p(w), _p(bias), _p(y), y.stride(0), M, N, K, act, int(out_f32), dtype,
                                            L.stream_ptr()), 'skinny_linear_fwd')
    return y


def skinny_linear_bwd(dtype, g, ysaved, w, x, act=ACT_NONE, mask=None, need_gx=True, need_gw=True, need_gb=True, gx_acc=None, batch=None):
    """(gx, dW, db) of skinny_linear_fwd; g f32 [M,N]; ysaved = the f32 output when act != NONE.  x may be a strided row view
    (stride(1) == 1).  gx_acc: a [M,K] (row-strided) view the input gradient is ADDED to instead of a fresh gx.
    batch (a ReduceBatch): the final sum of the 16 partial slabs rides in batch.flush() (dW / db are valid only then)"""
    M, K = x.shape
    N = w.shape[0]
    assert g.dtype == torch.float32 and g.is_contiguous() and (ysaved is None or (ysaved.dtype == torch.float32 and ysaved.is_contiguous()))
    assert x.stride(1) == 1
    if gx_acc is not None:
        assert gx_acc.shape == (M, K) and gx_acc.stride(1) == 1 and gx_acc.dtype == TORCH_DTYPE[dtype] and mask is None
        gx = gx_acc
    else:
        gx = torch.empty((M, K), device=x.device, dtype=TORCH_DTYPE[dtype]) if need_gx else None
    dw = torch.empty((N, K), device=x.device, dtype=torch.float32) if need_gw else None
    db = torch.empty((N,), device=x.device, dtype=torch.float32) if (need_gb and need_gw) else None
    lib = L.load()
    scratch = torch.empty((lib.sedt_skinny_linear_bwd_scratch(K) // 4,), device=x.device, dtype=torch.float32) if need_gw else None
    deferred = need_gw and batch is not None
    L.check(lib.sedt_skinny_linear_bwd(_p(g), _p(ysaved), g.stride(0), _p(w), _p(x), x.stride(0), _p(mask),
                                       mask.stride(0) if mask is not None else 0, _p(gx), gx.stride(0) if gx is not None else K,
                                       None if deferred else _p(dw), None if deferred else _p(db),
                                       _p(scratch), M, N, K, act, int(gx_acc is not None), dtype, L.stream_ptr()), 'skinny_linear_bwd')
    if deferred:                                  # sum of the 16 slabs [17][K] as a column-sum job of the batch's reduce launch
        tot = torch.empty((17 * K,), device=x.device, dtype=torch.float32)
        batch.add_colsum(scratch, 16, 17 * K, tot)
        dw = tot[:N * K].view(N, K)
        db = tot[16 * K:16 * K + N] if need_gb else None
    if need_gb and not need_gw:
        db = g.sum(0) if act == ACT_NONE else (g * ysaved * (1 - ysaved)).sum(0) if act == ACT_SIGMOID else (g * (ysaved > 0)).sum(0)
    return gx, dw, db


def _group_label(jobs):
    """bench.py's recorded step runs a group's problems one by one; this is the kernel instance the UN-recorded step launches them on as one
    group (sedt_igemm_group_describe), so that roofline.families books their flops on the row that actually ran"""
    return _describe((L.SedtIgemm * len(jobs))(*jobs), BF16, len(jobs)) or None


def linear_group(dtype, items):
    """several independent ``linear`` calls (each item: (x, w, kwargs of linear)) as one launch when the kernel allows it
    (sedt_igemm_group) - the q / k / v projections of an attention block, or their three dgrads.  Returns the outputs."""
    outs, args = [], []
    for x, w, kw in items:
        kw = dict(kw)
        M, K = x.shape
        N = w.shape[0]
        out_f32 = kw.pop('out_f32', False)
        out = kw.pop('out', None)
        if out is None:
            out = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_f32 else TORCH_DTYPE[dtype])
        outs.append(out)
        args.append(((M, N, K, x, x.stride(0), w, w.stride(0), out, out.stride(0)), dict(out_f32=int(out_f32), **kw)))
    if len(args) == 1 or PROFILE is not None or (_co['on'] and POOL.gemms) or (dtype == F32 and L.GEMM_X3 and X3_FAST):
        hint = None
        if len(args) > 1 and PROFILE is not None and dtype == BF16:
            hint = ('group', _group_label([igemm_args(*a, **kw) for a, kw in args]), 1.0)
        for a, kw in args:
            igemm(dtype, *a, hint=hint, **kw)
        return outs
    arr = (L.SedtIgemm * len(args))(*[igemm_args(*a, **kw) for a, kw in args])
    L.check(L.load().sedt_igemm_group(arr, len(args), L.gemm_dtype(dtype), L.stream_ptr()), 'igemm_group')
    return outs


# ---- the launch form of a convolution.  conv_fwd / conv_dgrad run every backbone convolution that is not a fused Bottleneck; three special
# forms stand beside the generic implicit GEMM.  conv_form decides, the envelopes below say when a form applies, CONV_FORMS holds the
# precedence.  A recording (PROFILE) launches the generic kernel whatever the plan and notes the planned form as the entry's hint.
#
# s2_parity: the input gradient of a stride-2 3x3 convolution (layer2 / layer3 block 0) by OUTPUT PARITY.  The transposed gather of the plain
# form walks all nine taps for every input pixel, but a pixel (hi, wi) only ever receives taps with kh = hi + 1 and kw = wi + 1 (mod 2): three
# of four (tap, pixel) pairs multiply rows of zeros.  Split by the parity of (hi, wi) the problem is four small REGULAR convolutions over dY -
# 1, 2, 2 and 4 taps - whose outputs interleave in dx: one grouped launch (sedt_igemm_group) of four problems that read their tap blocks of
# the packed dgrad weight in place (SedtIgemm.btap) and write every second row / column of dx (SedtIgemm.omap), epilogue operands (residual,
# ReLU mask bits) indexed by the dx pixel.  A quarter of the MFMAs, the same sums in the same order.
#
# dil_halves: layer4's dilated 3x3 convolutions (dilation 2, padding 2) run on a map of FOUR columns: the left tap column (kw = 0) lands inside
# the image only for output columns 2, 3 and the right one (kw = 2) only for columns 0, 1 - a third of the tap walk multiplies zero rows.
# Split by column half, each half is a regular 3 x 2-tap convolution over all four input columns with its own six tap blocks of the packed
# weight (btap) and its own two output columns (omap): two problems of 128 tiles of 128x128 in ONE grouped ping-pong launch
# (igemm3_w8_group_kernel), 2/3 of the K loop each.  Forward and input gradient (the mirror image) alike.
#
# Both grouped forms run in bf16 and in the fast bf16x3 form of the f32 mode (split operand images, f32 epilogue).
S2_PARITY = _dev_env('SEDT_S2_PARITY', '1') != '0'
DIL_HALVES = _dev_env('SEDT_DIL_HALVES', '1') != '0'


def _direct3x3_ok(kind, dtype, t, g, w, out, ep):
    """envelope of the direct 3x3 kernel (csrc/conv3x3_c64.hip): the layer1 conv2 geometry, plain epilogues.  The input gradient of a
    stride-1 3x3 conv is the same conv, taps flipped: the kernel takes it when no per-channel scale / bias is asked for"""
    return (CONV3_DIRECT and dtype == BF16 and g.Ci == 64 and g.Co == 64 and g.KH == 3 and g.KW == 3
            and g.sh == 1 and g.sw == 1 and g.ph == 1 and g.pw == 1 and g.dh == 1 and g.dw == 1 and g.Wi == 16
            and t.stride(0) == 64 and out.stride(0) == 64 and set(ep) <= {'scale', 'bias', 'act', 'mask', 'ldm', 'tile'}
            and ep.get('act', 0) in (0, ACT_RELU) and tuple(ep.get('tile', (0, 0))) == (0, 0)
            and (ep.get('mask') is None or (ep.get('ldm', 64) == 64 and ep.get('act', 0) == 0))
            and (kind == 'fwd' or ('scale' not in ep and 'bias' not in ep)))


def _grouped_ok(dtype, t, out, ep):
    """what both grouped forms ask: no co-scheduled riders; bf16, or the fast bf16x3 form of the f32 mode on f32 operands whose images the
    split kernel can make (16-byte aligned rows).  A grouped form that passes runs on split operands (x3) exactly when dtype is F32"""
    x3 = dtype == F32 and L.GEMM_X3 and X3_FAST
    if _co['on'] or not (dtype == BF16 or x3):
        return False
    return not x3 or (t.dtype == torch.float32 and out.dtype == torch.float32 and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0
                      and (ep.get('res') is None or ep['res'].dtype == torch.float32)
                      and (ep.get('mask') is None or ep.get('mask_bits') or ep['mask'].dtype == torch.float32))


def _s2_parity_ok(kind, dtype, dy, g, wb, out, ep):
    return (S2_PARITY and kind == 'dgrad' and _grouped_ok(dtype, dy, out, ep) and g.KH == 3 and g.KW == 3 and g.sh == 2 and g.sw == 2
            and g.ph == 1 and g.pw == 1 and g.dh == 1 and g.dw == 1 and g.Co % 64 == 0 and g.Ci % 8 == 0 and wb.stride(0) == 9 * g.Co
            and dy.stride(0) % 8 == 0 and out.stride(0) % 8 == 0 and set(ep) <= {'mask', 'ldm', 'mask_bits', 'res', 'ldr', 'alpha'})


def _dil_halves_ok(kind, dtype, t, g, w, out, ep):
    d = g.dh
    cin, cout = (g.Co, g.Ci) if kind == 'dgrad' else (g.Ci, g.Co)          # channels of the gathered tensor / of the output
    return (DIL_HALVES and _grouped_ok(dtype, t, out, ep) and g.KH == 3 and g.KW == 3 and g.sh == 1 and g.sw == 1 and g.dw == d and d >= 1
            and g.ph == d and g.pw == d and g.Wi == 2 * d and g.Wo == g.Wi and g.Ho == g.Hi and cin % 64 == 0 and cout % 128 == 0
            and w.stride(0) == 9 * cin and t.stride(0) % 8 == 0 and out.stride(0) % 8 == 0
            and set(ep) <= {'scale', 'bias', 'act', 'mask', 'ldm', 'mask_bits', 'res', 'ldr', 'alpha', 'bits_out', 'act_post_res'}
            and (t.shape[0] // 2 // 128) * (cout // 128) >= 96)         # (the halves pay while the two problems fill the chip with 128x128 tiles)


# form -> (envelope, share of the nine-tap walk the form executes); a new form is added here and, by kind and in order of precedence, below
_FORMS = {'direct3x3': (_direct3x3_ok, 1.0), 's2_parity': (_s2_parity_ok, 0.25), 'dil_halves': (_dil_halves_ok, 2.0 / 3.0)}
CONV_FORMS = {'fwd': ('direct3x3', 'dil_halves'), 'dgrad': ('s2_parity', 'dil_halves', 'direct3x3')}


def conv_form(kind, dtype, t, g, w, out, ep):
    """(form, x3, share) of the convolution conv_fwd (kind 'fwd', t = x) / conv_dgrad ('dgrad', t = dY) is asked for: the first form of
    CONV_FORMS[kind] whose envelope holds, else 'gemm'; whether the form runs on split operand images; the share of the tap walk it executes.
    Reads the geometry, the epilogue and the operands' dtype / address / strides / rows, and the switches as they stand at the call"""
    for form in CONV_FORMS[kind]:
        ok, share = _FORMS[form]
        if ok(kind, dtype, t, g, w, out, ep):
            return form, form != 'direct3x3' and dtype == F32, share
    return 'gemm', False, 1.0


def _s2_parity_subs(B, g, C_):
    for ph_ in (0, 1):                                   # parity of the input row hi = 2a + ph_
        nh, khs = (g.Hi + 1 - ph_) // 2, ([1] if ph_ == 0 else [0, 2])
        for pw_ in (0, 1):
            nw, kws = (g.Wi + 1 - pw_) // 2, ([1] if pw_ == 0 else [0, 2])
            if nh and nw:
                # a "transposed" stride-1 gather over the dY grid: tap (i, j) of the walk reads dY[a + ph_ - i][b + pw_ - j], i.e. the original
                # taps in ascending (kh, kw) order - rows / columns beyond the grid are masked by the kernel
                yield (B * nh * nw, (g.Ho, g.Wo, C_, nh, nw, len(khs), len(kws), 1, 1, ph_, pw_, 1, 1), (64, 64), (g.Hi, g.Wi, 2, 2, ph_, pw_),
                       [kh * 3 + kw for kh in khs for kw in kws])


def _dil_halves_subs(B, g, C_, transposed):
    d = g.dh
    for half in (0, 1):
        # forward: output columns [0, d) see taps kw in {1, 2}, columns [d, 2d) taps {0, 1}; the input gradient mirrors it
        kw0 = (1 - half) if not transposed else half
        yield (B * g.Ho * d, (g.Hi, g.Wi, C_, g.Ho, d, 3, 2, 1, 1, d, (d if transposed else 0), d, d), (128, 128), (g.Ho, g.Wo, 1, 1, 0, half * d),
               [kh * 3 + kw0 + j for kh in range(3) for j in range(2)])


def conv_group_jobs(form, kind, t, B, g, w, out, ep, x3):
    """the argument blocks of a grouped form ('s2_parity': four problems, 'dil_halves': two), nothing is launched: each a regular
    convolution (rows, geometry, tile, omap = (o_Hi, o_Wi, o_sh, o_sw, o_h0, o_w0), taps of the packed weight [cout][9][cin] it walks)"""
    transposed = kind == 'dgrad'
    cin, cout = (g.Co, g.Ci) if transposed else (g.Ci, g.Co)
    C_ = cin
    if x3:                          # operand images: t [pixels][2 cin] = [hi | lo], the weight [cout][9][3 cin] = [hi | hi | lo] per tap
        t, w = _split3([(t, 0, B * (g.Ho * g.Wo if transposed else g.Hi * g.Wi), cin, t.stride(0), 0), (w, 0, cout * 9, cin, cin, 1)])
        w = w.view(cout, 27 * cin)
        C_ = 3 * cin
    jobs = []
    for M, conv, tile, omap, taps in (_s2_parity_subs(B, g, C_) if form == 's2_parity' else _dil_halves_subs(B, g, C_, transposed)):
        a = igemm_args(M, cout, len(taps) * C_, t, t.stride(0), w, w.stride(0), out, out.stride(0), conv=conv, transposed=int(transposed),
                       tile=tile, out_f32=int(x3), **ep)
        a.omap, (a.o_Hi, a.o_Wi, a.o_sh, a.o_sw, a.o_h0, a.o_w0) = 1, omap
        a.btap_on, a.f32ep, a.awrap = 1, int(x3), (cin if x3 else 0)
        for i, tap in enumerate(taps):
            a.btap[i] = tap * C_
        jobs.append(a)
    return jobs


def conv_hint(kind, plan, t, B, g, w, out, ep):
    """what a recording notes beside the nine-tap problem it runs in place of the planned form: the direct kernel, or the kernel the grouped
    launch of the form's problems runs on and the share of the recorded flops it executes (bf16 only); None: nothing to note"""
    form, x3, share = plan
    if form == 'direct3x3':
        return 'conv3x3_c64_kernel'
    if form == 'gemm' or x3:
        return None
    return ('group', _group_label(conv_group_jobs(form, kind, t, B, g, w, out, ep, False)), share)


def _conv(kind, dtype, t, B, g, w, out, ep):
    """conv_fwd / conv_dgrad: plan, launch the planned form - or, under a recording, the generic GEMM with the plan as its hint"""
    plan = conv_form(kind, dtype, t, g, w, out, ep)
    form, x3, _ = plan
    if PROFILE is None and form == 'direct3x3':
        L.check(L.load().sedt_conv3x3_c64(_p(t), _p(w), int(kind == 'dgrad'), _p(ep.get('scale')), _p(ep.get('bias')),
                                          1 if ep.get('act', 0) == ACT_RELU else 0, _p(ep.get('mask')), _p(out), B, g.Hi, g.Wi, 64,
                                          L.stream_ptr()), 'conv3x3_c64')
    elif PROFILE is None and form != 'gemm':
        jobs = conv_group_jobs(form, kind, t, B, g, w, out, ep, x3)
        L.check(L.load().sedt_igemm_group((L.SedtIgemm * len(jobs))(*jobs), len(jobs), BF16, L.stream_ptr()),
                'igemm_group_s2' if form == 's2_parity' else 'igemm_group_dil')
    else:
        dgrad = kind == 'dgrad'
        if L.LAUNCH_LOG is not None and dgrad and not g.plain:          # (a transposed gather on the general path: which geometry)
            L.LAUNCH_LOG['conv_dgrad_gather:k%ds%d' % (g.KH, g.sh)] += 1
        M, N, K = (B * g.Hi * g.Wi, g.Ci, g.taps * g.Co) if dgrad else (B * g.Ho * g.Wo, g.Co, g.taps * g.Ci)
        hint = conv_hint(kind, plan, t, B, g, w, out, ep) if PROFILE is not None else None
        if dgrad:
            ep = dict(ep, transposed=0 if g.plain else 1)
        igemm(dtype, M, N, K, t, t.stride(0), w, K, out, out.stride(0), conv=None if g.plain else _geom_tuple(g, dgrad), hint=hint, **ep)
    return out


def conv_fwd(dtype, x, B, g, wf, out=None, **ep):
    """NHWC conv forward: x [B*Hi*Wi, Ci] (row stride = x.stride(0)), wf packed [Co][taps][Ci]"""
    if out is None:
        out = torch.empty((B * g.Ho * g.Wo, g.Co), device=x.device, dtype=TORCH_DTYPE[dtype])
    return _conv('fwd', dtype, x, B, g, wf, out, ep)


def conv_dgrad(dtype, dy, B, g, wb, out=None, **ep):
    """dx [B*Hi*Wi, Ci] = conv_transpose(dy [B*Ho*Wo, Co]); wb packed [Ci][taps][Co] (BN scale folded in)"""
    if out is None:
        out = torch.empty((B * g.Hi * g.Wi, g.Ci), device=dy.device, dtype=TORCH_DTYPE[dtype])
    return _conv('dgrad', dtype, dy, B, g, wb, out, ep)


# The input gradient of a stride-s 1x1 projection (pad 0: the skip path of layer2's / layer3's block 0) is non-zero only on the pixels the
# projection read - every s-th row and column, a quarter of the map at s = 2 - and there it is the plain GEMM dY W over the projection's
# OUTPUT grid.  proj_dgrad computes just that, [B Ho Wo, Ci]; the one consumer - conv1's input gradient, which takes it as its residual -
# reads it through SedtIgemm.rmap.  The dense form (a transposed gather over the input grid: three of four GEMM rows multiply zeros, three
# quarters of the result are zeros written to HBM and read back) stays behind the developer attribute for same-build A/Bs and as the
# reference path of tests/test_proj_compact_gpu.py.
PROJ_COMPACT = _dev_env('SEDT_PROJ_COMPACT', '1') != '0'


def proj_compact_ok(g):
    return PROJ_COMPACT and g.KH == 1 and g.KW == 1 and (g.sh > 1 or g.sw > 1) and g.ph == 0 and g.pw == 0 and g.dh == 1 and g.dw == 1


def proj_dgrad(dtype, dy, B, g, wb):
    """(side, extra epilogue arguments of the GEMM that takes it as ``res``): the input gradient of the 1x1 projection ``g`` from
    dy [B*Ho*Wo, Co] and wb, the packed dgrad operand [Ci][1][Co]"""
    if not proj_compact_ok(g):
        side = conv_dgrad(dtype, dy, B, g, wb)
        return side, dict(ldr=side.stride(0))
    M = B * g.Ho * g.Wo
    side = torch.empty((M, g.Ci), device=dy.device, dtype=TORCH_DTYPE[dtype])
    if L.LAUNCH_LOG is not None:
        L.LAUNCH_LOG['proj_dgrad:%dx%dx%d' % (M, g.Ci, g.Co)] += 1
    igemm(dtype, M, g.Ci, g.Co, dy, dy.stride(0), wb, g.Co, side, side.stride(0))
    return side, dict(ldr=side.stride(0), res_map=(g.Hi, g.Wi, g.sh, g.sw))


def _fused_bias_ok(dtype, dy, x, g):
    """envelope of the bf16 LDS-DMA wgrad kernel (csrc/wgrad3.hip / wgrad4.hip, envelope in wgrad_lds_envelope): only there the bias gradient rides along"""
    return (dtype == BF16 and L.load() is not None and g.Co % 8 == 0 and (g.taps * g.Ci) % 8 == 0 and dy.stride(0) % 8 == 0
            and x.stride(0) % 8 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and g.Ci % 8 == 0)


class ReduceBatch(object):
    """collects the split-K reductions of several wgrads and issues them as ONE launch (flush); keeps the slabs alive.
    Inside a runtime.async_wgrad() scope the wgrad GEMMs themselves are deferred too: flush() then issues all of them
    plus the reduction as ONE block on the side stream (one fork per layer instead of one per GEMM)."""

    def __init__(self, shared=False):
        """shared: this batch outlives the backward of the layer that fills it (WgradShare): it then holds NO reference to the gradient
        tensors - autograd's AccumulateGrad steals a gradient whose reference count is 1 and CLONES one that is still referenced, and a
        clone taken before the deferred launch has written the tensor would be garbage"""
        self.jobs, self.keep, self.deferred, self.operands = [], [], [], []
        self.group, self.group_dtype = [], None
        self.shared = shared
        self.expect = []            # shared: (parameter, data_ptr of the gradient tensor handed to autograd) - checked at the final flush

    def add_gemm(self, dtype, args, shape, code=None):
        """a weight-gradient GEMM to be issued with the others of this batch in one grouped launch.  code: the dtype code the entry point
        gets when it is not gemm_dtype(dtype) - the fast bf16x3 problems are bf16 problems on split operands"""
        self.group.append((args, shape, L.gemm_dtype(dtype) if code is None else code))
        self.group_dtype = dtype

    def _launch_group(self):
        if not self.group:
            return
        lib = L.load()
        if PROFILE is not None:                       # bench.py replays every GEMM on its own for the per-launch timing
            for a, shape, code in self.group:
                L.check(lib.sedt_igemm(C.byref(a), code, L.stream_ptr()), 'sedt_igemm')
                PROFILE.append((a, code, shape, (list(self.keep), list(self.operands)), 'wgrad_group'))
        else:
            i = 0
            while i < len(self.group):                # runs of equal dtype code: one grouped launch each
                j = i
                while j < len(self.group) and self.group[j][2] == self.group[i][2]:
                    j += 1
                arr = (L.SedtIgemm * (j - i))(*[g[0] for g in self.group[i:j]])
                L.check(lib.sedt_wgrad_group(arr, j - i, self.group[i][2], L.stream_ptr()), 'wgrad_group')
                i = j
        self.group = []

    def defer(self, body, operands):
        self.deferred.append(body)
        self.operands.extend(t for t in operands if t is not None)

    def add(self, slab, sk, R, taps, Ci, rowscale, out, cs, bias_out, cs_splitk=0):
        j = L.SedtReduceJob()
        j.slab, j.out, j.splitk, j.R, j.taps, j.Ci = slab.data_ptr(), out.data_ptr(), sk, R, taps, Ci
        j.cs_splitk = cs_splitk
        j.rowscale = rowscale.data_ptr() if rowscale is not None else None
        j.colsum_slab = cs.data_ptr() if cs is not None else None
        j.bias_out = bias_out.data_ptr() if (cs is not None and bias_out is not None) else None
        self.jobs.append(j)
        self.keep.append((slab, cs, rowscale, None, None) if self.shared else (slab, cs, rowscale, out, bias_out))
        if len(self.jobs) == L.MAX_REDUCE_JOBS and not _co['on'] and not self.shared:
            self._launch_group()
            self._launch()

    def add_colsum(self, partial, nrows, ncols, out):
        """out[c] = sum_r partial[r][c] in the same launch as the split-K reductions (LayerNorm gamma/beta partials)"""
        j = L.SedtReduceJob()
        j.colsum_slab, j.bias_out, j.splitk, j.R, j.taps, j.Ci = partial.data_ptr(), out.data_ptr(), nrows, ncols, 1, 0
        self.jobs.append(j)
        self.keep.append((partial, None, None, None if self.shared else out, None))

    def _launch(self):
        for i in range(0, len(self.jobs), L.MAX_REDUCE_JOBS):
            chunk = self.jobs[i:i + L.MAX_REDUCE_JOBS]
            arr = (L.SedtReduceJob * len(chunk))(*chunk)
            pf = None
            if self.prefetch is not None and RED_PREFETCH and i + L.MAX_REDUCE_JOBS >= len(self.jobs):      # (the last launch of the batch)
                pf = L.prefetch_arg(self.prefetch)
            L.check(L.load().sedt_multi_wgrad_reduce(arr, len(chunk), pf, L.stream_ptr()), 'multi_wgrad_reduce')
        self.jobs, self.keep = [], []

    prefetch = None

    def collect(self):
        """shared batches, at the end of a layer's backward: run the layer's deferred bodies NOW - they allocate the split-K slabs and
        build the argument blocks, nothing is launched (bf16x3: the operand splits are) - so that no closure keeps the gradient tensors
        referenced when the layer returns them to autograd.  The launches happen in the stack's final flush."""
        for body in self.deferred:
            body()
        self.deferred = []

    def flush(self, prefetch=None):
        """prefetch: up to three tensors (weights) the launch AFTER this batch's reduce launch will stream: that launch touches them"""
        from . import runtime
        self.prefetch = prefetch
        if _co['on'] and not runtime.async_wgrad_on():
            for body in self.deferred:              # allocate slabs / build the argument blocks; the GEMMs are not launched:
                body()                              # they ride along with later launches of the dgrad chain
            self.deferred = []
            if self.group_dtype in (None, BF16):
                # (not the gradient tensors themselves: an extra reference would make autograd clone them before they are written)
                POOL.push(self.group, BF16, self.jobs, [k[:3] for k in self.keep], self.operands)
                self.group, self.jobs, self.keep, self.operands = [], [], [], []
                return
        if self.deferred:
            with runtime.side(*self.operands):      # (the current stream itself unless runtime.async_wgrad is on)
                for body in self.deferred:
                    body()
                self._launch_group()
                self._launch()
            self.deferred, self.operands = [], []
        else:
            self._launch_group()
            self._launch()


DEFER_LAYER_WGRADS = _dev_env('SEDT_DEFER_LAYER_WGRADS', '1') != '0'
_defer = {'on': False}


class defer_layer_wgrads(object):
    """scope (the captured steppers' bodies): the weight gradients of ALL layers of a transformer stack are issued as ONE grouped GEMM
    launch + ONE reduce launch when the backward leaves the stack, instead of two launches per layer (three decoder layers at M = 704
    rows: 6 latency-bound launches -> 2; six per-op encoder layers of the B = 32 configurations: 12 -> 2).  Only inside a stepper: the
    gradients a layer returns are written later in stream order, which a consumer that reads them at AccumulateGrad time (torch DDP's
    hooks on the eager path) must not see."""

    def __init__(self, enable=True):
        self.enable = bool(enable) and DEFER_LAYER_WGRADS

    def __enter__(self):
        self.prev = _defer['on']
        _defer['on'] = self.enable
        return self

    def __exit__(self, *exc):
        _defer['on'] = self.prev
        return False


class WgradShare(object):
    """the ReduceBatch shared by the layers of one stack in one forward / backward pass (functional.EncoderLayerFn / DecoderLayerFn,
    cfg['wg_share']); None-safe helpers keep the layers' code paths identical with and without it"""

    def __init__(self):
        self.rb = None
        self.mark = 0               # rb.expect[:mark]: gradients of layers whose AccumulateGrad nodes have run by now

    @staticmethod
    def make():
        return WgradShare() if (_defer['on'] and not _co['on']) else None

    def batch(self):
        if self.rb is None:
            self.rb = ReduceBatch(shared=True)
        return self.rb

    def layer_done(self, last, prefetch=None):
        """end of a layer's backward; last: this is the last layer of the stack to run (layer 0)"""
        rb = self.rb
        if rb is None:
            return
        rb.collect()
        if last:
            for param, ptr in rb.expect[:self.mark]:          # (this layer's own gradients reach AccumulateGrad after it returns)
                g = param.grad                                # None: torch.autograd.grad captured the tensor itself (the DP segments)
                if g is not None and g.data_ptr() != ptr:
                    raise RuntimeError('a deferred weight gradient was cloned or accumulated by autograd before it was written: '
                                       'defer_layer_wgrads needs parameters whose .grad is None when the backward starts')
            rb.expect = []
            rb.flush(prefetch=prefetch)
            self.rb, self.mark = None, 0
        else:
            self.mark = len(rb.expect)


GRAD_SINK = None      # {parameter data_ptr: f32 view}: where the weight gradient of that parameter is to be written (grad_sink())


class grad_sink(object):
    """inside the scope, weight-gradient kernels called with ``param=`` write into the view registered for that parameter - the data-
    parallel steppers register the parameters' slots in the flat gradient buffer (FusedAdamW.flat_views), which spares the
    130 MB gather pass for the tensors that are produced this way"""

    def __init__(self, views):
        self.views = dict(views) if views else None      # own copy: a slot is handed out ONCE per scope (see _sink)

    def __enter__(self):
        global GRAD_SINK
        self.prev, GRAD_SINK = GRAD_SINK, self.views
        return self

    def __exit__(self, *a):
        global GRAD_SINK
        GRAD_SINK = self.prev
        return False


def _sink(param, shape):
    if GRAD_SINK is None or param is None:
        return None
    # pop: a parameter that receives a second contribution in the same backward (a module applied twice) gets an ordinary
    # buffer for it - autograd then sums the two into a new tensor and the gather pass copies that one
    v = GRAD_SINK.pop(param.data_ptr(), None)
    return v.view(shape) if v is not None and v.numel() == int(np.prod(shape)) else None


def _x3_wgrad_ok(dy, x, g, B):
    """envelope of the LDS-DMA weight-gradient kernels (wgrad_lds_envelope + wgrad3_conv_ok, csrc/wgrad3.hip) on the split operands"""
    if not X3_FAST or dy.dtype != torch.float32 or x.dtype != torch.float32:
        return False
    Co, Ci = g.Co, g.Ci
    if Co % 8 or Ci % 8 or dy.stride(0) % 4 or x.stride(0) % 4 or dy.data_ptr() % 16 or x.data_ptr() % 16:
        return False
    if not g.plain and ((64 % g.Wo) != 0 or g.Ho * g.Wo < 64 or g.Ho < 64 // g.Wo):
        return False
    return B * g.Ho * g.Wo * 3 * Co * 2 < (1 << 31) and B * g.Hi * g.Wi * 3 * Ci * 2 < (1 << 31)


def wgrad(dtype, dy, x, B, g, rowscale=None, out=None, bias_out=None, batch=None, param=None):
    """dW (Co, Ci, KH, KW) f32 = sum over pixels dy[pix][co] * gather(x)[pix][tap][ci] (* rowscale[co]).
    bias_out (f32 [Co]): also receives sum over pixels of dy (fused into the wgrad kernel when it can, else a colsum).
    batch: a ReduceBatch - the split-K reduction is deferred until batch.flush() (the result is valid only then).
    param: the parameter this is the gradient of - with a grad_sink() active the result lands in the registered view"""
    from . import runtime
    lib = L.load()
    Mo, No, Kp = g.Co, g.taps * g.Ci, B * g.Ho * g.Wo
    sk = lib.sedt_igemm_splitk(Mo, No, Kp, dtype)
    own_out = False                     # allocated here (not the caller's buffer, not a slot of the flat gradient buffer)
    if out is None:
        out = _sink(param, (g.Co, g.Ci, g.KH, g.KW))
        if out is None:
            out = torch.empty((g.Co, g.Ci, g.KH, g.KW), device=dy.device, dtype=torch.float32)
            own_out = True

    def body():
        conv = None if g.plain else _geom_tuple(g)
        if dtype == F32 and L.GEMM_X3 and _x3_wgrad_ok(dy, x, g, B):
            # fast bf16x3 (csrc/split3.hip): both operands split once, hi hi + lo hi as ONE problem over [dY_hi | dY_lo], hi lo as a second,
            # 3 sk slabs of [Co][taps Ci] for the reduce launch
            sk3 = max(1, lib.sedt_igemm_splitk(2 * Mo, No, Kp, BF16))
            rows_x = B * g.Hi * g.Wi
            dy3, x3 = _split3([(dy, 0, Kp, Mo, dy.stride(0), 0), (x, 0, rows_x, g.Ci, x.stride(0), 0)])
            slab = torch.empty((3 * sk3, Mo, No), device=dy.device, dtype=torch.float32)
            cs = torch.empty((2 * sk3, Mo), device=dy.device, dtype=torch.float32) if bias_out is not None else None
            a1 = igemm_args(2 * Mo, No, Kp, dy3, 2 * Mo, x3, 2 * g.Ci, slab, No, trans=1, conv=conv, out_f32=1, splitk=sk3, slab=slab,
                            colsum_out=cs)
            x3lo, slab2 = x3[:, g.Ci:2 * g.Ci], slab[2 * sk3:]
            a2 = igemm_args(Mo, No, Kp, dy3, 2 * Mo, x3lo, 2 * g.Ci, slab2, No, trans=1, conv=conv, out_f32=1, splitk=sk3, slab=slab2)
            tb = batch if batch is not None else ReduceBatch()
            tb.add_gemm(dtype, a1, (2 * Mo, No, Kp, 1, 0 if conv is None else 1), code=BF16)
            tb.add_gemm(dtype, a2, (Mo, No, Kp, 1, 0 if conv is None else 1), code=BF16)
            tb.add(slab, 3 * sk3, Mo, g.taps, g.Ci, rowscale, out, cs, bias_out, cs_splitk=2 * sk3)
            tb.keep.append((dy3, x3, None, None, None))
            if batch is None:
                tb._launch_group()
                tb._launch()
            return
        slab = torch.empty((sk, Mo, No), device=dy.device, dtype=torch.float32)
        fused = bias_out is not None and _fused_bias_ok(dtype, dy, x, g)
        cs = torch.empty((sk, Mo), device=dy.device, dtype=torch.float32) if fused else None
        if batch is not None:
            batch.add_gemm(dtype, igemm_args(Mo, No, Kp, dy, dy.stride(0), x, x.stride(0), slab, No, trans=1, conv=conv,
                                             out_f32=1, splitk=sk, slab=slab, colsum_out=cs),
                           (Mo, No, Kp, 1, 0 if conv is None else 1))
            batch.add(slab, sk, Mo, g.taps, g.Ci, rowscale, out, cs, bias_out if fused else None)
        else:
            igemm(dtype, Mo, No, Kp, dy, dy.stride(0), x, x.stride(0), slab, No, trans=1, conv=conv, out_f32=1, splitk=sk,
                  slab=slab, colsum_out=cs)
            L.check(lib.sedt_wgrad_reduce_bias(_p(slab), sk, Mo, g.taps, g.Ci, _p(rowscale), _p(out), _p(cs),
                                               _p(bias_out) if fused else None, L.stream_ptr()), 'wgrad_reduce')
        if bias_out is not None and not fused:
            colsum(dtype, dy, out=bias_out)

    if batch is not None:
        batch.defer(body, (dy, x, rowscale))              # issued by batch.flush(): one grouped launch for the whole layer
        if batch.shared and param is not None and own_out and tuple(param.shape) == tuple(out.shape[:param.dim()]):
            batch.expect.append((param, out.data_ptr()))      # (checked at the stack's final flush: autograd must have STOLEN this tensor)
    else:
        with runtime.side(dy, x, rowscale):               # off the dgrad critical path when runtime.async_wgrad is on
            body()
    return out


def linear_wgrad(dtype, dy, x, out=None, bias_out=None, batch=None, param=None):
    """dW [N,K] f32 = dy[M,N]^T @ x[M,K]; bias_out f32 [N] optionally receives the column sums of dy"""
    N, K = dy.shape[1], x.shape[1]
    g = ConvGeom(1, 1, K, N)
    return wgrad(dtype, dy, x, dy.shape[0], g, out=out.view(N, K, 1, 1) if out is not None else None,
                 bias_out=bias_out, batch=batch, param=param).view(N, K)


def colsum(dtype, x, out=None):
    """column sums of x[rows, cols] (compute dtype or f32) -> f32[cols]"""
    lib = L.load()
    rows, cols = x.shape
    if out is None:
        out = torch.empty((cols,), device=x.device, dtype=torch.float32)
    nb = lib.sedt_colsum_scratch(rows, cols)
    scratch = torch.empty((max(nb // 4, 1),), device=x.device, dtype=torch.float32)
    L.check(lib.sedt_colsum(_p(x), x.stride(0), rows, cols, int(x.dtype == torch.float32), dtype, _p(out), _p(scratch),
                            nb, L.stream_ptr()), 'colsum')
    return out


def dropout_grad(dtype, g, p, seed, seed_ptr=None, out=None):
    rows, cols = g.shape
    if out is None:
        out = torch.empty((rows, cols), device=g.device, dtype=g.dtype)
    L.check(L.load().sedt_dropout_grad(_p(g), g.stride(0), _p(out), out.stride(0), rows, cols, p, seed & 0xffffffff,
                                       _p(seed_ptr), dtype, L.stream_ptr()), 'dropout_grad')
    return out


def add(dtype, a, b, b_mod=0, out=None):
    rows, cols = a.shape
    if out is None:
        out = torch.empty_like(a)
    L.check(L.load().sedt_add(_p(a), _p(b), _p(out), rows, cols, b_mod, dtype, L.stream_ptr()), 'add')
    return out


def add_n(dtype, tensors, out=None):
    """sum of equally shaped contiguous tensors of the compute dtype: one launch for up to 8 (sedt_add_n has 8 pointer slots), more are
    folded in groups of 8 with the running sum as the first source of the next group (--dec_layers >= 5 hands over 2 shares per
    layer of the query-position gradient, functional.DecoderLayerFn)"""
    _dev_check(*tensors)
    tensors = list(tensors)
    n = len(tensors)
    assert n >= 1 and all(t.shape == tensors[0].shape and t.dtype == TORCH_DTYPE[dtype] and t.is_contiguous() for t in tensors)
    while n > 8:
        tensors = [add_n(dtype, tensors[:8])] + tensors[8:]
        n = len(tensors)
    if out is None:
        out = torch.empty_like(tensors[0])
    arr = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    L.check(L.load().sedt_add_n(arr, n, _p(out), tensors[0].numel(), dtype, L.stream_ptr()), 'add_n')
    return out


def cast(x, out_dtype):
    """f32 <-> compute dtype"""
    code = {torch.float32: F32, torch.bfloat16: BF16}
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=TORCH_DTYPE[out_dtype])
    L.check(L.load().sedt_cast(_p(x), code[x.dtype], _p(out), out_dtype, x.numel(), L.stream_ptr()), 'cast')
    return out


def relu_mask(dtype, g, y):
    g, y = g.contiguous(), y.contiguous()
    out = torch.empty_like(g)
    L.check(L.load().sedt_relu_mask(_p(g), _p(y), _p(out), g.numel(), dtype, L.stream_ptr()), 'relu_mask')
    return out


def copy2d(jobs):
    """jobs: (src tensor view start, dst tensor view start, outer, inner_bytes, src_stride_bytes, dst_stride_bytes) given as
    (src_ptr, dst_ptr, outer, inner, sstride, dstride) integers; up to 8 per launch (sedt_copy2d)"""
    for base in range(0, len(jobs), 8):
        chunk = jobs[base:base + 8]
        arr = (L.SedtCopyJob * len(chunk))()
        for n, (sp, dp, outer, inner, ss, ds) in enumerate(chunk):
            arr[n].src, arr[n].dst, arr[n].outer, arr[n].inner, arr[n].src_stride, arr[n].dst_stride = sp, dp, outer, inner, ss, ds
        L.check(L.load().sedt_copy2d(arr, len(chunk), L.stream_ptr()), 'copy2d')


def spsedt_dec_in(dtype, patch, query, B, Q, P, qpp, train, ratio=0.0, keep=None, seed=0, seed_ptr=None):
    """SP-SEDT decoder input [B*Q, D] from the patch queries [B*P, D] and the query embedding rows [Q, D] (f32); returns (dec_in, keep
    [Q, B] f32 or None) - reference spsedt.py:48-69 in one launch"""
    D = patch.shape[1]
    assert patch.is_contiguous() and patch.shape[0] == B * P and query.dtype == torch.float32 and query.is_contiguous() and query.shape == (Q, D)
    out = torch.empty((B * Q, D), device=patch.device, dtype=patch.dtype)
    keep_out = torch.empty((Q, B), device=patch.device, dtype=torch.float32) if train else None
    if keep is not None:
        keep = keep.to(device=patch.device, dtype=torch.float32).reshape(Q, B).contiguous()
    L.check(L.load().sedt_spsedt_dec_in(_p(patch), _p(query), _p(keep), _p(keep_out), _p(out), B, Q, P, qpp, D, int(train),
                                        float(ratio), seed & 0xffffffff, _p(seed_ptr), dtype, L.stream_ptr()), 'spsedt_dec_in')
    return out, keep_out


def spsedt_dec_in_bwd(dtype, g, keep, B, Q, P, qpp, train, need_patch=True):
    D = g.shape[1]
    g = g.contiguous()
    d_patch = torch.empty((B * P, D), device=g.device, dtype=g.dtype) if need_patch else None
    d_query = torch.empty((Q, D), device=g.device, dtype=torch.float32)
    L.check(L.load().sedt_spsedt_dec_in_bwd(_p(g), _p(keep), _p(d_patch), _p(d_query), B, Q, P, qpp, D, int(train), dtype, L.stream_ptr()),
            'spsedt_dec_in_bwd')
    return d_patch, d_query


def gelu_fwd(dtype, h, p=0.0, seed=0, seed_ptr=None):
    """a = dropout(gelu(h)) in one launch (reference transformer.py:423-431 'gelu' + the FFN dropout); h: the linear1 output"""
    h = h.contiguous()
    a = torch.empty_like(h)
    L.check(L.load().sedt_gelu_fwd(_p(h), _p(a), h.numel(), p, seed & 0xffffffff, _p(seed_ptr), dtype, L.stream_ptr()), 'gelu_fwd')
    return a


def gelu_bwd(dtype, g, h, p=0.0, seed=0, seed_ptr=None):
    """gradient wrt the pre-activation h of a = dropout(gelu(h)), given the gradient wrt a"""
    g, h = g.contiguous(), h.contiguous()
    out = torch.empty_like(g)
    L.check(L.load().sedt_gelu_bwd(_p(g), _p(h), _p(out), g.numel(), p, seed & 0xffffffff, _p(seed_ptr), dtype, L.stream_ptr()), 'gelu_bwd')
    return out


def sigmoid_grad(g, s):
    g, s = g.contiguous(), s.contiguous()
    out = torch.empty_like(g)
    L.check(L.load().sedt_sigmoid_grad(_p(g), _p(s), _p(out), g.numel(), L.stream_ptr()), 'sigmoid_grad')
    return out


def layernorm_fwd(dtype, x, gamma, beta, add_t=None, out=None):
    """out = (y, mean, rstd) preallocated (contiguous row ranges of larger buffers are fine)"""
    rows, D = x.shape
    assert x.is_contiguous() and (add_t is None or (add_t.is_contiguous() and add_t.shape == x.shape)), 'layernorm_fwd: contiguous rows'
    y2 = torch.empty_like(x) if add_t is not None else None
    if out is not None:
        y, mean, rstd = out
    else:
        y = torch.empty_like(x)
        mean = torch.empty((rows,), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
    assert y.is_contiguous() and y.shape == x.shape, 'layernorm_fwd: contiguous rows'
    L.check(L.load().sedt_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(add_t), _p(y), _p(y2), _p(mean), _p(rstd), rows, D,
                                        dtype, L.stream_ptr()), 'layernorm_fwd')
    return y, y2, mean, rstd


def layernorm_bwd(dtype, dy, x, gamma, mean, rstd, dy2=None, dres=None, want_param_grads=True, batch=None, drop=None, dres2=None):
    """batch (a ReduceBatch): the gamma/beta reduction - which only feeds the optimizer - is deferred to batch.flush() and
    rides in the layer's split-K reduction launch.
    drop = (p, seed, seed_ptr): also returns dx passed through that dropout mask (the gradient entering the sub-layer whose
    dropped output fed this LayerNorm) as a 4th result - one launch instead of layernorm_bwd + dropout_grad"""
    lib = L.load()
    rows, D = x.shape
    assert all(t is None or (t.is_contiguous() and t.shape == x.shape) for t in (dy, x, dy2, dres, dres2)), 'layernorm_bwd: contiguous rows'
    dx = torch.empty_like(x)
    dg = torch.empty((D,), device=x.device, dtype=torch.float32) if want_param_grads else None
    db = torch.empty((D,), device=x.device, dtype=torch.float32) if want_param_grads else None
    nb = lib.sedt_layernorm_bwd_scratch(rows, D)
    scratch = torch.empty((nb // 4,), device=x.device, dtype=torch.float32)
    dxd, p_, seed_, sp_ = None, 0.0, 0, None
    if drop is not None and drop[0] > 0:
        p_, seed_, sp_ = drop
        if _dev_env('SEDT_LN_DROP_FUSE', '1') == '0':        # A/B switch: separate dropout_grad launch
            dx, dg, db = layernorm_bwd(dtype, dy, x, gamma, mean, rstd, dy2, dres, want_param_grads, batch, dres2=dres2)
            return dx, dg, db, dropout_grad(dtype, dx, p_, seed_, sp_)
        dxd = torch.empty_like(x)
    deferred = want_param_grads and batch is not None
    L.check(lib.sedt_layernorm_bwd_drop(_p(dy), _p(dy2), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dres2), _p(dx),
                                        None if deferred else _p(dg), None if deferred else _p(db), _p(scratch), nb, rows, D,
                                        _p(dxd), p_, seed_ & 0xffffffff, _p(sp_), dtype, L.stream_ptr()), 'layernorm_bwd')
    if deferred:
        # the gamma/beta reduction of the per-workgroup partials rides in batch.flush() as one more job
        dgb = torch.empty((2 * D,), device=x.device, dtype=torch.float32)
        batch.add_colsum(scratch, nb // (2 * D * 4), 2 * D, dgb)
        dg, db = dgb[:D], dgb[D:]
    if drop is not None:
        return dx, dg, db, (dxd if dxd is not None else dx)
    return dx, dg, db


def attention_instance(dtype, q, k, v, o, Lq, Lk, amask=None, drop_p=0.0, do=None, dq=None, dk=None, dv=None):
    """the kernel instance attention_fwd (do is None) or attention_bwd launches for these tensors ('' if the call would be refused):
    sedt_attention_describe, nothing is launched"""
    def pl(t):
        return (_p(t), t.stride(0)) if t is not None else (None, 0)
    buf = C.create_string_buffer(96)
    args = pl(q) + pl(k) + pl(v) + pl(o) + pl(do) + pl(dq) + pl(dk) + pl(dv)
    L.load().sedt_attention_describe(*args, int(amask is not None), Lq, Lk, drop_p, dtype, int(do is not None), buf, 96)
    return buf.value.decode()


def attention_fwd(dtype, q, k, v, B, H, Lq, Lk, kpm=None, amask=None, drop_p=0.0, seed=0, seed_ptr=None, out=None):
    """q [B*Lq, >=H*32] / k, v [B*Lk, ...] row-strided views; returns (o [B*Lq, H*32], lse [B,H,Lq])"""
    if out is None:
        out = torch.empty((B * Lq, H * 32), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, H, Lq), device=q.device, dtype=torch.float32)
    if L.LAUNCH_LOG is not None:     # (lib.launch_log(): which kernel instance the dispatcher picks for this problem)
        L.LAUNCH_LOG['attention:' + attention_instance(dtype, q, k, v, out, Lq, Lk, amask, drop_p)] += 1
    L.check(L.load().sedt_attention_fwd(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0),
                                        _p(lse), _p(kpm), _p(amask), B, H, Lq, Lk, drop_p, seed & 0xffffffff, _p(seed_ptr),
                                        dtype, L.stream_ptr()), 'attention_fwd')
    return out, lse


def attention_bwd(dtype, q, k, v, o, do, lse, B, H, Lq, Lk, dq, dk, dv, kpm=None, amask=None, drop_p=0.0, seed=0,
                  seed_ptr=None):
    if L.LAUNCH_LOG is not None:
        L.LAUNCH_LOG['attention:' + attention_instance(dtype, q, k, v, o, Lq, Lk, amask, drop_p, do, dq, dk, dv)] += 1
    L.check(L.load().sedt_attention_bwd(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                        _p(do), do.stride(0), _p(lse), _p(kpm), _p(amask), _p(dq), dq.stride(0), _p(dk),
                                        dk.stride(0), _p(dv), dv.stride(0), B, H, Lq, Lk, drop_p, seed & 0xffffffff,
                                        _p(seed_ptr), dtype, L.stream_ptr()), 'attention_bwd')
    return dq, dk, dv


NO_RIDE = _dev_env('SEDT_CO_NORIDE', '0') == '1'      # experiment: park all wgrads until the end of the backward, no riders
CONV3_DIRECT = _dev_env('SEDT_CONV3_DIRECT', '1') != '0'   # direct 3x3 kernel for the layer1 conv2 geometry (conv3x3_c64.hip)
STEM_DIRECT = _dev_env('SEDT_STEM_DIRECT', '1') != '0'     # one-launch stem forward / backward (stem.hip)
# The pre-norm encoder layer on the x-stationary slab kernels (csrc/enc_slab.hip: two launches per layer instead of seven; a workgroup
# owns 32 tokens, only weights stream).  Default in the bf16 mode; SLAB_ENC = False (tests, A/B) keeps the per-op chain.
SLAB_ENC = _dev_env('SEDT_SLAB_ENC', '1') != '0'
SLAB_ENC_BWD = _dev_env('SEDT_SLAB_ENC_BWD', '1') != '0'      # the input-gradient chain of those layers on the slab kernels as well


SLAB_MIN_WGS = 192      # slabs (= workgroups) below which the per-op chain fills the chip better (B = 32: 128 slabs; same-box A/B on C3)
SLAB_MAX_WGS = 320      # ... and above which it wins again: every slab streams the layer's 3.4 MB of weights, the per-op GEMMs amortise them
                        # over 64-128 rows per tile (C4, B = 200: 800 slabs, 17.0 ms with the slab encoder against 16.65 ms without)


def encoder_slab_ok(dtype, D, H, S, FF, amask, B=None):
    return bool(SLAB_ENC and dtype == BF16 and amask is None and (B is None or SLAB_MIN_WGS <= B * ((S + 31) // 32) <= SLAB_MAX_WGS)
                and L.load().sedt_encoder_slab_ok(D, H, S, FF, dtype))


ENC_PREFETCH = _dev_env('SEDT_ENC_PREFETCH', '1') != '0'
RED_PREFETCH = _dev_env('SEDT_RED_PREFETCH', '1') != '0'


class BackwardChain(object):
    """what the backward that runs AFTER a node's own will stream first, handed from node to node while one forward is traced (backward
    order is the reverse of forward order): a node's forward reads ``top`` - the operands of the node before it, whose backward follows
    its own - keeps it on its autograd ctx, and leaves its own operands in ``top`` for the node after it.  The reduce launch that closes
    the node's backward then touches those operands (SedtPrefetch) so that they are L2-resident when the next backward streams them.
    One chain object per model forward (sedt.backbone.ResNet50Body.forward, sedt.transformer.Transformer.forward): no module- or
    process-level state, nothing survives the forward that created it"""
    __slots__ = ('top',)

    def __init__(self):
        self.top = None


def encoder_qkv_fwd(x, pos, gamma, beta, w_in_frag, b_in, B, S, train=True, prefetch=None):
    """xn = LayerNorm1(x); q | k = (xn + pos) Wqk^T + b; v = xn Wv^T + b.  x, pos [B*S, 256] bf16 contiguous; w_in_frag = the
    fragment-major in_proj_weight (packing.lookup_frag).  Returns (qk [B*S, 512], v [B*S, 256], (xn, xnp, mean, rstd) or None)"""
    _dev_check(x, pos, w_in_frag)
    M, D = x.shape
    assert x.is_contiguous() and pos.is_contiguous() and pos.shape == x.shape and M == B * S and D == 256 and x.dtype == torch.bfloat16
    qk = torch.empty((M, 2 * D), device=x.device, dtype=x.dtype)
    v = torch.empty((M, D), device=x.device, dtype=x.dtype)
    by = None
    if train:
        by = (torch.empty_like(x), torch.empty_like(x), torch.empty((M,), device=x.device, dtype=torch.float32),
              torch.empty((M,), device=x.device, dtype=torch.float32))
    s = by if by is not None else (None,) * 4
    # the next launch's weights: touched by this one so that they are L2-resident when it streams them
    pf = L.prefetch_arg(prefetch) if (prefetch and ENC_PREFETCH) else None
    L.check(L.load().sedt_encoder_qkv_fwd(_p(x), _p(pos), _p(gamma), _p(beta), _p(w_in_frag), _p(b_in), _p(qk), _p(v), _p(s[0]), _p(s[1]),
                                          _p(s[2]), _p(s[3]), B, S, pf, L.stream_ptr()), 'encoder_qkv_fwd')
    return qk, v, by


def encoder_attn_ffn_fwd(x, qk, v, kpm, w_o_frag, b_o, gamma2, beta2, w1_frag, b1, w2_frag, b2, B, S, FF, drop_p=0.0, seeds=(0, 0, 0, 0),
                         seed_ptr=None, train=True):
    """attention over the clip's keys + out-proj + residual + LayerNorm2 + the FFN pair + residual for every 32-token slab in ONE
    launch.  Returns (x2, (ctx, lse, x1, mean2, rstd2, x1n, h) or None); seeds = (attention, out-proj, hidden, FFN output)"""
    _dev_check(x, qk, v)
    M, D = x.shape
    assert x.is_contiguous() and qk.is_contiguous() and v.is_contiguous() and M == B * S
    x2 = torch.empty_like(x)
    by = None
    if train:
        f32 = dict(device=x.device, dtype=torch.float32)
        by = (torch.empty_like(x), torch.empty((B, 8, S), **f32), torch.empty_like(x), torch.empty((M,), **f32), torch.empty((M,), **f32),
              torch.empty_like(x), torch.empty((M, FF), device=x.device, dtype=x.dtype))
    s = by if by is not None else (None,) * 7
    L.check(L.load().sedt_encoder_attn_ffn_fwd(_p(x), _p(qk), _p(v), _p(kpm), _p(w_o_frag), _p(b_o), _p(gamma2), _p(beta2), _p(w1_frag),
                                               _p(b1), _p(w2_frag), _p(b2), _p(x2), _p(s[0]), _p(s[1]), _p(s[2]), _p(s[3]), _p(s[4]),
                                               _p(s[5]), _p(s[6]), B, S, FF, drop_p, seeds[0] & 0xffffffff, seeds[1] & 0xffffffff,
                                               seeds[2] & 0xffffffff, seeds[3] & 0xffffffff, _p(seed_ptr), L.stream_ptr()),
            'encoder_attn_ffn_fwd')
    return x2, by


# The prediction heads in ONE launch each way (csrc/heads_slab.hip).  Default in the bf16 mode.
FUSED_BNECK = int(_dev_env('SEDT_BNECK', '5'))      # 0 off, 1 layer1's identity blocks, 2 + layer2's, 3 + layer1's block 0, 4 + layer2's block 0 (forward), 5 + layer3's identity blocks


# The fused launch forms of a Bottleneck, in the order block_form tries them.  maps: input channels -> (the FUSED_BNECK level the form needs
# there, planes, map columns); ok: the library's host-side envelope call; nops: operands (3, or 4 with the projection); stride; ab_bits:
# the launch writes the sign bits of its two intermediates (a form that does not keeps the intermediates themselves when training);
# kernel: the forward kernel's name in a recording.
BlockForm = namedtuple('BlockForm', 'maps ok nops stride ab_bits kernel')
BLOCK_FORMS = {
    'bneck3': BlockForm({1024: (5, 256, 4)}, lambda lib, g, B, H, dt: lib.sedt_bneck3_ok(*g, B, H, dt), 3, 1, True, 'bneck3_kernel<false>'),
    'bneck': BlockForm({256: (1, 64, 16), 512: (2, 128, 8)}, lambda lib, g, B, H, dt: lib.sedt_bneck_ok(*g, dt), 3, 1, True,
                       'bneck_kernel<BG<{0}, {1}, {2}>, false'),
    'bneck2': BlockForm({256: (4, 128, 16)}, lambda lib, g, B, H, dt: lib.sedt_bneck2_ok(*g, dt), 4, 2, False, 'bneck2_fwd_kernel'),
    'bneck0': BlockForm({64: (3, 64, 16)}, lambda lib, g, B, H, dt: lib.sedt_bneck0_ok(*g, dt), 4, 1, True, 'bneck0_fwd_kernel'),
}


def block_form(dtype, blk, W, B=0, H=0):
    """the fused form a Bottleneck takes on a map of B clips x H rows x W columns, or None (the per-op chain): an identity block of layer1
    (256/64 on 16 columns) or layer2 (512/128 on 8) ('bneck', csrc/bneck.hip), of layer3 (1024/256 on 4) while B * ceil(H / 8) strips cover
    the chip about once ('bneck3', csrc/bneck3.hip), layer1's block 0 ('bneck0') or layer2's ('bneck2', forward only); bf16"""
    if dtype != BF16:
        return None
    g = (blk.cin, blk.planes, W, blk.stride, blk.dil, int(blk.ds))
    for name, row in BLOCK_FORMS.items():
        if blk.cin in row.maps and int(FUSED_BNECK) >= row.maps[blk.cin][0] and row.ok(L.load(), g, B, H, dtype):
            return name
    return None


def fusable_form(blk):
    """the form whose static geometry (channels, stride, dilation, projection) a block has - the one it takes when the map, the batch and
    FUSED_BNECK allow - or None: a weight plan lays the operands of these blocks out fragment-major as well"""
    for name, row in BLOCK_FORMS.items():
        if (blk.cin in row.maps and blk.planes == row.maps[blk.cin][1] and blk.stride == row.stride and blk.dil == 1
                and bool(blk.ds) == (row.nops == 4)):
            return name
    return None


def bneck_ok(dtype, blk, W, B=0, H=0):
    """the envelope of the fused identity block, either way (block_form 'bneck' / 'bneck3')"""
    return block_form(dtype, blk, W, B, H) in ('bneck', 'bneck3')


BNECK_PREFETCH = _dev_env('SEDT_BNECK_PREFETCH', '1') != '0'


def _bneck3_prefetch(nxt):
    return L.prefetch_arg(nxt) if (nxt is not None and BNECK_PREFETCH) else None


def block_fwd(form, x, B, H, W, wf, sb, train=True, want_bits=True, want_ab=False, nxt=None):
    """one Bottleneck forward in one launch.  x [B*H*W, C] bf16 contiguous; wf = the form's 3 or 4 fragment-major forward operands (conv1,
    conv2, conv3, projection); sb = their (scale, bias) pairs; nxt ('bneck3'): the next block's operands, touched by this launch so that
    they are L2-resident when that block streams them.  Returns (y, a, b, ybits, abits, bbits), y on the form's output grid.  Training:
    the sign bits of the two intermediates (all bneck_bwd needs of them; 'bneck2' has none) and, on request, those of y; want_ab: the
    intermediates themselves as well (what the weight-gradient GEMMs and the per-op backward read)"""
    _dev_check(x)
    row = BLOCK_FORMS[form]
    M, C = x.shape
    assert x.is_contiguous() and M == B * H * W and C in row.maps and W == row.maps[C][2]
    P = row.maps[C][1]
    Co, M2 = 4 * P, B * ((H - 1) // row.stride + 1) * (W // row.stride)
    dev = dict(device=x.device)
    y = torch.empty((M2, Co), dtype=torch.bfloat16, **dev)
    a = b = bits = abits = bbits = None
    if train:
        if row.ab_bits:
            abits, bbits = torch.empty((M, P // 8), dtype=torch.uint8, **dev), torch.empty((M2, P // 8), dtype=torch.uint8, **dev)
        if want_ab or not row.ab_bits:
            a, b = torch.empty((M, P), dtype=torch.bfloat16, **dev), torch.empty((M2, P), dtype=torch.bfloat16, **dev)
        if want_bits:
            bits = torch.empty((M2, Co // 8), dtype=torch.uint8, **dev)
    if PROFILE is not None:
        # (only the identity forms' records count the weights among their bytes)
        PROFILE_FUSED.append((row.kernel.format(C, P, W), 2.0 * (M * C * P + M2 * (9 * P * P + P * Co + (C * Co if row.nops == 4 else 0))),
                              M * C * 2.0 + M2 * (Co * 2.0 + (Co // 8 if bits is not None else 0))
                              + ((M + M2) * (P // 8) if abits is not None else 0) + ((M + M2) * P * 2.0 if a is not None else 0)
                              + (2.0 * (2 * C * P + 9 * P * P) if row.nops == 3 else 0)))
    planes = [_p(abits), _p(bbits), _p(bits)] if row.ab_bits else [_p(bits)]
    dims = {'bneck': (C, P, W, B, H), 'bneck3': (B, H, _bneck3_prefetch(nxt))}.get(form, (B, H))
    L.check(getattr(L.load(), 'sedt_%s_fwd' % form)(_p(x), _p(y), *[_p(w) for w in wf], *[_p(v) for pair in sb for v in pair], _p(a), _p(b),
                                                    *planes, *dims, L.stream_ptr()), form + '_fwd')
    return y, a, b, bits, abits, bbits


def bneck_fwd(x, B, H, W, wf, sb, train=True, want_bits=True, want_ab=False, nxt=None):
    """block_fwd of an identity block: 'bneck3' on 1024 channels, else 'bneck'"""
    return block_fwd('bneck3' if x.shape[1] == 1024 else 'bneck', x, B, H, W, wf, sb, train, want_bits, want_ab, nxt)


def bneck_bwd(gy, B, H, W, wt, abits, bbits, xbits, want_g=False, chain_only=False, nxt=None):
    """input gradient of the fused Bottleneck: gy [B*H*W, C] bf16 (already masked by [y > 0]); wt = the three fragment-major dgrad
    operands (conv1, conv2, conv3 order); abits / bbits from bneck_fwd; xbits = sign bits of the block input or None.
    Returns (gx, gb, ga): gb / ga [M, P] = the gradients of the two intermediates (want_g: a trainable block's weight gradients read them).
    chain_only: stop at ga (gx None; wt[0] and xbits unused) - the caller's block has another first convolution (layer1's block 0)"""
    assert gy.is_contiguous() and abits.is_contiguous() and bbits.is_contiguous() and (xbits is None or xbits.is_contiguous())
    M, C = gy.shape
    gx = None if chain_only else torch.empty_like(gy)
    gb = ga = None
    if want_g or chain_only:
        ga = torch.empty((M, C // 4), device=gy.device, dtype=torch.bfloat16)
        gb = torch.empty_like(ga) if want_g else None
    if PROFILE is not None:
        P_ = C // 4
        name = ('bneck3_kernel<true>' if C == 1024 else
                'bneck_kernel<BG<%d, %d, %d>, true, %s>' % (C, P_, W, 'true' if chain_only else 'false'))
        PROFILE_FUSED.append((name, 2.0 * M * ((1 if chain_only else 2) * C * P_ + 9 * P_ * P_),
                              M * (C * 2.0 * (1 if chain_only else 2) + C // 8 + 2 * (P_ // 8) + ((2 if want_g else 1 if chain_only else 0) * P_ * 2))
                              + 2.0 * (2 * C * P_ + 9 * P_ * P_)))
    if C == 1024:
        assert not chain_only
        L.check(L.load().sedt_bneck3_bwd(_p(gy), _p(gx), _p(wt[2]), _p(wt[1]), _p(wt[0]), _p(abits), _p(bbits), _p(xbits), _p(gb), _p(ga), B, H,
                                         _bneck3_prefetch(nxt), L.stream_ptr()), 'bneck3_bwd')
        return gx, gb, ga
    L.check(L.load().sedt_bneck_bwd(_p(gy), _p(gx), _p(wt[2]), _p(wt[1]), None if chain_only else _p(wt[0]), _p(abits), _p(bbits),
                                    None if chain_only else _p(xbits), _p(gb), _p(ga), C, C // 4, W, B, H, L.stream_ptr()), 'bneck_bwd')
    return gx, gb, ga


SLAB_HEADS = _dev_env('SEDT_SLAB_HEADS', '1') != '0'


HEADS_SLAB_MAX_ROWS = 12288     # (C4: 25,200 head rows = 788 slabs ran 0.5 % slower than the per-op heads, same-box A/B; C2 / C3 / C5: 2,000 rows, -1.2 %)


def heads_slab_ok(dtype, D, C1, CA, rows=0):
    return bool(SLAB_HEADS and dtype == BF16 and rows <= HEADS_SLAB_MAX_ROWS and L.load().sedt_heads_slab_ok(D, C1, CA, dtype))


def heads_fwd(x, wc, bc, w1f, b1, w2f, b2, w3, b3, wa, ba, Lh, B, Qp, train=True):
    """x [Lh*B*Qp, 256] bf16 contiguous; wc / w3 / wa f32 masters; w1f / w2f fragment-major.  Returns (cls [rows, C1], box [rows, 2], at
    [B, CA] or None, (h1, h2) or None)"""
    _dev_check(x, wc, w3)
    rows, D = x.shape
    assert x.is_contiguous() and rows == Lh * B * Qp and wc.is_contiguous() and w3.is_contiguous() and (wa is None or wa.is_contiguous())
    C1, CA = wc.shape[0], 0 if wa is None else wa.shape[0]
    f32 = dict(device=x.device, dtype=torch.float32)
    cls, box = torch.empty((rows, C1), **f32), torch.empty((rows, 2), **f32)
    at = torch.empty((B, CA), **f32) if CA else None
    hh = (torch.empty_like(x), torch.empty_like(x)) if train else None
    L.check(L.load().sedt_heads_fwd(_p(x), _p(wc), _p(bc), _p(w1f), _p(b1), _p(w2f), _p(b2), _p(w3), _p(b3), _p(wa), _p(ba), _p(cls), _p(box),
                                    _p(at), _p(hh[0]) if hh else None, _p(hh[1]) if hh else None, Lh, B, Qp, C1, CA, L.stream_ptr()), 'heads_fwd')
    return cls, box, at, hh


def heads_bwd(x, h1, h2, box, at, g_cls, g_box, g_at, wc, w3, wa, w2t, w1t, Lh, B, Qp):
    """returns (dhs, g_h1, g_h2, part [slabs, (C1 + CA + 2) * 257])"""
    rows, D = x.shape
    C1, CA = wc.shape[0], 0 if wa is None else wa.shape[0]
    dhs, g_h1, g_h2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    nsl = (rows + 31) // 32
    part = torch.empty((nsl, (C1 + CA + 2) * 257), device=x.device, dtype=torch.float32)
    for g in (g_cls, g_box, g_at):
        assert g is None or (g.dtype == torch.float32 and g.is_contiguous())
    L.check(L.load().sedt_heads_bwd(_p(x), _p(h1), _p(h2), _p(box), _p(at), _p(g_cls), _p(g_box), _p(g_at), _p(wc), _p(w3), _p(wa), _p(w2t),
                                    _p(w1t), _p(dhs), _p(g_h1), _p(g_h2), _p(part), Lh, B, Qp, C1, CA, L.stream_ptr()), 'heads_bwd')
    return dhs, g_h1, g_h2, part


def encoder_ffn_bwd(gx2, h, x1, mean2, rstd2, gamma2, w2t_frag, w1t_frag, wot_frag, B, S, drop_p=0.0, seeds=(0, 0), seed_ptr=None):
    """FFN backward + LayerNorm2 backward + out-proj input gradient per 32-token slab in ONE launch (csrc/enc_slab.hip).
    seeds = (FFN-output dropout, out-proj dropout).  Returns (g2, gh, gx1, g1, gctx, ln_part [slabs, 512])"""
    _dev_check(gx2, h, x1)
    M, D = gx2.shape
    FF = h.shape[1]
    assert gx2.is_contiguous() and h.is_contiguous() and x1.is_contiguous() and M == B * S
    nsl = B * ((S + 31) // 32)
    g2 = torch.empty_like(gx2) if drop_p > 0 else None
    g1 = torch.empty_like(gx2) if drop_p > 0 else None
    gh = torch.empty_like(h)
    gx1, gctx = torch.empty_like(gx2), torch.empty_like(gx2)
    part = torch.empty((nsl, 2 * D), device=gx2.device, dtype=torch.float32)
    L.check(L.load().sedt_encoder_ffn_bwd(_p(gx2), _p(h), _p(x1), _p(mean2), _p(rstd2), _p(gamma2), _p(w2t_frag), _p(w1t_frag),
                                          _p(wot_frag), _p(g2), _p(gh), _p(gx1), _p(g1), _p(gctx), _p(part), B, S, FF, drop_p,
                                          seeds[0] & 0xffffffff, seeds[1] & 0xffffffff, _p(seed_ptr), L.stream_ptr()), 'encoder_ffn_bwd')
    return (g2 if g2 is not None else gx2), gh, gx1, (g1 if g1 is not None else gx1), gctx, part


def encoder_qkv_bwd(dqk, dv, x, mean1, rstd1, gamma1, gx1, wint_frag, B, S):
    """gx = LayerNorm1'(dq|dk Wqk + dv Wv) + gx1 per slab in one launch.  Returns (gx, ln_part [slabs, 512])"""
    _dev_check(dqk, dv, x, gx1)
    M, D = x.shape
    assert dqk.is_contiguous() and dv.is_contiguous() and x.is_contiguous() and gx1.is_contiguous() and M == B * S
    gx = torch.empty_like(x)
    part = torch.empty((B * ((S + 31) // 32), 2 * D), device=x.device, dtype=torch.float32)
    L.check(L.load().sedt_encoder_qkv_bwd(_p(dqk), _p(dv), _p(x), _p(mean1), _p(rstd1), _p(gamma1), _p(gx1), _p(wint_frag), _p(gx),
                                          _p(part), B, S, L.stream_ptr()), 'encoder_qkv_bwd')
    return gx, part


def posenc(dtype, mask_u8, D):
    B, H, W = mask_u8.shape
    pos = torch.empty((B, H * W, D), device=mask_u8.device, dtype=TORCH_DTYPE[dtype])
    L.check(L.load().sedt_posenc(_p(mask_u8), _p(pos), B, H, W, D, dtype, L.stream_ptr()), 'posenc')
    return pos


def mask_resize(mask_u8, Hout, Wout):
    B, Hin, Win = mask_u8.shape
    out = torch.empty((B, Hout, Wout), device=mask_u8.device, dtype=torch.uint8)
    L.check(L.load().sedt_mask_resize(_p(mask_u8), _p(out), B, Hin, Win, Hout, Wout, L.stream_ptr()), 'mask_resize')
    return out


def bn_fold(w, b, rm, rv, scale=None, bias=None):
    n = w.numel()
    if scale is None:
        scale = torch.empty((n,), device=w.device, dtype=torch.float32)
        bias = torch.empty_like(scale)
    L.check(L.load().sedt_bn_fold(_p(w), _p(b), _p(rm), _p(rv), _p(scale), _p(bias), n, L.stream_ptr()), 'bn_fold')
    return scale, bias


def pack_conv(dtype, w, bnscale=None, want_fwd=True, want_bwd=True, wf=None, wb=None):
    """w (Co, Ci, KH, KW) or (N, K) f32 -> wf [Co][taps][Ci], wb [Ci][taps][Co]*bnscale in the compute dtype"""
    Co, Ci = w.shape[0], w.shape[1]
    taps = w.numel() // (Co * Ci)
    td = TORCH_DTYPE[dtype]
    if want_fwd and wf is None:
        wf = torch.empty((Co, taps * Ci), device=w.device, dtype=td)
    if want_bwd and wb is None:
        wb = torch.empty((Ci, taps * Co), device=w.device, dtype=td)
    L.check(L.load().sedt_pack_conv(_p(w), Co, Ci, taps, _p(bnscale), _p(wf), _p(wb), dtype, L.stream_ptr()), 'pack_conv')
    return wf, wb


def stem_prep(dtype, w0, b0, w1):
    wcat = torch.empty((64, 128), device=w1.device, dtype=TORCH_DTYPE[dtype])
    L.check(L.load().sedt_stem_prep(_p(w0), _p(b0), _p(w1), _p(wcat), dtype, L.stream_ptr()), 'stem_prep')
    return wcat


def stem_im2col(dtype, x, B, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    col = torch.empty((B * Ho * Wo, 128), device=x.device, dtype=TORCH_DTYPE[dtype])
    L.check(L.load().sedt_stem_im2col(_p(x), _p(col), B, H, W, dtype, L.stream_ptr()), 'stem_im2col')
    return col, Ho, Wo


def stem_pool_ok(dtype, W):
    """the one-launch stem (conv0 o conv1 o FrozenBN o ReLU o max-pool) exists for the bf16 mode and 64 mel bands"""
    return dtype == BF16 and W == 64 and STEM_DIRECT


def stem_pool_fwd(x, wcat, scale, bias, B, H, W, want_idx=True, want_s1=False):
    """x f32 [B][H][64] -> (pool bf16 [B*Hp*16, 64], idx uint8 or None, Hp, Wp[, s1 bf16 [B*Ho*32, 64]])"""
    Ho = (H - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, 16
    pool = torch.empty((B * Hp * Wp, 64), device=x.device, dtype=torch.bfloat16)
    idx = torch.empty((B * Hp * Wp, 64), device=x.device, dtype=torch.uint8) if want_idx else None
    s1 = torch.empty((B * Ho * 32, 64), device=x.device, dtype=torch.bfloat16) if want_s1 else None
    L.check(L.load().sedt_stem_pool_fwd(_p(x), _p(wcat), _p(scale), _p(bias), _p(pool), _p(idx), _p(s1), B, H, W, L.stream_ptr()),
            'stem_pool_fwd')
    return (pool, idx, Hp, Wp, s1) if want_s1 else (pool, idx, Hp, Wp)


def stem_pool_wgrad(x, g, idx, pool, rowscale, B, H, W):
    """G f32 [64][128] (wcat's layout) = bn_scale[co] * sum over pixels of maxpool_bwd(g)[pixel][co] * patch[pixel][k]"""
    lib = L.load()
    ns = lib.sedt_stem_pool_wgrad_slabs(B, H)
    slab = torch.empty((ns, 64, 128), device=x.device, dtype=torch.float32)
    G = torch.empty((64, 128), device=x.device, dtype=torch.float32)
    L.check(lib.sedt_stem_pool_wgrad(_p(x), _p(g), _p(idx), _p(pool), _p(slab), ns, B, H, W, L.stream_ptr()), 'stem_pool_wgrad')
    L.check(lib.sedt_wgrad_reduce_bias(_p(slab), ns, 64, 1, 128, _p(rowscale), _p(G), None, None, L.stream_ptr()), 'wgrad_reduce')
    return G


def stem_conv0_grad(G, w1):
    from . import runtime
    dw0 = torch.empty((3, 1, 1, 1), device=G.device, dtype=torch.float32)
    db0 = torch.empty((3,), device=G.device, dtype=torch.float32)
    with runtime.side(G):                       # G comes from a wgrad: stay on its stream
        L.check(L.load().sedt_stem_conv0_grad(_p(G), _p(w1), _p(dw0), _p(db0), L.stream_ptr()), 'stem_conv0_grad')
    return dw0, db0


def maxpool_fwd(dtype, x, B, H, W, Cch):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B * Ho * Wo, Cch), device=x.device, dtype=x.dtype)
    idx = torch.empty((B * Ho * Wo, Cch), device=x.device, dtype=torch.uint8)
    L.check(L.load().sedt_maxpool_fwd(_p(x), _p(y), _p(idx), B, H, W, Cch, dtype, L.stream_ptr()), 'maxpool_fwd')
    return y, idx, Ho, Wo


def maxpool_bwd(dtype, dy, idx, relu_src, B, H, W, Cch, y=None):
    """dx of the 3x3/s2 max-pool, optionally through the ReLU that produced the pooled tensor: relu_src = that tensor at
    full resolution, or (cheaper) y = the pooled output itself"""
    dx = torch.empty((B * H * W, Cch), device=dy.device, dtype=dy.dtype)
    L.check(L.load().sedt_maxpool_bwd_y(_p(dy), _p(idx), _p(relu_src), _p(y), _p(dx), B, H, W, Cch, dtype, L.stream_ptr()),
            'maxpool_bwd')
    return dx


def avgpool(dtype, x, B, P, Cch):
    out = torch.empty((B, Cch), device=x.device, dtype=torch.float32)
    L.check(L.load().sedt_avgpool(_p(x), _p(out), B, P, Cch, dtype, L.stream_ptr()), 'avgpool')
    return out


def sumsq(g, out, accumulate=False):
    lib = L.load()
    nb = lib.sedt_sumsq_scratch(g.numel())
    scratch = torch.empty((nb // 4,), device=g.device, dtype=torch.float32)
    L.check(lib.sedt_sumsq(_p(g), g.numel(), _p(out), _p(scratch), nb, int(accumulate), L.stream_ptr()), 'sumsq')
    return out


def adamw_clip(p, g, m, v, sumsq_t, max_norm, lr, beta1, beta2, eps, weight_decay, step):
    L.check(L.load().sedt_adamw_clip(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(sumsq_t), max_norm, lr, beta1, beta2, eps,
                                     weight_decay, step, L.stream_ptr()), 'adamw_clip')


def set_criterion(logits, boxes, at, dense, empty_weight, layer_of, w_ce, w_bbox, w_giou, w_weak, fl=False, alpha_fl=0.5,
                  gamma_fl=1.0, nonfinite=None, q0=0, at_p=None, w_weak_p=0.0, wp_all=False):
    """device half of SetCriterion in one launch (csrc/criterion.hip).  logits [L,B,Qs,C+1], boxes [L,B,Qs,2] (the Q queries
    q0 .. q0+Q-1 of every clip take part, Q from the dense targets), at [Bat,C] or None - all f32 contiguous; dense =
    SetCriterion.dense_views(...).  fl: the focal-loss variant (sedt.py:176, 211-218).  nonfinite: optional int32 device word set
    to 1 when the weighted total is NaN/inf.  at_p [Bp,C]: the pooled clip-level probabilities of a --pooling model (loss_weak_p over
    the weak clips, or over all labelled ones when wp_all = the reference's weak_mask None).  Returns (out[4L+6], total scalar,
    state); state feeds set_criterion_bwd."""
    _dev_check(logits, boxes)
    Lh, B, Qs, C1 = logits.shape
    Q = dense['tc'].shape[2]
    assert logits.dtype == torch.float32 and boxes.dtype == torch.float32 and logits.is_contiguous() and boxes.is_contiguous()
    assert boxes.shape == (Lh, B, Qs, 2) and Lh <= L.CRIT_MAXL and len(layer_of) == Lh and 0 <= q0 and q0 + Q <= Qs
    a = L.SedtCriterion()
    dl = torch.empty((Lh, B, Q, C1), device=logits.device, dtype=torch.float32)
    db, db2 = torch.empty((Lh, B, Q, 2), device=logits.device, dtype=torch.float32), torch.empty((Lh, B, Q, 2), device=logits.device, dtype=torch.float32)
    dat = None
    out = torch.empty(4 * Lh + 6, device=logits.device, dtype=torch.float32)
    total = torch.empty((), device=logits.device, dtype=torch.float32)
    a.logits, a.boxes, a.out, a.total = logits.data_ptr(), boxes.data_ptr(), out.data_ptr(), total.data_ptr()
    a.dlogits, a.dboxes, a.dboxes2 = dl.data_ptr(), db.data_ptr(), db2.data_ptr()
    for k in ('tc', 'coef', 'wbox', 'tbox', 'tgt_len'):
        setattr(a, k, dense[k].data_ptr())
    if dense.get('num_boxes') is not None:          # None: the kernel sums the final layer's box weights itself
        a.num_boxes = dense['num_boxes'].data_ptr()
    a.empty_weight = empty_weight.data_ptr()
    a.L, a.B, a.ns, a.Q, a.C, a.n_lab, a.Qs, a.q0 = Lh, B, dense['ns'], Q, C1 - 1, dense['n_lab'], Qs, q0
    assert dense['tgt_len'].numel() == B and dense['L'] == Lh and empty_weight.is_cuda and empty_weight.numel() == C1
    if at is not None:
        assert at.dtype == torch.float32 and at.is_contiguous() and at.dim() == 2 and at.shape[1] == C1 - 1
        dat = torch.empty_like(at)
        a.at, a.dat, a.gt_weak, a.Bat = at.data_ptr(), dat.data_ptr(), dense['gt_weak'].data_ptr(), at.shape[0]
        assert dense['n_lab'] <= at.shape[0]
    dat_p = None
    if at_p is not None:
        assert at is not None, 'loss_weak_p needs the audio-tag output (the reference builds its targets in loss_weak)'
        if wp_all and at_p.shape[0] != dense['n_lab']:
            # reference sedt.py:184 with weak_mask None indexes both tensors with None: [1, B, C] against [1, n_lab, C] - BCELoss raises
            # on the shape mismatch whenever unlabelled clips ride in the batch
            raise ValueError(f"loss_weak_p with weak_mask=None needs every clip of the batch labelled (at_p has {at_p.shape[0]} clips, "
                             f"{dense['n_lab']} are labelled): the reference's BCELoss rejects the shapes (sedt.py:184)")
        assert at_p.dtype == torch.float32 and at_p.is_contiguous() and at_p.dim() == 2 and at_p.shape[1] == C1 - 1
        assert dense['n_lab'] <= at_p.shape[0]
        dat_p = torch.empty_like(at_p)
        a.at_p, a.dat_p, a.Bp, a.w_weak_p, a.wp_all = at_p.data_ptr(), dat_p.data_ptr(), at_p.shape[0], w_weak_p, int(bool(wp_all))
    for i in range(Lh):
        a.layer_of[i], a.w_ce[i], a.w_bbox[i], a.w_giou[i] = layer_of[i], w_ce[i], w_bbox[i], w_giou[i]
    a.w_weak = w_weak
    a.fl, a.alpha_fl, a.gamma_fl = int(bool(fl)), alpha_fl, gamma_fl
    if nonfinite is not None:
        assert nonfinite.dtype == torch.int32 and nonfinite.is_cuda
        a.nonfinite = nonfinite.data_ptr()
    if dense.get('split') is not None:              # {ns, n_lab} of this batch as device words (mix-up moves the boundary)
        assert dense['split'].dtype == torch.int32 and dense['split'].is_cuda and dense['split'].numel() >= 2
        a.split = dense['split'].data_ptr()
    scratch = torch.empty(Lh * B * Q * 5, device=logits.device, dtype=torch.float32)
    L.check(L.load().sedt_set_criterion(a, _p(scratch), L.stream_ptr()), 'set_criterion')
    return out, total, (a, dl, db, db2, dat, dat_p, (Lh, B, Qs, C1))


def set_criterion_bwd(state, g, gtotal=None):
    """gradients of (logits, boxes, at, at_p) - in the layout of the head outputs, zero rows for queries outside the window - given the
    gradient g[4L+6] of the loss vector and / or the gradient of the separately returned total (either may be None)"""
    a, dl, db, db2, dat, dat_p, (Lh, B, Qs, C1) = state
    g = None if g is None else g.contiguous().float()
    gtotal = None if gtotal is None else gtotal.contiguous().float()
    gl = torch.empty((Lh, B, Qs, C1), device=dl.device, dtype=torch.float32)
    gb = torch.empty((Lh, B, Qs, 2), device=dl.device, dtype=torch.float32)
    gat = None if dat is None else torch.empty_like(dat)
    gat_p = None if dat_p is None else torch.empty_like(dat_p)
    L.check(L.load().sedt_set_criterion_bwd(a, _p(g), _p(gtotal), _p(gl), _p(gb), _p(gat), _p(gat_p), L.stream_ptr()), 'set_criterion_bwd')
    return gl, gb, gat, gat_p


def match_targets(logits, boxes, tables, dense, layer_of, w_class, w_bbox, w_giou, max_targets, assign=None, fl=False,
                  fine_tune=False, normalize=False, epsilon=1.0, alpha=1.0, alpha_fl=0.5, gamma_fl=1.0, ft_rand=None, ft_seed=0,
                  seed_ptr=None, q0=0):
    """device-side Hungarian matching + dense targets in one launch (csrc/criterion.hip).  tables: dict with lab_cat (int64),
    lab_off (int32 [B+1]), box_cat (f32 [N,2]), box_off (int32 [ns+1]), ratio_cat (f32 or None); dense: the views of
    SetCriterion.dense_views, written in place.  fl / fine_tune / normalize: the matcher variants of matcher.py:73-78,
    99-121, 124-132 (ft_rand [ns,Q] f32 injects the uniforms of the fine-tune branch; else a counter hash of ft_seed)."""
    _dev_check(logits, boxes)
    Lh, B, Qs, C1 = logits.shape
    Q = dense['tc'].shape[2]                        # queries q0 .. q0+Q-1 of the Qs head rows per clip are matched
    assert logits.dtype == torch.float32 and boxes.dtype == torch.float32 and logits.is_contiguous() and boxes.is_contiguous()
    assert 0 <= q0 and q0 + Q <= Qs
    a = L.SedtMatch()
    a.logits, a.boxes = logits.data_ptr(), boxes.data_ptr()
    assert tables['lab_cat'].dtype == torch.int64 and tables['lab_off'].dtype == torch.int32 and tables['box_off'].dtype == torch.int32
    assert tables['box_cat'].dtype == torch.float32 and tables['lab_off'].numel() >= B + 1 and tables['box_off'].numel() >= dense['ns'] + 1
    for k in ('lab_cat', 'lab_off', 'box_cat', 'box_off'):
        assert tables[k].is_cuda and tables[k].is_contiguous()
        setattr(a, k, tables[k].data_ptr())
    if tables.get('ratio_cat') is not None:
        assert tables['ratio_cat'].dtype == torch.float32 and tables['ratio_cat'].is_cuda
        a.ratio_cat = tables['ratio_cat'].data_ptr()
    for k in ('tc', 'coef', 'wbox', 'tbox', 'tidx', 'tgt_len'):
        setattr(a, k, dense[k].data_ptr())
    if dense['gt_weak'].numel():
        a.gt_weak = dense['gt_weak'].data_ptr()
    if assign is not None:
        assert assign.dtype == torch.int32 and assign.numel() == Lh * dense['ns'] * Q
        a.assign = assign.data_ptr()
    a.L, a.B, a.ns, a.Q, a.C, a.n_lab, a.max_targets, a.Qs, a.q0 = Lh, B, dense['ns'], Q, C1 - 1, dense['n_lab'], max_targets, Qs, q0
    assert dense['L'] == Lh and dense['tgt_len'].numel() == B
    for i in range(Lh):
        a.layer_of[i] = layer_of[i]
    a.w_class, a.w_bbox, a.w_giou = w_class, w_bbox, w_giou
    a.fl, a.fine_tune, a.normalize = int(bool(fl)), int(bool(fine_tune)), int(bool(normalize))
    a.alpha_fl, a.gamma_fl, a.epsilon, a.alpha = alpha_fl, gamma_fl, epsilon, alpha
    if ft_rand is not None:
        assert ft_rand.dtype == torch.float32 and ft_rand.is_cuda and ft_rand.is_contiguous() and ft_rand.numel() >= dense['ns'] * Q
        a.ft_rand = ft_rand.data_ptr()
    a.ft_seed = ft_seed & 0xffffffff
    if seed_ptr is not None:
        a.seed_ptr = seed_ptr.data_ptr()
    if dense.get('split') is not None:
        assert dense['split'].dtype == torch.int32 and dense['split'].is_cuda and dense['split'].numel() >= 2
        a.split = dense['split'].data_ptr()
    L.check(L.load().sedt_match_targets(a, L.stream_ptr()), 'match_targets')


def sum_f32(x, out=None):
    """out[0] = sum(x) in a fixed order (one small launch)"""
    x = x.contiguous()
    assert x.dtype == torch.float32 and x.is_cuda
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float32)
    L.check(L.load().sedt_sum_f32(_p(x), x.numel(), _p(out), L.stream_ptr()), 'sum_f32')
    return out


def _pool_args(logits, boxes, attn, mode, q0, Q):
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 3 and logits.is_cuda
    B, Qs, C1 = logits.shape
    a = L.SedtPoolAt()
    a.logits, a.B, a.Qs, a.q0, a.Q, a.C, a.mode = logits.data_ptr(), B, Qs, q0, Q, C1 - 1, L.POOL_MODES[mode]
    if mode == 'weighted_sum':
        assert boxes is not None and boxes.dtype == torch.float32 and boxes.is_contiguous() and boxes.shape == (B, Qs, 2)
        a.boxes = boxes.data_ptr()
    if mode == 'attn':
        assert attn is not None and attn.dtype == torch.float32 and attn.is_contiguous() and attn.shape == (B, Q, C1 - 1)
        a.attn = attn.data_ptr()
    return a


def pool_at(logits, boxes, attn, mode, q0, Q):
    """--pooling variants (sedt.py:96-119; csrc/pool_at.hip): at_p [B,C] from the final layer's class logits [B,Qs,C+1] (event
    queries q0 .. q0+Q-1), the boxes [B,Qs,2] (mode 'weighted_sum') or the attention logits [B,Q,C] (mode 'attn'); all f32."""
    a = _pool_args(logits, boxes, attn, mode, q0, Q)
    out = torch.empty((a.B, a.C), device=logits.device, dtype=torch.float32)
    L.check(L.load().sedt_pool_at(a, _p(out), L.stream_ptr()), 'pool_at')
    return out


def pool_at_bwd(logits, boxes, attn, mode, q0, Q, g):
    """(glogits [B,Qs,C+1], gboxes [B,Qs,2] | None, gattn [B,Q,C] | None) for the gradient g [B,C] that reached at_p"""
    a = _pool_args(logits, boxes, attn, mode, q0, Q)
    g = g.contiguous().float()
    assert g.shape == (a.B, a.C)
    gl = torch.empty_like(logits)
    gb = torch.empty_like(boxes) if mode == 'weighted_sum' else None
    ga = torch.empty_like(attn) if mode == 'attn' else None
    L.check(L.load().sedt_pool_at_bwd(a, _p(g), _p(gl), _p(gb), _p(ga), L.stream_ptr()), 'pool_at_bwd')
    return gl, gb, ga


def feature_loss(pred, gt, dense, layer_of, num_boxes, w=None, nonfinite=None, base=None):
    """SP-SEDT feature-reconstruction loss (sedt.py:263-283) of every decoder layer in one launch.  pred [L,B,Q,F] f32,
    gt [B*P,F] f32, w [L] f32 layer weights.  Returns (out[L+1]: loss per dense layer + their weighted sum,
    dpred [L,B,Q,F] = d loss[d] / d pred, unweighted) - and, with base (a device scalar: the criterion's running weighted total), a third
    result total = base + out[L]."""
    _dev_check(pred, gt)
    Lh, B, Q, F = pred.shape
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.is_contiguous() and gt.is_contiguous()
    ns = dense['ns']
    P = gt.shape[0] // max(ns, 1)
    assert gt.shape == (ns * P, F) and dense['L'] == Lh and num_boxes.numel() == 1
    dpred = torch.empty_like(pred)
    rowloss = torch.empty(Lh * ns * Q, device=pred.device, dtype=torch.float32)
    out = torch.empty(Lh + 1, device=pred.device, dtype=torch.float32)
    lay = (C.c_int32 * Lh)(*layer_of)
    total = torch.empty((), device=pred.device, dtype=torch.float32) if base is not None else None
    if base is not None:
        assert base.dtype == torch.float32 and base.numel() == 1 and base.is_cuda
    L.check(L.load().sedt_feature_loss(_p(pred), _p(gt), _p(dense['wbox']), _p(dense['tidx']), _p(num_boxes), lay, _p(w), Lh, B, ns, Q, P, F,
                                       _p(rowloss), _p(out), _p(dpred), _p(nonfinite), _p(base), _p(total), L.stream_ptr()), 'feature_loss')
    return (out, dpred) if base is None else (out, dpred, total)


def scale_layers(x, g, gtot, w, idx=None):
    """in place: x[l] *= g[d] + gtot[0] * w[d], d = idx[l] (identity when None)   (x [L, ...] f32; g, w [L]; gtot [1])"""
    Lh = x.shape[0]
    per = x.numel() // Lh
    ia = None if idx is None else (C.c_int32 * Lh)(*idx)
    L.check(L.load().sedt_scale_layers(_p(x), _p(g), _p(gtot), _p(w), ia, Lh, per, L.stream_ptr()), 'scale_layers')
    return x


def postprocess(logits, boxes, sizes=None, tags=None, at_m=2, is_semi=False, threshold=0.5):
    """PostProcess.forward on the device (sedt.py:355-396): (scores [B,Q], labels [B,Q] int64, boxes [B,Q,2])"""
    _dev_check(logits, boxes)
    B, Q, C1 = logits.shape
    logits, boxes = logits.detach().float().contiguous(), boxes.detach().float().contiguous()
    tg = None if tags is None else tags.to(device=logits.device, dtype=torch.float32).contiguous()
    sz = None if sizes is None else sizes.to(device=logits.device, dtype=torch.float32).reshape(-1).contiguous()
    scores = torch.empty((B, Q), device=logits.device, dtype=torch.float32)
    labels = torch.empty((B, Q), device=logits.device, dtype=torch.int64)
    out = torch.empty((B, Q, 2), device=logits.device, dtype=torch.float32)
    L.check(L.load().sedt_postprocess(_p(logits), _p(boxes), _p(tg), _p(sz), B, Q, C1 - 1, at_m, 0.0 if threshold is None else float(threshold),
                                      int(bool(is_semi)), _p(scores), _p(labels), _p(out), L.stream_ptr()), 'postprocess')
    return scores, labels, out


def pseudo_labels(logits, boxes, at, thr, min_len, tables, counter=None, del_overlap=True):
    """engine.get_pseudo_labels on the device (engine.py:300-348): fills the flat target tables (dict with lab_cat int64,
    box_cat f32 [N,2], lab_off / box_off int32 [B+1]) that match_targets reads; counter int32 [C] accumulates the kept events
    per class."""
    _dev_check(logits, boxes, thr)
    B, Q, C1 = logits.shape
    logits, boxes = logits.detach().float().contiguous(), boxes.detach().float().contiguous()
    at = None if at is None else at.detach().float().contiguous()
    assert thr.dtype == torch.float32 and thr.numel() == C1 - 1 and thr.is_contiguous()
    assert tables['lab_cat'].dtype == torch.int64 and tables['box_cat'].dtype == torch.float32
    assert tables['lab_off'].dtype == torch.int32 and tables['box_off'].dtype == torch.int32
    assert tables['lab_off'].numel() >= B + 1 and tables['box_off'].numel() >= B + 1
    cap = min(tables['lab_cat'].numel(), tables['box_cat'].numel() // 2)
    if counter is not None:
        assert counter.dtype == torch.int32 and counter.numel() >= C1 - 1 and counter.is_cuda
    L.check(L.load().sedt_pseudo_labels(_p(logits), _p(boxes), _p(at), _p(thr), float(min_len), B, Q, C1 - 1, int(bool(del_overlap)),
                                        _p(tables['lab_cat']), _p(tables['box_cat']), _p(tables['lab_off']), _p(tables['box_off']),
                                        _p(counter), cap, L.stream_ptr()), 'pseudo_labels')


def _clip_table_args(clip_idx, B, table, n_clips, dur=False):
    """the asserts the three clip-level scoring launches share: clip indices and utilities.scoring.ClipReference's device table"""
    assert clip_idx.dtype == torch.int32 and clip_idx.numel() == B and clip_idx.is_contiguous()
    assert table['off'].dtype == torch.int32 and table['off'].numel() >= n_clips + 1
    assert table['present'].dtype == torch.int32 and table['present'].numel() >= n_clips
    assert table['cls'].dtype == torch.int32 and table['on'].dtype == torch.float64 and table['end'].dtype == torch.float64
    assert not dur or (table['dur'].dtype == torch.float64 and table['dur'].numel() >= n_clips)


def event_metrics_update(scores, labels, boxes, at_tags, clip_idx, table, n_clips, max_ref, ev_counts, tag_counts, fusion,
                         threshold=0.5, min_duration=0.2, max_len=10.0, t_collar=0.2, pct=0.2, del_overlap=True, optimal=True,
                         seg_counts=None, sdi_counts=None, time_resolution=1.0, n_seg_words=1):
    """decode_strong + sed_eval's event-based and clip-level counts of one fusion strategy's PostProcess outputs, accumulated into
    ev_counts int64 [n_fusion, C, 3] / tag_counts int64 [n_fusion + 1, C, 3] (include/sedt_hip.h: sedt_event_metrics_update).
    table: dict of the device reference table (present int32 [n_clips], off int32 [n_clips + 1], cls int32, on / end float64);
    clip_idx int32 [B] (-1 = outside the table); at_tags int64 [B, C] or None.  With seg_counts int64 [n_fusion, C, 3] and
    sdi_counts int64 [n_fusion, 3] the same launch adds sed_eval's segment-based counts at ``time_resolution`` seconds over
    ``n_seg_words`` words of 64 segments per clip (sedt_event_segment_metrics_update)."""
    _dev_check(scores, labels, boxes, clip_idx, ev_counts, tag_counts)
    B, Q = scores.shape
    nf, C = ev_counts.shape[0], ev_counts.shape[1]
    assert scores.dtype == torch.float32 and labels.dtype == torch.int64 and boxes.dtype == torch.float32
    assert scores.is_contiguous() and labels.is_contiguous() and boxes.is_contiguous() and tuple(boxes.shape) == (B, Q, 2)
    assert tuple(labels.shape) == (B, Q)
    _clip_table_args(clip_idx, B, table, n_clips)
    assert ev_counts.dtype == torch.int64 and tuple(ev_counts.shape) == (nf, C, 3) and ev_counts.is_contiguous()
    assert tag_counts.dtype == torch.int64 and tuple(tag_counts.shape) == (nf + 1, C, 3) and tag_counts.is_contiguous()
    if at_tags is not None:
        assert at_tags.dtype == torch.int64 and tuple(at_tags.shape) == (B, C) and at_tags.is_contiguous() and at_tags.is_cuda
    if seg_counts is None:
        L.check(L.load().sedt_event_metrics_update(_p(scores), _p(labels), _p(boxes), _p(at_tags), _p(clip_idx), _p(table['present']),
                                                   _p(table['off']),
                                                   _p(table['cls']), _p(table['on']), _p(table['end']), int(n_clips), int(max_ref), B, Q, C,
                                                   nf, int(fusion), float(threshold), float(min_duration), float(max_len), float(t_collar),
                                                   float(pct), int(bool(del_overlap)), int(bool(optimal)), _p(ev_counts), _p(tag_counts),
                                                   L.stream_ptr()), 'event_metrics_update')
        return
    _dev_check(seg_counts, sdi_counts)
    assert seg_counts.dtype == torch.int64 and tuple(seg_counts.shape) == (nf, C, 3) and seg_counts.is_contiguous()
    assert sdi_counts.dtype == torch.int64 and tuple(sdi_counts.shape) == (nf, 3) and sdi_counts.is_contiguous()
    L.check(L.load().sedt_event_segment_metrics_update(
        _p(scores), _p(labels), _p(boxes), _p(at_tags), _p(clip_idx), _p(table['present']), _p(table['off']), _p(table['cls']),
        _p(table['on']), _p(table['end']), int(n_clips), int(max_ref), B, Q, C, nf, int(fusion), float(threshold), float(min_duration),
        float(max_len), float(t_collar), float(pct), int(bool(del_overlap)), int(bool(optimal)), _p(ev_counts), _p(tag_counts),
        float(time_resolution), int(n_seg_words), _p(seg_counts), _p(sdi_counts), L.stream_ptr()), 'event_segment_metrics_update')


DECODE_MAX_THRESHOLDS = 1024      # csrc/event_records.h: SEDT_MAX_THRESHOLDS


def decode_events_views(packed, Q):
    """typed views on a packed decode buffer [K, B, 1 + 5 Q] (int32; a device tensor, a host tensor or a numpy array alike):
    (count [K,B] int32, class [K,B,Q] int32, times [K,B,Q,2] f32 {onset, offset}, score [K,B,Q] f32, query [K,B,Q] int32)"""
    f32 = torch.float32 if torch.is_tensor(packed) else np.float32
    K, B = packed.shape[0], packed.shape[1]
    slots = packed[:, :, 1:].reshape(K, B, Q, 5)
    return packed[:, :, 0], slots[..., 0], slots[..., 1:3].view(f32), slots[..., 3].view(f32), slots[..., 4]


def decode_events(scores, labels, boxes, thresholds, n_classes, min_duration=0.2, max_len=10.0, del_overlap=True, out=None):
    """decode_strong + the clip to [0, max_len] of one fusion strategy's PostProcess outputs (scores [B,Q] f32, labels [B,Q] int64,
    boxes [B,Q,2] f32 seconds) at every threshold of the DEVICE f32 vector ``thresholds`` [K], written out as event records in the
    reference's output order (include/sedt_hip.h: sedt_decode_events).  ``thresholds`` [K, C] holds one threshold per operating
    point and class: a query is compared with the one of its label (sedt_decode_events_classwise).  max_len: a value float32 holds
    exactly, inf = no clip.  Returns (packed, count, class, times, score, query): the int32 buffer [K, B, 1 + 5 Q] (``out`` when
    given) and decode_events_views of it."""
    _dev_check(scores, labels, boxes, thresholds, out)
    B, Q = scores.shape
    K = thresholds.shape[0] if thresholds.dim() else 0
    assert scores.dtype == torch.float32 and labels.dtype == torch.int64 and boxes.dtype == torch.float32
    assert scores.is_contiguous() and labels.is_contiguous() and boxes.is_contiguous() and tuple(boxes.shape) == (B, Q, 2)
    assert tuple(labels.shape) == (B, Q) and thresholds.dtype == torch.float32 and thresholds.is_contiguous()
    assert thresholds.dim() == 1 or tuple(thresholds.shape) == (K, int(n_classes)), (tuple(thresholds.shape), n_classes)
    if out is None:
        out = torch.empty((K, B, 1 + 5 * Q), device=scores.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and tuple(out.shape) == (K, B, 1 + 5 * Q) and out.is_contiguous()
    entry = L.load().sedt_decode_events if thresholds.dim() == 1 else L.load().sedt_decode_events_classwise
    L.check(entry(_p(scores), _p(labels), _p(boxes), _p(thresholds), B, Q, int(n_classes), K, float(min_duration), float(max_len),
                  int(bool(del_overlap)), _p(out), L.stream_ptr()), 'decode_events' if thresholds.dim() == 1 else 'decode_events_classwise')
    return (out,) + decode_events_views(out, Q)


def event_sweep_update(records, clip_idx, table, n_clips, max_ref, n_classes, ev_counts, tag_counts, fusion, t_collar=0.2, pct=0.2,
                       optimal=True):
    """sed_eval's event-based and the clip-level counts of one fusion strategy's event records (``records``: the int32 buffer
    [K, B, 1 + 5 Q] decode_events filled) at every threshold of the grid, accumulated into ev_counts / tag_counts int64
    [n_fusion, K, C, 3] at row ``fusion`` (include/sedt_hip.h: sedt_event_sweep_update).  table: event_metrics_update's device
    reference table; clip_idx int32 [B] (-1 = outside the table).  Nothing is decoded again and nothing is read back."""
    _dev_check(records, clip_idx, ev_counts, tag_counts)
    K, B = records.shape[0], records.shape[1]
    C = int(n_classes)
    Q = (records.shape[2] - 1) // 5
    assert records.dtype == torch.int32 and records.dim() == 3 and records.shape[2] == 1 + 5 * Q and records.is_contiguous()
    _clip_table_args(clip_idx, B, table, n_clips)
    nf = ev_counts.shape[0]
    assert ev_counts.dtype == torch.int64 and tuple(ev_counts.shape) == (nf, K, C, 3) and ev_counts.is_contiguous()
    assert tag_counts.dtype == torch.int64 and tuple(tag_counts.shape) == (nf, K, C, 3) and tag_counts.is_contiguous()
    L.check(L.load().sedt_event_sweep_update(_p(records), _p(clip_idx), _p(table['present']), _p(table['off']), _p(table['cls']),
                                             _p(table['on']), _p(table['end']), int(n_clips), int(max_ref), B, Q, C, K, nf, int(fusion),
                                             float(t_collar), float(pct), int(bool(optimal)), _p(ev_counts), _p(tag_counts),
                                             L.stream_ptr()), 'event_sweep_update')


def psds_update(records, clip_idx, table, n_clips, max_ref, n_classes, counts, fusion, dtc=0.5, gtc=0.5, cttc=0.3):
    """the PSDS confusion counts of one fusion strategy's event records (``records``: the int32 buffer [K, B, 1 + 5 Q] decode_events
    filled), accumulated into counts int64 [n_fusion, K, C, C + 1] at row ``fusion`` (include/sedt_hip.h: sedt_psds_update).
    table: event_metrics_update's device reference table plus 'dur' float64 [n_clips], the clips' durations in seconds;
    clip_idx int32 [B] (-1 = outside the table).  Nothing is decoded again and nothing is read back."""
    _dev_check(records, clip_idx, counts)
    K, B = records.shape[0], records.shape[1]
    C = int(n_classes)
    Q = (records.shape[2] - 1) // 5
    assert records.dtype == torch.int32 and records.dim() == 3 and records.shape[2] == 1 + 5 * Q and records.is_contiguous()
    _clip_table_args(clip_idx, B, table, n_clips, dur=True)
    nf = counts.shape[0]
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (nf, K, C, C + 1) and counts.is_contiguous()
    L.check(L.load().sedt_psds_update(_p(records), _p(clip_idx), _p(table['present']), _p(table['off']), _p(table['cls']), _p(table['on']),
                                      _p(table['end']), _p(table['dur']), int(n_clips), int(max_ref), B, Q, C, K, nf, int(fusion),
                                      float(dtc), float(gtc), float(cttc), _p(counts), L.stream_ptr()), 'psds_update')


STITCH_MAX_DEPTH = 8              # csrc/stitch.hip: earlier windows that may still be open when a window is reached
STITCH_WORDS = 8                  # words of one stitched event {onset f64, offset f64, score f32, n_merged, window, query}


def stitch_events_views(out):
    """typed views on a stitched event buffer [K, R, C, cap, 8] (int32; a device tensor, a host tensor or a numpy array alike):
    (times [K,R,C,cap,2] f64 {onset, offset}, score [K,R,C,cap] f32, n_merged, window, query [K,R,C,cap] int32)"""
    f32, f64 = (torch.float32, torch.float64) if torch.is_tensor(out) else (np.float32, np.float64)
    return out[..., 0:4].view(f64), out[..., 4].view(f32), out[..., 5], out[..., 6], out[..., 7]


def stitch_events(records, win_off, win_start, rec_dur, n_classes, merge_gap=0.0, cap=64, n_windows=None, out=None, count=None,
                  status=None):
    """the event records of the overlapping windows of R recordings (``records``: int32 [K, W_stride, 1 + 5 Q], decode_events' words,
    one row per window) merged into one event list per (threshold, recording, class): include/sedt_hip.h: sedt_stitch_events.
    win_off int32 [R + 1], win_start float64 [W], rec_dur float64 [R] on the device; n_windows: W (else W_stride).  Returns
    (count [K,R,C] int32, out [K,R,C,cap,8] int32, status [K,R] int32); ``out`` is left untouched past min(count, cap), so pass one
    that is filled with what those slots should read."""
    _dev_check(records, win_off, win_start, rec_dur, out, count, status)
    K, Ws = records.shape[0], records.shape[1]
    Q = (records.shape[2] - 1) // 5
    C, R = int(n_classes), win_off.numel() - 1
    W = Ws if n_windows is None else int(n_windows)
    assert records.dtype == torch.int32 and records.dim() == 3 and records.shape[2] == 1 + 5 * Q and records.is_contiguous()
    assert win_off.dtype == torch.int32 and win_off.dim() == 1 and R >= 0 and win_off.is_contiguous()
    assert win_start.dtype == torch.float64 and win_start.numel() >= W and win_start.is_contiguous()
    assert rec_dur.dtype == torch.float64 and rec_dur.numel() >= R and rec_dur.is_contiguous()
    if out is None:
        out = torch.zeros((K, R, C, int(cap), STITCH_WORDS), device=records.device, dtype=torch.int32)
    if count is None:
        count = torch.empty((K, R, C), device=records.device, dtype=torch.int32)
    if status is None:
        status = torch.empty((K, R), device=records.device, dtype=torch.int32)
    assert out.dtype == torch.int32 and tuple(out.shape) == (K, R, C, int(cap), STITCH_WORDS) and out.is_contiguous()
    assert count.dtype == torch.int32 and tuple(count.shape) == (K, R, C) and count.is_contiguous()
    assert status.dtype == torch.int32 and tuple(status.shape) == (K, R) and status.is_contiguous()
    L.check(L.load().sedt_stitch_events(_p(records), _p(win_off), _p(win_start), _p(rec_dur), K, W, Ws, R, Q, C, float(merge_gap), int(cap),
                                        _p(count), _p(out), _p(status), L.stream_ptr()), 'stitch_events')
    return count, out, status


STREAM_EMIT_WORDS = 10            # words of one emitted event: the stitched event's eight, then {class, pad}
STREAM_OPEN = 640                 # csrc/stitch_sweep.h: SEDT_ST_OPEN, the most events one launch can make final per (threshold, stream)


def stitch_stream_state_bytes(K, S):
    """the bytes of the open-set state of K thresholds x S streams (include/sedt_hip.h: sedt_stitch_stream_state_bytes)"""
    return int(L.load().sedt_stitch_stream_state_bytes(int(K), int(S)))


def stitch_stream_state(K, S, device):
    """a fresh state for stitch_stream: (state int32 [K * S * words], status int32 [K, S]), zeroed"""
    n = stitch_stream_state_bytes(K, S) // 4
    return torch.zeros(n, dtype=torch.int32, device=device), torch.zeros((int(K), int(S)), dtype=torch.int32, device=device)


def stitch_stream_views(emit):
    """typed views on an emit buffer [K, S, emit_cap, 10] (int32; a device tensor, a host tensor or a numpy array alike):
    (times [K,S,emit_cap,2] f64 {onset, offset}, score [K,S,emit_cap] f32, n_merged, window, query, class [K,S,emit_cap] int32)"""
    f32, f64 = (torch.float32, torch.float64) if torch.is_tensor(emit) else (np.float32, np.float64)
    return emit[..., 0:4].view(f64), emit[..., 4].view(f32), emit[..., 5], emit[..., 6], emit[..., 7], emit[..., 8]


def stitch_stream(records, action, row, t_w, dur, win_index, n_classes, merge_gap, state, emit, emit_count, status):
    """one window of each of S live streams into the streams' open sets (``state``: stitch_stream_state's), the events that became
    final appended to ``emit`` int32 [K, S, emit_cap, 10] at ``emit_count`` int32 [K, S] (in/out): include/sedt_hip.h:
    sedt_stitch_stream.  records int32 [K, B, 1 + 5 Q]; action, row, win_index int32 [S], t_w, dur float64 [S] on the device;
    status int32 [K, S].  Nothing is read back."""
    _dev_check(records, action, row, t_w, dur, win_index, state, emit, emit_count, status)
    K, B = records.shape[0], records.shape[1]
    Q = (records.shape[2] - 1) // 5
    S = action.numel()
    assert records.dtype == torch.int32 and records.dim() == 3 and records.shape[2] == 1 + 5 * Q and records.is_contiguous()
    for t in (action, row, win_index):
        assert t.dtype == torch.int32 and t.numel() == S and t.is_contiguous()
    for t in (t_w, dur):
        assert t.dtype == torch.float64 and t.numel() == S and t.is_contiguous()
    assert emit.dtype == torch.int32 and emit.dim() == 4 and tuple(emit.shape[:2]) == (K, S) and emit.shape[3] == STREAM_EMIT_WORDS
    assert emit.is_contiguous() and state.dtype == torch.int32 and state.is_contiguous()
    assert emit_count.dtype == torch.int32 and tuple(emit_count.shape) == (K, S) and emit_count.is_contiguous()
    assert status.dtype == torch.int32 and tuple(status.shape) == (K, S) and status.is_contiguous()
    L.check(L.load().sedt_stitch_stream(_p(records), _p(action), _p(row), _p(t_w), _p(dur), _p(win_index), K, S, B, Q, int(n_classes),
                                        float(merge_gap), int(emit.shape[2]), _p(state), 4 * state.numel(), _p(emit), _p(emit_count),
                                        _p(status), L.stream_ptr()), 'stitch_stream')
    return emit, emit_count, status


def stream_reset(state, status, which=None):
    """the streams with which[s] != 0 (int32 [S] on the device; None: all) start again: their headers in ``state`` and their
    ``status`` [K, S] words read zero afterwards (sedt_stream_reset)"""
    _dev_check(state, status, which)
    K, S = status.shape
    assert state.dtype == torch.int32 and state.is_contiguous() and status.dtype == torch.int32 and status.is_contiguous()
    assert which is None or (which.dtype == torch.int32 and which.numel() == S and which.is_contiguous())
    L.check(L.load().sedt_stream_reset(_p(state), 4 * state.numel(), _p(which), K, S, _p(status), L.stream_ptr()), 'stream_reset')


def _ring_jobs(jobs_host, jobs):
    h = np.ascontiguousarray(jobs_host, dtype=np.int32).reshape(-1, 4)
    if len(h):
        _dev_check(jobs)
        assert jobs.dtype == torch.int32 and jobs.numel() >= h.size and jobs.is_contiguous()
    return h, h.ctypes.data_as(C.c_void_p) if len(h) else None, _p(jobs) if len(h) else None


def stream_append(src, jobs_host, jobs, ring):
    """samples of the flat staged float32 vector ``src`` into the streams' rings ``ring`` float32 [S, ring_samples]: one launch for
    all jobs {stream, ring write position, offset in src, n} (``jobs_host`` int32 [J, 4] is checked on the host, ``jobs`` is its
    device copy): sedt_stream_append"""
    _dev_check(src, ring)
    assert src.dtype == torch.float32 and src.is_contiguous() and ring.dtype == torch.float32 and ring.dim() == 2 and ring.is_contiguous()
    h, hp, dp = _ring_jobs(jobs_host, jobs)
    L.check(L.load().sedt_stream_append(_p(src), src.numel(), hp, dp, len(h), _p(ring), ring.shape[0], ring.shape[1], L.stream_ptr()),
            'stream_append')


def stream_cut(ring, jobs_host, jobs, wave):
    """windows out of the streams' rings into ``wave`` float32 [B, window]: one launch fills every row - a job {stream, ring read
    position, length, row} copies across the wrap point and zero-pads, a row without a job is zeroed: sedt_stream_cut"""
    _dev_check(ring, wave)
    assert wave.dtype == torch.float32 and wave.dim() == 2 and wave.is_contiguous()
    assert ring.dtype == torch.float32 and ring.dim() == 2 and ring.is_contiguous()
    h, hp, dp = _ring_jobs(jobs_host, jobs)
    L.check(L.load().sedt_stream_cut(_p(ring), ring.shape[0], ring.shape[1], hp, dp, len(h), _p(wave), wave.shape[0], wave.shape[1],
                                     L.stream_ptr()), 'stream_cut')


def _recording_args(count, out, stitch_status, cap, rec_idx, table, counters, status):
    """the shape, dtype and contiguity asserts the two recording-metrics launches share; returns (K, R, C, n_fusion, status)"""
    _dev_check(count, out, stitch_status, rec_idx, table['off'], table['on'], table['end'], status, *counters)
    K, R, C = count.shape
    assert count.dtype == torch.int32 and count.dim() == 3 and count.is_contiguous()
    assert out.dtype == torch.int32 and tuple(out.shape) == (K, R, C, int(cap), STITCH_WORDS) and out.is_contiguous()
    assert stitch_status.dtype == torch.int32 and tuple(stitch_status.shape) == (K, R) and stitch_status.is_contiguous()
    assert rec_idx.dtype == torch.int32 and rec_idx.numel() == R and rec_idx.is_contiguous()
    n_rec, n_ev = int(table['n_rec']), int(table['n_events'])
    assert table['off'].dtype == torch.int32 and table['off'].numel() >= n_rec * C + 1 and table['off'].is_contiguous()
    assert table['on'].dtype == torch.float64 and table['on'].numel() >= n_ev and table['on'].is_contiguous()
    assert table['end'].dtype == torch.float64 and table['end'].numel() >= n_ev and table['end'].is_contiguous()
    nf = counters[0].shape[0]
    if status is None:
        status = torch.empty((K, R), device=count.device, dtype=torch.int32)
    assert status.dtype == torch.int32 and tuple(status.shape) == (K, R) and status.is_contiguous()
    return K, R, C, nf, status


def recording_event_counts(count, out, stitch_status, cap, rec_idx, table, ev_counts, tag_counts, fusion, t_collar=0.2, pct=0.2,
                           optimal=True, status=None):
    """sed_eval's event-based counts and the recording-level presence counts of one fusion strategy's stitched event lists
    (stitch_events' count [K,R,C], out [K,R,C,cap,8], status [K,R] and cap) against the recordings' annotations, accumulated into
    ev_counts / tag_counts int64 [n_fusion, K, C, 3] at row ``fusion`` (include/sedt_hip.h: sedt_recording_event_counts).
    rec_idx int32 [R]: the recordings' indices in the reference table (-1 = not evaluated); table: dict of the device CSR table over
    (reference recording, class) - off int32 [n_rec * C + 1], on / end float64 [n_events] - with the host ints n_rec and n_events.
    Returns status int32 [K, R] (``status`` when given).  Nothing is read back."""
    K, R, C, nf, status = _recording_args(count, out, stitch_status, cap, rec_idx, table, (ev_counts, tag_counts), status)
    assert ev_counts.dtype == torch.int64 and tuple(ev_counts.shape) == (nf, K, C, 3) and ev_counts.is_contiguous()
    assert tag_counts.dtype == torch.int64 and tuple(tag_counts.shape) == (nf, K, C, 3) and tag_counts.is_contiguous()
    L.check(L.load().sedt_recording_event_counts(_p(count), _p(out), _p(stitch_status), _p(rec_idx), _p(table['off']), _p(table['on']),
                                                 _p(table['end']), int(table['n_rec']), int(table['n_events']), K, R, C, int(cap), nf,
                                                 int(fusion), float(t_collar), float(pct), int(bool(optimal)), _p(ev_counts),
                                                 _p(tag_counts), _p(status), L.stream_ptr()), 'recording_event_counts')
    return status


def recording_segment_counts(count, out, stitch_status, cap, rec_idx, table, n_words, seg_counts, sdi_counts, fusion, time_resolution=1.0,
                             status=None):
    """sed_eval's segment-based counts of one fusion strategy's stitched event lists against the recordings' annotations at
    ``time_resolution`` seconds per segment, accumulated into seg_counts int64 [n_fusion, K, C, 3] and sdi_counts int64 [n_fusion, K, 3]
    at row ``fusion`` (include/sedt_hip.h: sedt_recording_segment_counts).  n_words int32 [R]: the 64-segment words every recording
    spans; the other arguments as recording_event_counts.  Returns status int32 [K, R].  Nothing is read back."""
    K, R, C, nf, status = _recording_args(count, out, stitch_status, cap, rec_idx, table, (seg_counts, sdi_counts), status)
    _dev_check(n_words)
    assert n_words.dtype == torch.int32 and n_words.numel() == R and n_words.is_contiguous()
    assert seg_counts.dtype == torch.int64 and tuple(seg_counts.shape) == (nf, K, C, 3) and seg_counts.is_contiguous()
    assert sdi_counts.dtype == torch.int64 and tuple(sdi_counts.shape) == (nf, K, 3) and sdi_counts.is_contiguous()
    L.check(L.load().sedt_recording_segment_counts(_p(count), _p(out), _p(stitch_status), _p(rec_idx), _p(table['off']), _p(table['on']),
                                                   _p(table['end']), _p(n_words), int(table['n_rec']), int(table['n_events']), K, R, C,
                                                   int(cap), nf, int(fusion), float(time_resolution), _p(seg_counts), _p(sdi_counts),
                                                   _p(status), L.stream_ptr()), 'recording_segment_counts')
    return status


def recording_psds_counts(count, out, stitch_status, cap, rec_idx, table, rec_dur, counts, fusion, dtc=0.5, gtc=0.5, cttc=0.3,
                          pass_words=None, status=None):
    """the PSDS confusion counts of one fusion strategy's stitched event lists (stitch_events' count [K,R,C], out [K,R,C,cap,8], status
    [K,R] and cap) against the recordings' annotations, accumulated into counts int64 [n_fusion, K, C, C + 1] at row ``fusion``: psds_update's
    layout (include/sedt_hip.h: sedt_recording_psds_counts).  rec_idx and table as recording_event_counts, the table with 'pmax' float64
    [n_events]: per (recording, class) list the running maximum of 'end'; rec_dur float64 [R]: the recordings' lengths in seconds;
    pass_words int64 [>= K * R * C * ceil(cap / 64)]: the launch's workspace (allocated when None).  Returns status int32 [K, R]
    (``status`` when given).  Nothing is read back."""
    K, R, C, nf, status = _recording_args(count, out, stitch_status, cap, rec_idx, table, (counts,), status)
    _dev_check(table['pmax'], rec_dur, pass_words)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (nf, K, C, C + 1) and counts.is_contiguous()
    assert table['pmax'].dtype == torch.float64 and table['pmax'].numel() >= int(table['n_events']) and table['pmax'].is_contiguous()
    assert rec_dur.dtype == torch.float64 and rec_dur.numel() == R and rec_dur.is_contiguous()
    n_pass = K * R * C * ((int(cap) + 63) // 64)
    if pass_words is None:
        pass_words = torch.empty(max(n_pass, 1), device=count.device, dtype=torch.int64)
    assert pass_words.dtype == torch.int64 and pass_words.numel() >= n_pass and pass_words.is_contiguous()
    L.check(L.load().sedt_recording_psds_counts(_p(count), _p(out), _p(stitch_status), _p(rec_idx), _p(table['off']), _p(table['on']),
                                                _p(table['end']), _p(table['pmax']), _p(rec_dur), int(table['n_rec']),
                                                int(table['n_events']), K, R, C, int(cap), nf, int(fusion), float(dtc), float(gtc),
                                                float(cttc), _p(pass_words), _p(counts), _p(status), L.stream_ptr()),
            'recording_psds_counts')
    return status


def mixup(x1, x2, jobs, out=None):
    """feature half of utilities/mixup.py: out[i] = lam * x1[src1] + (1 - lam) * x2[src2] / x1[src1] / x2[src2] per job record
    (jobs: uint8 device tensor of n 16-byte records {int32 src1, src2, mode; f32 lam}); x1 / x2 / out f32 [*, clip...]"""
    _dev_check(x1, x2, jobs)
    assert x1.dtype == torch.float32 and x2.dtype == torch.float32 and x1.is_contiguous() and x2.is_contiguous()
    assert jobs.dtype == torch.uint8 and jobs.numel() % 16 == 0
    n = jobs.numel() // 16
    if out is None:
        out = torch.empty((n,) + tuple(x1.shape[1:]), device=x1.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == n and out[0].numel() == x1[0].numel() == x2[0].numel()
    L.check(L.load().sedt_mixup(_p(x1), _p(x2), _p(jobs), n, x1[0].numel(), _p(out), L.stream_ptr()), 'mixup')
    return out


def mixup_targets(tab1, tab2, lam, mix_num, tab_out, jobs, max_events=20):
    """label half of mixup_label_unlabel (utilities/mixup.py:129-196) on the device: tab1 = the labelled targets, tab2 = the pseudo
    targets (sedt.TargetTables), lam = f32 device [2] {lam, 1 - lam}; writes the merged targets into tab_out (every clip strong)
    and the B2 feature-mixing records into jobs (uint8 [16 * B2])."""
    d1, d2, do = tab1.as_dict(), tab2.as_dict(), tab_out.as_dict()
    B2 = tab2.B
    assert tab_out.B == B2 and tab_out.ns == B2 and jobs.dtype == torch.uint8 and jobs.numel() >= 16 * B2 and jobs.is_cuda
    assert lam.dtype == torch.float32 and lam.numel() >= 2 and lam.is_cuda and 0 <= mix_num <= min(tab1.B, B2)
    cap = min(do['lab_cat'].numel(), do['box_cat'].numel() // 2)
    L.check(L.load().sedt_mixup_targets(_p(d1['lab_cat']), _p(d1['lab_off']), _p(d1['box_cat']), _p(d1['box_off']), _p(d1['ratio_cat']),
                                        _p(tab1.split), tab1.B, tab1.ns, _p(d2['lab_cat']), _p(d2['lab_off']), _p(d2['box_cat']),
                                        _p(d2['box_off']), B2, _p(lam), mix_num, max_events, _p(do['lab_cat']), _p(do['lab_off']),
                                        _p(do['box_cat']), _p(do['box_off']), _p(do['ratio_cat']), cap, _p(jobs), L.stream_ptr()),
            'mixup_targets')
    return tab_out


def mixup_plan(src_blob, B_src, max_targets_src, B, ns, n_lab, index, lam, mix_num, max_events, max_targets_out, out_blob, jobs, status):
    """label half of mixup_data (utilities/mixup.py:13-127) on the device - utilities.mixup.plan_mixup_data for targets that were built
    on the device: src_blob = the uint8 blob sedt_cut_clips wrote for B_src clips of up to max_targets_src events, read under the
    static split (ns, n_lab) of its first B clips; index int32 [B] and lam f32 [2] {lam, 1 - lam} on the device; writes the merged
    targets into out_blob (uint8, the dynamic-split TargetTables layout of B clips with ratio, max_targets_out events per clip), the B
    feature-mixing records into jobs (uint8 [16 * B]) and status int32 [B] (include/sedt_hip.h: sedt_mixup_plan).  ONE launch."""
    _dev_check(src_blob, index, lam, out_blob, jobs, status)
    B_src, B, Ms, Mo = int(B_src), int(B), int(max_targets_src), int(max_targets_out)
    assert src_blob.dtype == torch.uint8 and out_blob.dtype == torch.uint8 and jobs.dtype == torch.uint8
    assert src_blob.is_contiguous() and out_blob.is_contiguous() and jobs.is_contiguous() and status.is_contiguous()
    if B >= 1 and B_src >= 1 and Ms >= 1 and Mo >= 1:                      # (the entry point refuses the rest with its own message)
        assert src_blob.numel() >= 8 * B_src + 16 + 16 * B_src * Ms, 'mixup_plan: the source blob is smaller than its layout'
        assert out_blob.numel() >= 8 * B + 16 + 20 * B * Mo, 'mixup_plan: the output blob is smaller than the tables with ratio'
        assert jobs.numel() >= 16 * B and status.dtype == torch.int32 and status.numel() >= B
        assert index.dtype == torch.int32 and index.numel() >= B and index.is_contiguous()
        assert lam.dtype == torch.float32 and lam.numel() >= 2 and lam.is_contiguous()
    L.check(L.load().sedt_mixup_plan(_p(src_blob), B_src, Ms, B, int(ns), int(n_lab), _p(index), _p(lam), int(mix_num), int(max_events),
                                     Mo, _p(out_blob), _p(jobs), _p(status), L.stream_ptr()), 'mixup_plan')
    return out_blob
