"""The rows of tests/test_glue_envelope_gpu.py and tests/test_glue_check_cpu.py: the glue, pooling and skinny-head kernels of
csrc/misc.hip, csrc/split3.hip and csrc/skinny.hip at their vector, block, chunk and LDS edges.  Importable without a GPU; nothing here
is sampled: every row listed runs.

A row is a dict with a 'name'; CASES maps a kernel key (the keys of glue_check.KERNELS) to its rows.  The numbers a row is chosen for -
threads, blocks, chunks, LDS bytes - are functions of the row at the end of the module, so that tests/test_glue_check_cpu.py can
assert that each table reaches the edge it names.
"""
import itertools

DTS = ('f32', 'bf16')
N_EDGE = (1, 255, 256, 257, 513)            # both sides of one 256-thread block, and of two
N8_EDGE = (8, 2040, 2048, 2056)             # eight elements per thread: 255, 256, 257 threads


def _named(rows, fmt):
    out = []
    for r in rows:
        r = dict(r)
        r['name'] = fmt.format(**r)
        out.append(r)
    names = [r['name'] for r in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


# ------------------------------------------------------------------------------------------------ elementwise
ADD = _named([dict(rows=1, cols=n, b_mod=0, dt=dt) for n in N_EDGE for dt in DTS] +
             [dict(rows=r, cols=c, b_mod=m, dt=dt) for r, c, m in ((13, 24, 5), (37, 7, 37), (9, 40, 1)) for dt in DTS] +       # ((1, 256, 0) is the count row 256)
             [dict(rows=0, cols=24, b_mod=0, dt=dt) for dt in DTS], 'add_{rows}x{cols}_mod{b_mod}_{dt}')
CAST = _named([dict(n=n, src=s, dst=d) for n in (0,) + N_EDGE for s in DTS for d in DTS], 'cast_{src}_{dst}_n{n}')
RELU_MASK = _named([dict(n=n, dt=dt) for n in (0,) + N_EDGE for dt in DTS], 'relu_mask_n{n}_{dt}')
SIGMOID_GRAD = _named([dict(n=n) for n in (0,) + N_EDGE], 'sigmoid_grad_n{n}')
# via: 'c' = the C entry point (<= 8 sources), 'ops' = ops.add_n, which folds 9 sources into two launches
ADD_N = _named([dict(k=k, n=n, dt=dt, via='c') for k in (1, 2, 3, 8) for n in N8_EDGE for dt in DTS] +
               [dict(k=9, n=n, dt=dt, via='ops') for n in (8, 2056) for dt in DTS] +
               [dict(k=2, n=0, dt=dt, via='c') for dt in DTS], 'add_n_{k}src_n{n}_{dt}_{via}')
# seed mode: 'val' by value, 'ptr' through seed_ptr, 'both' (they add)
DROPOUT_GRAD = _named([dict(rows=r, cols=c, p=p, seed=s, dt=dt) for r, c in ((5, 24), (3, 104)) for p in (0.0, 0.1, 0.5)
                       for s in ('val', 'ptr', 'both') for dt in DTS] +
                      [dict(rows=0, cols=24, p=0.1, seed='val', dt=dt) for dt in DTS], 'dropout_grad_{rows}x{cols}_p{p}_{seed}_{dt}')
GELU = _named([dict(n=n, p=p, dt=dt) for n in (0,) + N8_EDGE for p in (0.0, 0.1) for dt in DTS], 'gelu_n{n}_p{p}_{dt}')

# copy2d: jobs as (outer, inner bytes).  Word counts 255 / 256 / 257 in one item; a one-block job followed by a 71-block one (the blk0
# walk); 'ops' = nine jobs through ops.copy2d (two launches)
_C8 = [(1, 1024), (70, 1028), (1, 1028), (3, 4), (70, 12), (3, 1024), (1, 1020), (3, 1028)]
COPY2D = [dict(name='copy2d_1job', jobs=[(1, 4)], via='c'),
          dict(name='copy2d_3jobs', jobs=[(1, 1020), (70, 1028), (3, 12)], via='c'),
          dict(name='copy2d_8jobs', jobs=_C8, via='c'),
          dict(name='copy2d_9jobs_ops', jobs=_C8 + [(70, 4)], via='ops')]

# split3: jobs as (rows, cols, pad of ld, pattern)
_S4 = [(1, 4), (3, 260), (5, 1024), (7, 148)]
SPLIT3 = [dict(name=f'split3_1job_{r}x{c}_ld{pad}_pat{pat}', jobs=[(r, c, pad, pat)]) for r, c in _S4 for pad in (0, 12) for pat in (0, 1)] + \
         [dict(name='split3_3jobs', jobs=[(1, 4, 0, 1), (5, 1024, 12, 0), (3, 260, 0, 1)]),
          dict(name='split3_8jobs', jobs=[(r, c, pad, pat) for (r, c), pad, pat in zip(_S4 + _S4, (0, 12, 0, 12, 12, 0, 12, 0), (0, 1, 1, 0, 1, 0, 0, 1))])]

# SP-SEDT decoder input.  mode: eval | given (train, keep passed in) | drawn (train, keep drawn at `ratio`)
_DI = [(1, 1, 1, 1, 64), (3, 7, 3, 3, 64), (2, 9, 9, 1, 128), (5, 20, 10, 2, 256)]
_DI_MODES = [('eval', 0.0), ('given', 0.0), ('drawn', 0.0), ('drawn', 0.3), ('drawn', 1.0)]
DEC_IN = _named([dict(B=B, Q=Q, P=P, qpp=qpp, D=D, mode=m, ratio=r, dt=dt) for B, Q, P, qpp, D in _DI for m, r in _DI_MODES for dt in DTS],
                'dec_in_B{B}_Q{Q}_P{P}_qpp{qpp}_D{D}_{mode}{ratio}_{dt}')
DEC_IN_BWD = _named([dict(B=B, Q=3, P=2, qpp=2, D=D, need_patch=npatch, dt=dt) for B in (1, 2, 3, 4, 5, 9, 33, 37) for D in (64, 128, 256)
                     for npatch in (1, 0) for dt in DTS], 'dec_in_bwd_B{B}_D{D}_patch{need_patch}_{dt}')

# ------------------------------------------------------------------------------------------------ reductions and pooling
# view: 0 = dense rows, 8 = a column view (ld = cols + 8); in_f32: an f32 input under the bf16 mode
_CS_ROWS, _CS_COLS = (1, 3, 4, 5, 255, 256, 257, 513), (1, 63, 64, 65, 130)
COLSUM = _named([dict(rows=r, cols=65, view=0, in_f32=0, dt=dt) for r in _CS_ROWS for dt in DTS] +
                [dict(rows=257, cols=c, view=0, in_f32=0, dt=dt) for c in _CS_COLS if c != 65 for dt in DTS] +
                [dict(rows=65537, cols=8, view=0, in_f32=0, dt=dt) for dt in DTS] +
                [dict(rows=513, cols=130, view=8, in_f32=0, dt=dt) for dt in DTS] +
                [dict(rows=257, cols=65, view=8, in_f32=1, dt='bf16')], 'colsum_{rows}x{cols}_view{view}_inf32{in_f32}_{dt}')
# off: the input starts `off` bytes behind a 32-byte boundary: 16 sends a C % 8 == 0 row to the scalar kernel
AVGPOOL = _named([dict(B=3, P=P, C=C, off=0, dt=dt) for C in (8, 688, 2048, 4, 2044) for P in (1, 3, 4, 5, 32) for dt in DTS] +
                 [dict(B=3, P=P, C=688, off=16, dt=dt) for P in (5, 32) for dt in DTS] +
                 [dict(B=0, P=4, C=8, off=0, dt=dt) for dt in DTS], 'avgpool_B{B}_P{P}_C{C}_off{off}_{dt}')
_MP = [(2, h, w, 8) for h, w in ((1, 1), (1, 2), (2, 1), (2, 3), (3, 2), (3, 3), (4, 5), (5, 4), (4, 4), (5, 5))] + [(2, 5, 33, 128)]
MAXPOOL = _named([dict(B=B, H=H, W=W, C=C, dt=dt) for B, H, W, C in _MP for dt in DTS], 'maxpool_B{B}_{H}x{W}_C{C}_{dt}')

# ------------------------------------------------------------------------------------------------ positional and layout
MASK_RESIZE = _named([dict(B=3, Hin=a, Win=b, Hout=c, Wout=d) for a, b, c, d in
                      ((500, 64, 32, 4), (496, 64, 31, 4), (1001, 64, 63, 4), (248, 64, 16, 4), (7, 5, 3, 2), (3, 2, 7, 5), (1, 1, 4, 4))] +
                     [dict(B=0, Hin=7, Win=5, Hout=3, Wout=2)], 'mask_resize_B{B}_{Hin}x{Win}_to_{Hout}x{Wout}')
POSENC = _named([dict(B=B, H=H, W=W, D=D, mask=m, dt=dt) for B, H, W, D in ((1, 1, 1, 8), (2, 5, 3, 64), (2, 31, 4, 256), (3, 32, 4, 256))
                 for m in ('none', 'suffix', 'column', 'holes') for dt in DTS], 'posenc_B{B}_{H}x{W}_D{D}_{mask}_{dt}')
STEM_IM2COL = _named([dict(B=B, H=H, W=W, dt=dt) for B, H, W in ((2, 7, 20), (2, 8, 33), (1, 500, 64), (1, 3, 2042)) for dt in DTS],
                     'stem_im2col_B{B}_{H}x{W}_{dt}')

# ------------------------------------------------------------------------------------------------ skinny heads
SK_NK = ((1, 64), (2, 256), (11, 256), (16, 256), (11, 1024), (16, 512), (16, 1024))
SK_M = (1, 15, 16, 17, 33)
SK_OPTS = list(itertools.product((1, 0), ('none', 'relu', 'sigmoid'), (1, 0)))          # (bias, act, out_f32): 12 combinations
# every (M, N, K, dtype) with one of the 12 option sets in rotation, and every option set at every (N, K, dtype) at M = 17.
# Each row runs twice: x aligned (the vector loader) and x as a column view 8 elements into a wider buffer (the scalar loader).
SKINNY_FWD = _named([dict(M=M, N=N, K=K, dt=dt, bias=SK_OPTS[(i + j) % 12][0], act=SK_OPTS[(i + j) % 12][1], out_f32=SK_OPTS[(i + j) % 12][2])
                     for i, M in enumerate(SK_M) if M != 17 for j, (N, K) in enumerate(SK_NK) for dt in DTS] +
                    [dict(M=17, N=N, K=K, dt=dt, bias=b, act=a, out_f32=o) for N, K in SK_NK for b, a, o in SK_OPTS for dt in DTS],
                    'skinny_fwd_M{M}_N{N}_K{K}_b{bias}_{act}_of{out_f32}_{dt}')
# input gradient.  mask: the ReLU mask of the input; acc: gx is added to a strided view (ld = K + 8)
SKINNY_DGRAD = _named([dict(M=M, N=N, K=K, act=a, mask=m, acc=acc, dt=dt) for M, N, K in ((33, 11, 64), (3, 16, 1024), (17, 2, 256))
                       for a, m, acc in (('none', 0, 0), ('sigmoid', 1, 0), ('relu', 0, 1), ('sigmoid', 0, 1)) for dt in DTS],
                      'skinny_dgrad_M{M}_N{N}_K{K}_{act}_mask{mask}_acc{acc}_{dt}')
# weight gradient.  db: the bias gradient asked for; deferred: the final sum rides in a ReduceBatch (through ops.skinny_linear_bwd)
SKINNY_WGRAD = _named([dict(M=M, N=N, K=K, act=a, db=db, deferred=0, dt=dt) for M in (1, 15, 16, 17, 33, 1000, 16384)
                       for N, K, a, db in ((11, 256, 'sigmoid', 1), (16, 64, 'none', 0)) for dt in DTS] +
                      [dict(M=33, N=11, K=256, act='sigmoid', db=1, deferred=1, dt=dt) for dt in DTS] +
                      [dict(M=1000, N=2, K=256, act='relu', db=1, deferred=0, dt=dt) for dt in DTS],
                      'skinny_wgrad_M{M}_N{N}_K{K}_{act}_db{db}_def{deferred}_{dt}')

CASES = dict(add=ADD, cast=CAST, relu_mask=RELU_MASK, sigmoid_grad=SIGMOID_GRAD, add_n=ADD_N, dropout_grad=DROPOUT_GRAD, gelu=GELU,
             copy2d=COPY2D, split3=SPLIT3, dec_in=DEC_IN, dec_in_bwd=DEC_IN_BWD, colsum=COLSUM, avgpool=AVGPOOL, maxpool=MAXPOOL,
             mask_resize=MASK_RESIZE, posenc=POSENC, stem_im2col=STEM_IM2COL, skinny_fwd=SKINNY_FWD, skinny_dgrad=SKINNY_DGRAD,
             skinny_wgrad=SKINNY_WGRAD)


# ------------------------------------------------------------------------------------------------ what a row reaches
def nblk(n, per=256):
    return (n + per - 1) // per


def colsum_chunks(rows):
    return min(max((rows + 255) // 256, 1), 256)


def colsum_last_chunk_rows(rows):
    ch = colsum_chunks(rows)
    rpc = (rows + ch - 1) // ch
    return rows - (ch - 1) * rpc


def copy_blocks(job):
    outer, inner = job
    return nblk(outer * (inner // 4))


def split_blocks(job):
    return nblk(job[0] * job[1] // 4)


def avgpool_kernel(c):
    """'vec8' or 'scalar': csrc/misc.hip sedt_avgpool's test (the frames are 32-byte aligned before `off`)"""
    return 'vec8' if c['C'] % 8 == 0 and c['off'] % 32 == 0 else 'scalar'


def maxpool_blocks(c):
    vec = 8 if c['dt'] == 'bf16' else 4
    Wo = (c['W'] - 1) // 2 + 1
    n = Wo * (c['C'] // vec)
    bs = min(256, (n + 63) // 64 * 64)
    return nblk(n, bs)


def skinny_fwd_lds(N, K):
    return (N + 16) * (K + 4) * 4


def skinny_dgrad_lds(N, K):
    return N * K * 4


def skinny_wgrad_lds(M):
    return max(((M + 15) // 16) * 16, 4 * 17 * 64) * 4


def stem_lds(W):
    return 7 * (W + 6) * 4
