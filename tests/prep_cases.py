"""The rows of tests/test_prep_envelope_gpu.py and tests/test_prep_check_cpu.py: weight packing (sedt_multi_pack, sedt_pack_conv,
sedt_pack_frag), FrozenBN fold, the stem's weight preparation and conv0 gradient, and the split-K finishing pass
(sedt_multi_wgrad_reduce and its single-job entry points) at their tile, vector, unroll and job-table edges.  Importable without a GPU;
nothing here is sampled: every row listed runs.

A row is a dict with a 'name'; CASES maps a kernel key (the keys of prep_check.KERNELS) to its rows.  The rules the rows are chosen by -
the pack kernel's tile and path, the reduce kernel's mode and block count, the unroll remainders - are restated as functions at the end
of the module, so that tests/test_prep_check_cpu.py can assert that each table holds a row on either side of every condition.
"""
from glue_cases import DTS, _named

# ------------------------------------------------------------------------------------------------ multi_pack / pack_conv
# (Cout, Cin, taps); mis: which pointer sits off its 16-byte boundary (w by 4 bytes, wf / wb by one element); scale / wf / wb: given or null
PACK_T1_VEC = [(64, 64), (8, 8), (72, 136), (128, 200)]
PACK_T1_SCALAR = [(65, 64), (64, 63), (1, 1), (11, 256), (256, 20)]
PACK_T9_VEC = [(32, 32), (8, 8), (40, 96), (64, 40)]
PACK_T9_SCALAR = [(33, 32), (24, 12)]
PACK_RT_TAPS = (2, 3, 4, 5, 8)
PACK_RT_SHAPES = [(32, 32), (40, 24)]
PACK_MIS = [(72, 136, 1), (40, 96, 9), (8, 8, 1)]            # Cin % 8 == 0 and Cout % 8 == 0: scalar by alignment alone


def _pack(Co, Ci, taps, dt, scale=1, wf=1, wb=1, mis='none'):
    return dict(Co=Co, Ci=Ci, taps=taps, dt=dt, scale=scale, wf=wf, wb=wb, mis=mis)


_P = []
for _dt in DTS:
    _P += [_pack(co, ci, 1, _dt) for co, ci in PACK_T1_VEC + PACK_T1_SCALAR]
    _P += [_pack(co, ci, 9, _dt) for co, ci in PACK_T9_VEC + PACK_T9_SCALAR]
    _P += [_pack(co, ci, t, _dt) for t in PACK_RT_TAPS for co, ci in PACK_RT_SHAPES]
    _P += [_pack(co, ci, t, _dt, mis=m) for (co, ci, t), m in zip(PACK_MIS, ('w', 'wf', 'wb'))]
    # null wf / null wb on the vector and the scalar path (both tile widths), null scale on both
    _P += [_pack(co, ci, t, _dt, wf=f, wb=b) for co, ci, t in ((72, 136, 1), (65, 64, 1), (40, 96, 9), (33, 32, 9)) for f, b in ((0, 1), (1, 0))]
    _P += [_pack(co, ci, t, _dt, scale=0) for co, ci, t in ((72, 136, 1), (64, 63, 1), (64, 40, 9), (24, 12, 9), (40, 24, 3))]
PACK = _named(_P, 'pack_{Co}x{Ci}x{taps}_{dt}_s{scale}_f{wf}_b{wb}_mis-{mis}')

# ------------------------------------------------------------------------------------------------ pack_frag
FRAG_NK = [(32, 32), (64, 32), (32, 64), (96, 160)]
FRAG = _named([dict(N=n, K=k, src=s, wf=f, wb=b) for s in DTS for n, k in FRAG_NK for f, b in ((1, 1), (1, 0), (0, 1))],
              'frag_{N}x{K}_{src}_f{wf}_b{wb}')

# ------------------------------------------------------------------------------------------------ FrozenBN fold, stem
BN_N = (1, 255, 256, 257, 2048)
BN_FOLD = _named([dict(n=n) for n in (0,) + BN_N], 'bn_fold_n{n}')
STEM_PREP = _named([dict(dt=dt) for dt in DTS], 'stem_prep_{dt}')
STEM_CONV0_GRAD = [dict(name='stem_conv0_grad')]

# ------------------------------------------------------------------------------------------------ split-K reduce
# splitk slices of [R][taps][Ci] -> out [R][Ci][taps] (* rowscale[r]).  cs: None = no riding column sums, 0 = cs_splitk 0 (the sums have
# splitk slices), k > 0 = cs_splitk k.  mis: the slab ('slab') or the output ('out') 4 bytes past a 16-byte boundary.  Ci = 0: sums only.
RED_SK0 = (1, 2, 4, 5, 6, 8, 9, 15)
RED_PER0 = {4: (1, 4), 1020: (3, 340), 1024: (4, 256), 1028: (1, 1028)}
RED_SK3 = (16, 17, 20, 21, 23, 24, 25, 40)
RED_PER3 = {252: (3, 84), 256: (1, 256), 260: (5, 52)}
RED_CS_R = (1, 63, 64, 65, 130)
RED_CS_SLICES = (1, 3, 4, 5, 13, 16, 17, 29, 512)


def _red(sk, R, taps, Ci, scale, cs=None, mis='none'):
    return dict(splitk=sk, R=R, taps=taps, Ci=Ci, scale=scale, cs=cs, mis=mis)


_R = []
_R += [_red(sk, R, 1, Ci, (i + j) % 2) for i, sk in enumerate(RED_SK0) for j, (R, Ci) in enumerate(RED_PER0.values())]
_R += [_red(sk, R, 1, Ci, (i + j) % 2) for i, sk in enumerate(RED_SK3) for j, (R, Ci) in enumerate(RED_PER3.values())]
_R += [_red(sk, R, 9, Ci, (sk + R) % 2) for Ci in (64, 128) for R in (1, 3) for sk in (1, 2, 3, 4, 5)]
_R += [_red(3, 3, t, 64, t % 2) for t in (2, 3, 4, 8)] + [_red(4, 2, 2, 128, 1)]
_R += [_red(3, 2, 9, 20, 1), _red(5, 7, 1, 6, 0), _red(2, 2, 10, 64, 1), _red(4, 3, 1, 6, 1), _red(1, 2, 9, 20, 0)]
# the wide modes' shapes with a pointer off its boundary: mode 2 by alignment
_R += [_red(sk, R, taps, Ci, sc, mis=m) for m in ('slab', 'out')
       for sk, R, taps, Ci, sc in ((5, 3, 1, 340, 1), (9, 4, 1, 256, 0), (17, 3, 1, 84, 1), (3, 3, 9, 64, 0), (2, 1, 9, 128, 1))]
# riding column sums: R at the 64-column block edges; more sum blocks than reduce blocks (taps 1, Ci 4, R 130: one block of mode 0, three of sums)
_R += [_red(3, R, 1, 4, R % 2, cs=0) for R in RED_CS_R]
_R += [_red(2, 65, 1, 8, n % 2, cs=n) for n in RED_CS_SLICES if n != 2] + [_red(5, 3, 9, 64, 1, cs=3), _red(17, 3, 1, 84, 0, cs=16),
                                                                          _red(3, 70, 9, 20, 1, cs=0), _red(16, 65, 1, 4, 1, cs=0)]
_R += [_red(n, 256, 1, 0, 0, cs=0) for n in (1, 15, 16, 512)] + [_red(5, 100, 1, 0, 0, cs=0)]
REDUCE = _named(_R, 'reduce_sk{splitk}_R{R}_t{taps}_Ci{Ci}_s{scale}_cs{cs}_mis-{mis}')

CASES = dict(pack=PACK, frag=FRAG, bn_fold=BN_FOLD, stem_prep=STEM_PREP, stem_conv0_grad=STEM_CONV0_GRAD, reduce=REDUCE)
MAX_REDUCE_JOBS = 40


# ------------------------------------------------------------------------------------------------ the rules the rows are chosen by
def pack_tile(c):
    """tile edge of multi_pack_kernel: 64 for one tap, 32 otherwise"""
    return 64 if c['taps'] == 1 else 32


def pack_blocks(c):
    ts = pack_tile(c)
    return ((c['Co'] + ts - 1) // ts) * ((c['Ci'] + ts - 1) // ts)


def pack_path(c):
    """'vec' (pack_tile_vec), 'scalar' (pack_tile with a compile-time tap count) or 'runtime' (pack_tile<T, 0>)"""
    if c['taps'] not in (1, 9):
        return 'runtime'
    return 'vec' if c['Co'] % 8 == 0 and c['Ci'] % 8 == 0 and c['mis'] == 'none' else 'scalar'


def reduce_mode(c):
    """reduce_job_mode (csrc/misc.hip)"""
    if c['mis'] != 'none':
        return 2
    if c['taps'] == 1 and c['Ci'] % 4 == 0:
        return 3 if c['splitk'] >= 16 else 0
    if 1 < c['taps'] <= 9 and c['Ci'] % 64 == 0:
        return 1
    return 2


def reduce_blocks(c, sums=True):
    """reduce_job_blocks, and with sums the blocks the riding column sums need on top (sedt_multi_wgrad_reduce)"""
    per, mode = c['R'] * c['taps'] * c['Ci'], reduce_mode(c)
    nb = (per + 1023) // 1024 if mode == 0 else c['R'] * (c['Ci'] // 64) if mode == 1 else (per + 255) // 256
    return max(nb, (c['R'] + 63) // 64) if (sums and c['cs'] is not None) else nb


def cs_slices(c):
    return None if c['cs'] is None else (c['cs'] if c['cs'] > 0 else c['splitk'])


def find_job(blk0, b, fault=None):
    """the binary search of multi_pack_kernel / multi_wgrad_reduce_kernel / pack_frag_kernel: the last job whose first block is <= b"""
    lo, hi = 0, len(blk0) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if (blk0[mid] < b if fault == 'search_off_by_one' else blk0[mid] <= b):
            lo = mid
        else:
            hi = mid - 1
    return lo


def table_coverage(nblocks, fault=None):
    """per job of a table with these block counts, the local block indices the search hands it"""
    blk0 = [sum(nblocks[:i]) for i in range(len(nblocks))]
    got = [[] for _ in nblocks]
    for b in range(sum(nblocks)):
        j = find_job(blk0, b, fault)
        got[j].append(b - blk0[j])
    return got


def reduce_table():
    """the 40 jobs of the one-launch table: every mode, sums-only jobs, riding sums, misaligned jobs, runs of one-block neighbours"""
    rows = REDUCE[::4]
    rows = rows + [c for c in REDUCE if not c['Ci'] and c not in rows]
    rows = rows + [c for c in REDUCE if reduce_blocks(c) == 1 and c not in rows][:MAX_REDUCE_JOBS - len(rows)]
    assert len(rows) == MAX_REDUCE_JOBS
    return rows


def pack_table(dt):
    """about 70 jobs: every row of the dtype, then its one-block rows again (runs of adjacent one-block jobs) and the larger ones"""
    rows = [c for c in PACK if c['dt'] == dt]
    return rows + [c for c in rows if pack_blocks(c) == 1] + [c for c in rows if pack_blocks(c) >= 4][::-1]
