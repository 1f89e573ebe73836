"""The rows of tests/test_input_envelope_gpu.py and tests/test_input_check_cpu.py: the seven kernels of csrc/input.hip at their band,
frame, wave and LDS edges.  Importable without a GPU; nothing here is sampled: every row listed runs.

A row is a dict with a 'name', the entry it is driven through ('via': 'ops' = the Python class or op, 'c' = the C entry point via
lib.load(), where the Python layer cannot express the case) and the 'edge' it is there for.  CASES maps a kernel key (the keys of
input_check.KERNELS) to its rows.  The numbers a row is chosen for - G, idle threads, trips per thread, LDS bytes, clips per wave, boxes
per lane, float4 per block - are functions of the row at the end of the module, so that tests/test_input_check_cpu.py can assert that
each table reaches the edge it names.

Augmentation records are (nframes_raw, tm_t, tm_t0, fm_f, fm_f0, fm_on, fs_shift), the field order of utilities.transforms._AUG.

query_patches: a constant crop gives range = 0 and 0 / 0 in the reference as well (the reference divides by max - min too), so no row
has one: every crop is cut from continuous random data.
"""
LDS_MAX = 160 * 1024
THREADS = 1024
FS = (2, 40, 64, 128, 1024)
MAX_BAND = 4                                   # FreqShift's default max_band (utilities.transforms.DeviceBoxTransform fs=)
MODES4 = ((1, 1), (0, 0), (1, 0), (0, 1))      # (apply_log, mean/std given)
MODES2 = ((1, 1), (0, 0))


def rec(nraw, tm=(0, 0), fm=(0, 0, 0), sh=0):
    """tm = (t0, t), fm = (on, f0, f) -> a record in _AUG order"""
    return (nraw, tm[1], tm[0], fm[2], fm[1], fm[0], sh)


def _expand(rows, modes_of):
    out = []
    for r in rows:
        for log, norm in modes_of(r):
            q = dict(r, log=log, norm=norm)
            q['name'] = f"{r['name']}_log{log}_norm{norm}"
            out.append(q)
    names = [r['name'] for r in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


# ------------------------------------------------------------------------------------------------ box_transform
_FR = {2: 37, 40: 30, 64: 20, 128: 11, 1024: 39}           # frames per F of the band rows (F = 1024 needs frames <= 39)


def _bt_bands(F):
    fr, q = _FR[F], max(1, F // 4)
    return dict(name=f'bt_F{F}', edge='F', via='ops', F=F, frames=fr, modes=4,
                recs=[rec(fr - 1, tm=(fr - 3, 3), fm=(1, F - q, q), sh=1), rec(fr + 2, fm=(1, 0, 1), sh=-1), rec(fr, tm=(0, 2), sh=0)])


_BT = [_bt_bands(F) for F in FS] + [
    dict(name=f'bt_elems_{fr}x64', edge='elements', via='ops', F=64, frames=fr, recs=[rec(fr, fm=(1, 3, 5), sh=2), rec(fr + 1), rec(fr - 1, tm=(1, 2))])
    for fr in (15, 16, 17)] + [
    dict(name='bt_1frame_F64', edge='frames1', via='ops', F=64, frames=1, recs=[rec(1, fm=(1, 60, 4)), rec(0), rec(2, sh=-3)]),
    dict(name='bt_1frame_F1024', edge='frames1', via='ops', F=1024, frames=1, recs=[rec(1, fm=(1, 0, 7), sh=5), rec(3)]),
    dict(name='bt_nraw_F40', edge='nraw', via='ops', F=40, frames=30,
         recs=[rec(0), rec(1, fm=(1, 2, 9)), rec(29, sh=3), rec(30, tm=(5, 4)), rec(31, fm=(1, 30, 10), sh=-2), rec(60, tm=(28, 2))]),
    dict(name='bt_nraw_F64', edge='nraw', via='ops', F=64, frames=20,
         recs=[rec(0, fm=(1, 0, 3)), rec(1), rec(19), rec(20), rec(21, fm=(1, 10, 3)), rec(40, sh=1)]),
    dict(name='bt_time_mask', edge='tm', via='ops', F=64, frames=20,
         recs=[rec(20, tm=(13, 7)), rec(10, tm=(12, 5)), rec(20, tm=(5, 0)), rec(25, tm=(0, 20)), rec(10, tm=(8, 6), fm=(1, 7, 20))]),
    dict(name='bt_freq_mask', edge='fm', via='ops', F=64, frames=20,
         recs=[rec(20, fm=(1, 41, 23)), rec(18, fm=(1, 0, 64)), rec(20, fm=(1, 9, 0)), rec(20, fm=(0, 3, 5)), rec(22, fm=(1, 63, 1), tm=(2, 3))]),
    dict(name='bt_const_fill', edge='const_fill', via='c', F=40, frames=30, fill_mean=0, fill_const=-3.5,
         recs=[rec(30, fm=(1, 35, 5)), rec(12, fm=(1, 0, 40)), rec(31, fm=(1, 7, 0)), rec(30, fm=(0, 3, 5)), rec(30, fm=(1, 11, 13), sh=-7)]),
    dict(name='bt_shift_F40', edge='shift', via='ops', F=40, frames=30, recs=[rec(30 + (s % 3) - 1, sh=s, fm=(1, 36, 4)) for s in (-39, -1, 0, 1, 39)]),
    dict(name='bt_shift_F64', edge='shift', via='ops', F=64, frames=20, recs=[rec(20, sh=s) for s in (-MAX_BAND, MAX_BAND, -63, 63)]),
    dict(name='bt_silence', edge='silence', via='ops', F=64, frames=20, silent_clips=(0,), silent_bands={1: (17,), 2: (0, 63)},
         recs=[rec(20, fm=(1, 4, 9)), rec(20, fm=(1, 15, 5)), rec(25, sh=1)]),
    dict(name='bt_lds_639x64', edge='lds', via='ops', F=64, frames=639, recs=[rec(641, fm=(1, 50, 14), sh=-1), rec(639, tm=(630, 9), fm=(1, 0, 64))]),
    dict(name='bt_lds_640x64_refused', edge='lds', via='ops', F=64, frames=640, refuse=True, recs=[rec(640)]),
]
BOX_TRANSFORM = _expand(_BT, lambda r: MODES4 if r.get('modes') == 4 else (((1, 1),) if r.get('refuse') or r['frames'] > 600 else MODES2))


# ------------------------------------------------------------------------------------------------ box_transform_views
# recs: per clip (view 0 record, view 1 record, noise_on); both views carry the same nframes_raw
def vrec(nraw, on, fm0=(0, 0, 0), sh0=0, tm1=(0, 0), fm1=(0, 0, 0), sh1=0):
    return (rec(nraw, fm=fm0, sh=sh0), rec(nraw, tm=tm1, fm=fm1, sh=sh1), on)


_VFR = {2: 520, 40: 30, 64: 20, 128: 11, 1024: 3}


def _bv_bands(F):
    fr, G, q = _VFR[F], THREADS // F, max(1, F // 4)
    ns = (1, G - 1, G, G + 1)
    return dict(name=f'bv_F{F}', edge='F', via='ops', F=F, frames=fr,
                recs=[vrec(n, 1, fm0=(1, 0, q), sh0=1, tm1=(min(i, fr - 1), 1), fm1=(1, F - q, q), sh1=-1) for i, n in enumerate(ns)])


_BV = [_bv_bands(F) for F in FS] + [
    dict(name='bv_nel_2048', edge='pair_loop', via='ops', F=2, frames=1030, recs=[vrec(n, 1, fm0=(1, 1, 1), sh1=1, tm1=(1000, 30)) for n in (1023, 1024, 1025)]),
    dict(name='bv_noise_all0', edge='noise_on', via='ops', F=64, frames=20, recs=[vrec(n, 0, sh0=2, fm1=(1, 3, 9), tm1=(2, 5)) for n in (19, 22, 20)]),
    dict(name='bv_noise_all1', edge='noise_on', via='ops', F=64, frames=20, recs=[vrec(n, 1, sh0=2, fm1=(1, 3, 9), tm1=(2, 5)) for n in (19, 22, 20)]),
    dict(name='bv_noise_alt', edge='noise_on', via='ops', F=64, frames=20,
         recs=[vrec(n, i % 2, fm0=(1, 60, 4), sh0=-2, fm1=(1, 3, 9), sh1=3, tm1=(17, 3)) for i, n in enumerate((19, 22, 20, 40))]),
    dict(name='bv_zero_band', edge='zero_band', via='ops', F=64, frames=20, silent_bands={0: (5,), 1: (0, 63)}, recs=[vrec(20, 1), vrec(23, 1, sh1=1)]),
    dict(name='bv_const_fill', edge='const_fill', via='c', F=40, frames=30, fill_mean=0, fill_const=-3.5,
         recs=[vrec(30, 1, fm0=(1, 35, 5), fm1=(1, 0, 3)), vrec(12, 0, fm0=(1, 0, 40), fm1=(1, 1, 1))]),
    dict(name='bv_lds_622x64', edge='lds', via='ops', F=64, frames=622, recs=[vrec(624, 1, fm0=(1, 0, 64), fm1=(1, 50, 14), sh1=-1), vrec(622, 1, tm1=(600, 22))]),
    dict(name='bv_lds_623x64_refused', edge='lds', via='ops', F=64, frames=623, refuse=True, recs=[vrec(623, 1)]),
    dict(name='bv_drawn_F40', edge='drawn', via='ops', F=40, frames=30, drawn=True, offset=123456, seed=0xC0FFEE, extra_stride=5,
         recs=[vrec(26, 1, fm0=(1, 4, 4), sh1=1), vrec(31, 0, sh0=-1), vrec(29, 1, tm1=(3, 4), fm1=(1, 30, 10))]),
]
BOX_TRANSFORM_VIEWS = _expand(_BV, lambda r: ((1, 1),) if r.get('refuse') or r['frames'] > 600 or r.get('drawn') else MODES2)


# ------------------------------------------------------------------------------------------------ scaler_update
# calls: the batches of nframes_raw handed to successive sedt_scaler_update calls on the same accumulators (which start non-zero);
# the concatenation of the calls is run as one call too and must give the same bits.  All rows go through the C entry point: the
# Scaler class owns its accumulators (they start at zero, outside any guard frame) and refuses row counts outside the batch.
_SFR = {2: 37, 40: 30, 64: 20, 128: 11, 1024: 5}
_SC = [dict(name=f'sc_F{F}', edge='F', via='c', F=F, frames=_SFR[F],
            calls=[[0, 1, _SFR[F] - 1], [_SFR[F], _SFR[F] + 1, 2 * _SFR[F]]]) for F in FS] + [
    dict(name='sc_groups_F40', edge='nraw', via='c', F=40, frames=30, calls=[[24, 25, 26], [1, 0]]),
    dict(name='sc_clamp', edge='clamp', via='c', F=64, frames=20, raw_stride=23, calls=[[-3, 28, 20], [2 ** 31 - 1, -2 ** 31]]),
    dict(name='sc_B1', edge='B', via='c', F=64, frames=20, calls=[[21], [17]]),
    dict(name='sc_B2', edge='B', via='c', F=64, frames=20, calls=[[21, 3], [17, 20]]),
    dict(name='sc_B5', edge='B', via='c', F=64, frames=20, calls=[[21, 3, 20, 19, 40], [17, 20, 1, 22, 5]]),
    dict(name='sc_lds_575x64', edge='lds', via='c', F=64, frames=575, calls=[[577], [575]]),
    dict(name='sc_lds_576x64_refused', edge='lds', via='c', F=64, frames=576, refuse=True, calls=[[576]]),
]
SCALER = _expand(_SC, lambda r: ((1, 1),) if r.get('refuse') or r['frames'] > 500 else ((1, 0), (0, 0)))       # (norm is unused)


# ------------------------------------------------------------------------------------------------ mixup
# jobs: (src1, src2, mode, lam) per output clip; x1 and x2 hold three clips each
_JOBS = [(2, 1, 0, 0.37), (0, 1, 1, 0.0), (1, 0, 2, 0.0), (2, 0, 0, 0.0), (1, 2, 0, 1.0), (2, 2, 1, 0.5), (0, 0, 2, 0.5)]
MIX_C4 = (1, 255, 256, 257, 64 * 256, 64 * 256 + 1, 2 * 64 * 256 + 5)
MIXUP = [dict(name=f'mix_c4_{n}', edge='c4', via='ops', clip4=n, rem=0, jobs=_JOBS) for n in MIX_C4] + [
    dict(name='mix_one_job', edge='jobs', via='c', clip4=257, rem=0, jobs=[(1, 2, 0, 0.37)]),
    dict(name='mix_n_out_0', edge='n_out0', via='c', clip4=256, rem=0, jobs=[]),
    dict(name='mix_elems_not_x4_refused', edge='refuse', via='c', clip4=1, rem=2, jobs=_JOBS[:1], refuse=True),
]


# ------------------------------------------------------------------------------------------------ mixup_targets
# A row builds its targets in input_check.MixupTargets.make from these fields:
#   B1, ns1 (table value), split (the split1 device word, or None), B2, mix_num, max_events, max_targets (cap = B2 * max_targets unless
#   'cap' is given as an offset to the merged total), ratio1 / ratio_out present, and 'design': clip index -> a named pair of targets.
def _mt(name, edge, B1, B2, mix_num, ns1=None, split=None, max_events=20, max_targets=20, ratio1=1, ratio_out=1, cap=None, design=None):
    return dict(name=name, edge=edge, via='c', B1=B1, ns1=B1 if ns1 is None else ns1, split=split, B2=B2, mix_num=mix_num, max_events=max_events,
                max_targets=max_targets, ratio1=ratio1, ratio_out=ratio_out, cap=cap, design=design or {})


MT_B2 = (1, 15, 16, 17, 33, 70)
MT_NBOX = (63, 64, 65, 130)
MIXUP_TARGETS = [_mt(f'mt_B2_{b}', 'B2', B1=b, B2=b, mix_num=b, design={b - 1: 'touch'} if b > 1 else {}) for b in MT_B2] + \
    [_mt(f'mt_nbox_{n}', 'nbox', B1=3, B2=3, mix_num=3, max_events=n, max_targets=n, design={1: ('many', n), 2: ('many_clash_last', n)}) for n in MT_NBOX] + [
    _mt('mt_max_events', 'max_events', B1=6, B2=6, mix_num=6, max_events=6,
        design={0: ('count', 6, 0), 1: ('count', 7, 0), 2: ('count', 3, 3), 3: ('count', 3, 4), 4: ('count', 0, 6), 5: ('count', 0, 7)}),
    _mt('mt_touch', 'touch', B1=5, B2=5, mix_num=5, design={0: 'touch', 1: 'ulp_apart', 2: 'other_class_overlap', 3: 'touch_reversed', 4: 'overlap'}),
    _mt('mt_weak', 'weak', B1=6, B2=6, mix_num=6, ns1=3, design={4: 'weak_first', 5: 'weak_plain'}),
    _mt('mt_split', 'split', B1=6, B2=6, mix_num=6, ns1=5, split=2, design={3: 'weak_first'}),
    _mt('mt_split_above', 'split', B1=6, B2=6, mix_num=6, ns1=3, split=5, design={4: 'weak_first'}),
    _mt('mt_mix0', 'mix_num', B1=0, B2=5, mix_num=0),
    _mt('mt_mix0_B1', 'mix_num', B1=4, B2=5, mix_num=0),
    _mt('mt_mix_all', 'mix_num', B1=18, B2=18, mix_num=18, design={17: 'overlap', 16: 'touch'}),
    _mt('mt_cap_short', 'cap', B1=5, B2=7, mix_num=5, cap=-1, design={0: 'touch'}),
    _mt('mt_cap_exact', 'cap', B1=5, B2=7, mix_num=5, cap=0, design={0: 'touch'}),
    _mt('mt_no_ratio1', 'ratio', B1=5, B2=6, mix_num=4, ratio1=0, design={1: 'overlap'}),
    _mt('mt_no_ratio_out', 'ratio', B1=5, B2=6, mix_num=4, ratio_out=0, design={1: 'overlap'}),
    _mt('mt_no_ratios', 'ratio', B1=5, B2=6, mix_num=4, ratio1=0, ratio_out=0, design={1: 'overlap'}),
]


# ------------------------------------------------------------------------------------------------ query_patches
# jobs: (clip, s_idx, e_idx)
def _qp_jobs(T, hs, B=2):
    jobs = []
    for i, h in enumerate(hs):
        jobs.append((i % B, 0, h))
        jobs.append(((i + 1) % B, T - h, T))
        if 2 * h < T:
            jobs.append((i % B, (T - h) // 2, (T - h) // 2 + h))
    return jobs


QP_H = (1, 2, 3, 127, 128, 129, 255, 256)
QUERY = [
    dict(name='qp_F64_T300', edge='h', via='c', B=2, T=300, F=64, fixed=0, jobs=_qp_jobs(300, QP_H + (300,))),
    dict(name='qp_F24_T140', edge='F', via='c', B=2, T=140, F=24, fixed=0, jobs=_qp_jobs(140, (1, 2, 3, 127, 128, 129, 140))),
    dict(name='qp_F8_T260', edge='F', via='c', B=3, T=260, F=8, fixed=0, jobs=_qp_jobs(260, QP_H + (260,), B=3)),
    dict(name='qp_fixed', edge='fixed', via='c', B=2, T=300, F=64, fixed=1, jobs=[(0, 0, 128), (1, 172, 300), (1, 0, 128), (0, 172, 300), (0, 57, 185)]),
    dict(name='qp_fixed_F24', edge='fixed', via='c', B=2, T=128, F=24, fixed=1, jobs=[(1, 0, 128), (0, 0, 128)]),
    dict(name='qp_ops', edge='ops', via='ops', B=2, T=300, F=64, fixed=0, jobs=[(0, 30, 90), (0, 100, 228), (1, 7, 290), (1, 150, 151)]),
    dict(name='qp_none', edge='n0', via='c', B=1, T=140, F=24, fixed=0, jobs=[]),
    dict(name='qp_lds_2558x64', edge='lds', via='c', B=1, T=2558, F=64, fixed=0, jobs=[(0, 0, 2558), (0, 2557, 2558), (0, 1200, 1328)]),
    dict(name='qp_lds_2559x64_refused', edge='lds', via='c', B=1, T=2559, F=64, fixed=0, refuse=True, jobs=[(0, 0, 128)]),
]

CASES = dict(box_transform=BOX_TRANSFORM, box_transform_views=BOX_TRANSFORM_VIEWS, scaler_update=SCALER, mixup=MIXUP,
             mixup_targets=MIXUP_TARGETS, query_patches=QUERY)


# ------------------------------------------------------------------------------------------------ what a row reaches
def groups(F):
    """G: the row groups the 1024 threads of a workgroup form over F bands (csrc/input.hip: G = 1024 / F)"""
    return THREADS // F


def idle_threads(F):
    """threads with g >= G in the band-sum loops"""
    return THREADS - groups(F) * F


def trips(n, per=THREADS):
    """trips of the busiest thread of a stride-`per` loop over n elements"""
    return (n + per - 1) // per


def rows_per_group(nraw, F):
    """rows the busiest (g, c) thread adds in a band sum"""
    return trips(max(nraw, 0), groups(F))


def raw_stride(c):
    """rows between two clips of the raw batch: the issue's max nraw + 3 unless the row sets it"""
    if 'raw_stride' in c:
        return c['raw_stride']
    if 'calls' in c:
        n = max(max(b) for b in c['calls'])
    elif isinstance(c['recs'][0][0], tuple):
        n = max(r[0][0] for r in c['recs'])
    else:
        n = max(r[0] for r in c['recs'])
    return max(n, 1) + c.get('extra_stride', 3)


def lds_box_transform(frames, F):
    return (frames * F + 16) * 4


def lds_views(frames, F):
    return (frames * F + 16 + F + groups(F) * F) * 4


def lds_scaler(frames, F):
    return 2 * groups(F) * F * 8 + (frames * F + 16) * 4


def lds_query(T, F):
    return ((T * F + 15) & ~15) + 32 * 4


def query_scratch_offset(h, F):
    """byte offset of the reduction scratch behind an h x F crop of 8-bit codes"""
    return (h * F + 15) & ~15


def mix_grid_x(clip4):
    return min((clip4 + 255) // 256, 64)


def mix_trips(clip4):
    """grid-stride trips of the busiest thread of mixup_kernel"""
    return trips(clip4, mix_grid_x(clip4) * 256)


def clips_per_wave(B2):
    """unlabelled clips the busiest of the 16 waves of mixup_targets_kernel takes"""
    return (B2 + 15) // 16


def boxes_per_lane(n):
    """candidate boxes the busiest lane of a wave checks"""
    return (n + 63) // 64
