"""Rows for tests/test_update_envelope_gpu.py and tests/test_update_check_cpu.py: the chunk tables handed to the clip / AdamW / EMA /
gradient-gather kernels of csrc/misc.hip.  A row is ONE launch (one table); a chunk is (n, byte offsets of its tensors inside their
16-byte aligned NaN-filled buffers, bf16 flag, lr, wd).  Every row is run whole: nothing is sampled.

Lengths: 1 (one lane), 3 / 5 / 7 / 9 (n & 3 and n & 7 tails around one vector), 4 / 8 (no tail), 1023 / 1024 / 1025 (one pass of 256
lanes x float4 and its two neighbours), 4097 (several passes and a tail), 65535 / 65536 (the largest chunk the host tables build).
multi_sumsq adds n4 = n >> 2 in {767, 768, 769, 1023, 1024, 1025}: its four-loads-in-flight loop runs while i + 3 * 256 < n4, so lane 0
enters it from n4 = 769 and lane 255 from n4 = 1024; each with n & 3 in {0, 3}.  multi_gather splits a chunk over 8 workgroups of
per = roundup8(ceil(n / 8)) elements: 1 / 7 / 8 (one workgroup, seven empty), 9 (8 + 1), 56 / 57 / 63 / 64 / 65 (per = 8: seven or eight
workgroups, then per = 16), 16383 / 16384 / 16385 (per = 2048 and 2056: a tail in the last workgroup), 65535 / 65536.

Offsets (bytes from a 16-byte boundary).  The f32 kernels vectorise only when EVERY pointer of the chunk is 16-byte aligned, so each
of p, g, m, v is misaligned alone (+4, +8, +4, +12), then all four.  A bf16 gradient is read 8 bytes at a time by multi_adamw (needs
g % 8 == 0) and 16 bytes at a time by multi_sumsq (g % 16 == 0): +0 vectorises both, +8 only multi_adamw, +2 neither.
"""

LEN = (1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4097, 65535, 65536)
LEN_SUMSQ = LEN + tuple(4 * n4 + r for n4 in (767, 768, 769, 1023, 1024, 1025) for r in (0, 3))
LEN_GATHER = (1, 7, 8, 9, 56, 57, 63, 64, 65, 16383, 16384, 16385, 65535, 65536)
LEN_CORE = (1, 5, 8, 1025, 4097)

# (name, (p, g, m, v) byte offsets, bf16 gradient)
ALIGN_ADAMW = (('a', (0, 0, 0, 0), False), ('p4', (4, 0, 0, 0), False), ('g8', (0, 8, 0, 0), False), ('m4', (0, 0, 4, 0), False),
               ('v12', (0, 0, 0, 12), False), ('all', (4, 8, 12, 4), False),
               ('bf0', (0, 0, 0, 0), True), ('bf2', (0, 2, 0, 0), True), ('bf8', (0, 8, 0, 0), True), ('bf0_p4', (4, 0, 0, 0), True))
ALIGN_CORE = tuple(a for a in ALIGN_ADAMW if a[0] in ('a', 'all', 'bf2', 'bf8'))
ALIGN_SUMSQ = (('a', 0, False), ('g4', 4, False), ('g8', 8, False), ('g12', 12, False), ('bf0', 0, True), ('bf2', 2, True), ('bf8', 8, True))
# (name, (p, shadow) byte offsets)
ALIGN_EMA = (('a', (0, 0)), ('p4', (4, 0)), ('s8', (0, 8)), ('both', (12, 4)))
# (name, (source, destination) byte offsets); the destination is f32 (modes 0, 1) or bf16 (modes 2, 3)
ALIGN_GATHER_F32 = (('a', (0, 0)), ('s4', (4, 0)), ('d8', (0, 8)), ('both', (12, 4)))
ALIGN_GATHER_BF = (('a', (0, 0)), ('s4', (4, 0)), ('d2', (0, 2)), ('d8', (0, 8)), ('both', (8, 2)))

LR, WD = 1e-3, 1e-2
# per-chunk (lr, wd), cycled over the chunks of a table: the default pair, wd = 0, lr = 0 (p must keep its bits), 3 x lr
HYPER = ((LR, WD), (LR, 0.0), (0.0, WD), (3 * LR, WD))
BETAS, EPS = (0.9, 0.999), 1e-8
EMA_DEFAULT = 0.9996                 # the decay the benchmark and the semi-supervised tests train with
EMA_DECAYS = (0.0, 1.0, 0.999, EMA_DEFAULT)
STEPS = (1, 2, 3, 10, 1000, 100000)


def _chunks(lens, aligns):
    out = []
    for a, offs, bf in aligns:
        for n in lens:
            lr, wd = HYPER[len(out) % len(HYPER)]
            out.append(dict(n=n, off=tuple(offs), bf=bf, lr=lr, wd=wd, tag=f'{a}_n{n}'))
    return out


def _adamw(name, lens, aligns, step, max_norm, gscale=1.0, moments='nonzero'):
    """max_norm None: no clipping and a NULL sumsq pointer; gscale 0: all-zero gradients"""
    return dict(name=name, kind='adamw', chunks=_chunks(lens, aligns), step=step, max_norm=max_norm, gscale=gscale, moments=moments)


ADAMW = [
    # the mixed table: every length x every alignment, f32 and bf16 gradients, per-chunk lr / wd; first step, clipped
    _adamw('adamw_full_step1_clip', LEN, ALIGN_ADAMW, 1, 0.1, moments='zero'),
    # the same chunks with moments in place, no clipping, null sumsq (the table-order row)
    _adamw('adamw_full_step3_noclip', LEN, ALIGN_ADAMW, 3, None),
] + [
    _adamw(f'adamw_core_step{s}_clip', LEN_CORE, ALIGN_CORE, s, 0.1, moments='zero' if s == 1 else 'nonzero') for s in STEPS
] + [
    # the norm (about 1e-4) is below max_norm: the coefficient is exactly 1, the result equals the unclipped launch bit for bit
    _adamw('adamw_core_step2_below', LEN_CORE, ALIGN_CORE, 2, 0.1, gscale=1e-6),
    _adamw('adamw_core_step1_below_zero_moments', LEN_CORE, ALIGN_CORE, 1, 0.1, gscale=1e-6, moments='zero'),
    # all-zero gradients with clipping on: sumsq = 0, coef = min(1, 0.1 / 1e-6) = 1; with zero moments v = 0 and g = 0 (denominator eps)
    _adamw('adamw_core_step1_zero_grad_zero_moments', LEN_CORE, ALIGN_CORE, 1, 0.1, gscale=0.0, moments='zero'),
    _adamw('adamw_core_step10_zero_grad', LEN_CORE, ALIGN_CORE, 10, 0.1, gscale=0.0),
]
BELOW = ('adamw_core_step2_below', 'adamw_core_step1_below_zero_moments')

SUMSQ = [dict(name='sumsq_full', kind='sumsq', gscale=1.0,
              chunks=[dict(n=n, off=(0, o, 0, 0), bf=bf, lr=0.0, wd=0.0, tag=f'{a}_n{n}') for a, o, bf in ALIGN_SUMSQ for n in LEN_SUMSQ]),
         dict(name='sumsq_core_1e-6', kind='sumsq', gscale=1e-6,
              chunks=[dict(n=n, off=(0, o, 0, 0), bf=bf, lr=0.0, wd=0.0, tag=f'{a}_n{n}') for a, o, bf in ALIGN_SUMSQ for n in LEN_CORE])]

EMA = [dict(name=f'ema_decay{d}', kind='ema', decay=d,
            chunks=[dict(n=n, off=(o[0], 0, o[1], 0), bf=False, lr=0.0, wd=0.0, tag=f'{a}_n{n}') for a, o in ALIGN_EMA for n in LEN])
       for d in EMA_DECAYS]

GATHER = [dict(name=f'gather_mode{mode}', kind='gather', mode=mode,
               chunks=[dict(n=n, off=(o[1], o[0], 0, 0), bf=bool(mode & 2), lr=0.0, wd=0.0, tag=f'{a}_n{n}')
                       for a, o in (ALIGN_GATHER_BF if mode & 2 else ALIGN_GATHER_F32) for n in LEN_GATHER])
          for mode in (0, 1, 2, 3)]

# single-tensor entry points
SUMSQ1_N = (1, 2047, 2048, 2049, 1024 * 2048 + 2049)           # the last: above the 1024-part cap, the grid-stride loop runs twice
ADAMW1_N = (1, 255, 256, 257)

# the guard / step-word / seed-word rows of multi_sumsq: (name, what the gradient holds, guard before (None: null pointer),
# guard must be up afterwards, the step word must advance)
GUARD_ROWS = (
    ('finite', 'finite', 0, False, True),
    ('one_inf', 'inf', 0, True, False),
    ('one_nan', 'nan', 0, True, False),
    ('finite_1e20', '1e20', 0, True, False),                  # every element finite, every square infinite
    ('overflow_in_sum', 'sum_overflow', 0, True, False),      # every square and every partial finite, their sum infinite
    ('total_2.9e38', '2.9e38', 0, False, True),
    ('sticky', 'finite', 1, True, False),                     # already up: stays up on a finite norm, the step word stays
    ('null_guard_finite', 'finite', None, False, True),
    ('null_guard_inf', 'inf', None, False, True),             # nothing to consult: the step word always advances
)

ALL = ADAMW + SUMSQ + EMA + GATHER
