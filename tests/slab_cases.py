"""Case tables of tests/test_slab_envelope_gpu.py and tests/test_slab_check_cpu.py: the smallest shapes at which each thing in the
slab kernels (csrc/enc_slab.hip, csrc/heads_slab.hip) can go wrong.

ENC (d_model 256, 8 heads): one row per (B, S) of {(1,1), (2,31), (1,32), (3,33), (2,64), (2,97), (1,127), (2,128)} - a lone token,
both sides of the 32-row slab edge, tail slabs behind one to three full ones, clips whose slab index needs blockIdx / SL with S % 32 != 0 -
plus a second S = 64 row.  FF in {512, 1024, 1536, 2048} (one hidden chunk; even and odd chunk counts = both phases of the
double-buffered hidden tile), each with a tail slab (nvalid < 32) and with a full slab.  p in {0, 0.1}.  Every row runs in training and in
inference.  kpm: tests/slab_check.kpm_pattern (none, a padded tail crossing a 32-key tile, scattered, key 0, a clip with a single live key,
padding that differs between the clips of a batch).  No row pads EVERY key of a clip: all its scores are -inf and there is no finite
reference.  kind: 'steps' (row magnitudes 4^-4 .. 4^4 with offsets) or 'mean100' (mean 100, std 0.05).

HEADS: (L, B, Qp) of {(1,1,1), (1,1,31), (1,1,32), (1,1,33), (1,2,32), (1,2,31), (2,3,11), (3,2,21)}: the audio-tag rows
((L - 1) B + b) Qp fall on the first row of a slab (rows 0, 32), on its last row (row 31) and in its middle (33, 44, 55; 84, 105);
(C1, CA) of {(1,0), (11,10), (16,16), (11,0), (16,1)}; g_at absent with CA > 0.  Every row also runs in inference (h1 / h2 null).
"""


def _enc(B, S, FF, p, kpm, kind='steps'):
    return dict(name=f'enc_b{B}_s{S}_ff{FF}_p{p}_{kpm or "nopad"}_{kind}', B=B, S=S, FF=FF, p=p, kpm=kpm, kind=kind)


ENC = [
    _enc(1, 1, 512, 0.1, None),
    _enc(2, 31, 1024, 0.1, 'differ'),
    _enc(1, 32, 512, 0.0, 'key0'),
    _enc(3, 33, 1536, 0.1, 'tail'),
    _enc(2, 64, 1536, 0.0, 'scattered'),
    _enc(2, 64, 512, 0.1, 'key0'),
    _enc(2, 97, 2048, 0.1, 'single'),
    _enc(1, 127, 1024, 0.1, 'scattered', 'mean100'),
    _enc(2, 128, 2048, 0.1, 'tail'),
    _enc(3, 33, 2048, 0.0, 'differ'),
]


def _heads(L, B, Qp, C1, CA, g_at=True):
    return dict(name=f'heads_l{L}_b{B}_q{Qp}_c{C1}_a{CA}' + ('' if g_at or not CA else '_nogat'), L=L, B=B, Qp=Qp, C1=C1, CA=CA, g_at=g_at)


HEADS = [
    _heads(1, 1, 1, 1, 0),
    _heads(1, 1, 31, 11, 10),
    _heads(1, 1, 32, 16, 16),
    _heads(1, 1, 33, 11, 0),
    _heads(1, 2, 32, 16, 1),
    _heads(1, 2, 31, 11, 10),
    _heads(2, 3, 11, 16, 16),
    _heads(3, 2, 21, 11, 10, g_at=False),
    _heads(2, 3, 11, 1, 0),
    _heads(1, 2, 31, 16, 1, g_at=False),
]

# refused calls (tests/test_slab_envelope_gpu.py): what is changed in an otherwise valid call
ENC_REFUSALS = [dict(S=0), dict(S=129), dict(FF=256), dict(FF=768), dict(p=1.0), dict(partial=True)]
HEADS_REFUSALS = [dict(C1=0), dict(C1=17), dict(CA=17), dict(wa_null=True), dict(h1_only=True)]
