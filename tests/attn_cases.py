"""Case tables of tests/test_attn_ln_envelope_gpu.py (resolved on the host by tests/test_attn_check_cpu.py).

ATTN: one row per attention case.  `fwd` / `bwd` name the kernel instance sedt_attention_fwd / sedt_attention_bwd must reach for the
row's layout (as sedt_attention_describe prints it); bwd = '' means the backward must be REFUSED (an error return, no launch).

  dt       'bf16' | 'f32'
  B, H     clips, heads (B in {1, 3, 5}, H in {8, 3, 1})
  Lq, Lk   lengths - both sides of every 32-tile edge of the MFMA kernels
  kpm      None | 'tail' (the last 5 + b keys of clip b; needs Lk > 9) | 'one' (all but key (7 b + 3) % Lk padded) |
           'tiles' (whole 32-key tiles emptied: keys >= 32 of even clips, keys < 32 (b + 1) of odd clips... see kpm_pattern) |
           'mid' (keys Lk/3 .. Lk/2 + b)
  amask    additive [Lq, Lk] mask: finite values in +-3 and -inf (every row keeps a live key)
  p        dropout probability (0, 0.1, 0.5)
  gain     standard deviation of q and k (1, 3)
  layout   'packed'  q | k column halves of one 512-wide buffer, v its own; o and the gradients inside wider buffers
           'stride'  row strides the MFMA kernels refuse (not a multiple of 8 bf16 / 4 f32 elements) -> the generic kernels
           'o_off'   an o view that starts 8 bytes into its allocation (not 16-byte aligned): the bf16 backward and both f32
                     kernels read / write o as 16-byte vectors and must step aside

LN: LayerNorm rows (dt, D, rows, input kind, which optional tensors).
"""

def _b(x):
    return 'true' if x else 'false'


def _row(name, dt, B, H, Lq, Lk, kpm=None, amask=False, p=0.0, gain=1, layout='packed', fwd=None, bwd=None):
    return dict(name=name, dt=dt, B=B, H=H, Lq=Lq, Lk=Lk, kpm=kpm, amask=amask, p=p, gain=gain, layout=layout, fwd=fwd, bwd=bwd)


def _fwd16(Lk, am):
    return f'attn_fwd_mfma_kernel<{(Lk + 31) // 32}, {_b(am)}>'


def _bwd16(Lq, Lk, am):
    return f'attn_bwd_mfma_kernel<{(Lq + 31) // 32}, {(Lk + 31) // 32}, {_b(am)}>'


def _fwd32(Lk, am, p):
    return f'attn_f32_fwd_kernel<{1 if Lk <= 32 else 4}, {_b(am)}, {_b(p > 0)}>'


def _bwd32(Lq, Lk, am, p):
    return f'attn_f32_bwd_kernel<{1 if Lq <= 32 else 4}, {1 if Lk <= 32 else 4}, {_b(am)}, {_b(p > 0)}>'


GEN_F16, GEN_B16, GEN_F32, GEN_B32 = 'attn_fwd_kernel<__bf16>', 'attn_bwd_kernel<__bf16>', 'attn_fwd_kernel<float>', 'attn_bwd_kernel<float>'

_SHAPES = ((1, 8), (3, 3), (5, 1), (3, 8), (1, 3), (5, 3))
_KPM = (None, 'tail', 'mid', 'tiles', 'one')
_P = (0.0, 0.1, 0.5)


def _bf16_rows():
    out = []
    # the backward's 4 x 4 tile grid (1 to 4 waves), both mask instantiations; the lengths walk the tile edges +-1
    lq_of = {1: (1, 11, 21, 32), 2: (33, 64), 3: (65, 96), 4: (97, 127, 128)}
    lk_of = {1: (1, 31, 32), 2: (33, 64), 3: (65, 96), 4: (97, 127, 128)}
    n = 0
    for ntq in (1, 2, 3, 4):
        for ntk in (1, 2, 3, 4):
            for am in (False, True):
                Lq, Lk = lq_of[ntq][n % len(lq_of[ntq])], lk_of[ntk][(n // 2) % len(lk_of[ntk])]
                B, H = _SHAPES[n % len(_SHAPES)]
                kpm = _KPM[n % len(_KPM)]
                if Lk <= 9 and kpm in ('tail', 'mid', 'tiles'):
                    kpm = None if Lk == 1 else 'one'
                if kpm == 'tiles' and Lk <= 32:
                    kpm = 'tail'
                out.append(_row(f'bf16_q{Lq}_k{Lk}_{"am" if am else "na"}', 'bf16', B, H, Lq, Lk, kpm, am, _P[n % 3], 3 if n % 4 == 1 else 1,
                                fwd=_fwd16(Lk, am), bwd=_bwd16(Lq, Lk, am)))
                n += 1
    # the forward's key tiles 5..8 (the backward is generic above 128 keys / queries), both mask instantiations
    for n, Lk in enumerate((129, 160, 161, 192, 193, 224, 225, 255, 256)):
        for am in ((False, True) if Lk in (129, 161, 193, 225) else (bool(n % 2),)):
            B, H = _SHAPES[(n + am) % len(_SHAPES)]
            Lq = (21, 11, 128, 33, 1, 65, 127, 97, 64)[n]
            out.append(_row(f'bf16_q{Lq}_k{Lk}_{"am" if am else "na"}', 'bf16', B, H, Lq, Lk, _KPM[(n + 1) % len(_KPM)], am, _P[(n + am) % 3],
                            fwd=_fwd16(Lk, am), bwd=GEN_B16))
    out += [
        # more edge lengths of the decoder (Q = 11 / 21 queries, odd element indices under dropout) and the encoder (S = 124 / 128)
        _row('bf16_dec_self_q11', 'bf16', 5, 8, 11, 11, None, True, 0.1, fwd=_fwd16(11, True), bwd=_bwd16(11, 11, True)),
        _row('bf16_dec_self_q21', 'bf16', 3, 8, 21, 21, None, False, 0.5, fwd=_fwd16(21, False), bwd=_bwd16(21, 21, False)),
        _row('bf16_dec_cross_q21_k127', 'bf16', 3, 8, 21, 127, 'tail', False, 0.1, fwd=_fwd16(127, False), bwd=_bwd16(21, 127, False)),
        _row('bf16_enc_s124', 'bf16', 3, 8, 124, 124, 'tiles', False, 0.1, gain=3, fwd=_fwd16(124, False), bwd=_bwd16(124, 124, False)),
        _row('bf16_q128_k97_one', 'bf16', 5, 3, 128, 97, 'one', True, 0.0, fwd=_fwd16(97, True), bwd=_bwd16(128, 97, True)),
        _row('bf16_q64_k33_tiles', 'bf16', 5, 3, 64, 33, 'tiles', False, 0.1, fwd=_fwd16(33, False), bwd=_bwd16(64, 33, False)),
        _row('bf16_q96_k96_mid', 'bf16', 3, 3, 96, 96, 'mid', True, 0.5, gain=3, fwd=_fwd16(96, True), bwd=_bwd16(96, 96, True)),
        # the generic kernels by size ...
        _row('bf16_gen_q129_k129', 'bf16', 3, 3, 129, 129, 'mid', True, 0.1, fwd=_fwd16(129, True), bwd=GEN_B16),
        _row('bf16_gen_q257_k257', 'bf16', 1, 3, 257, 257, 'tail', False, 0.1, fwd=GEN_F16, bwd=GEN_B16),
        _row('bf16_gen_q11_k512', 'bf16', 3, 1, 11, 512, 'tiles', True, 0.5, fwd=GEN_F16, bwd=''),
        _row('bf16_gen_q256_k256', 'bf16', 1, 8, 256, 256, None, False, 0.0, fwd=_fwd16(256, False), bwd=GEN_B16),
        # ... by a row stride the MFMA paths refuse ...
        _row('bf16_gen_stride', 'bf16', 3, 3, 33, 65, 'tail', True, 0.1, layout='stride', fwd=GEN_F16, bwd=GEN_B16),
        # ... and by an o that is not 16-byte aligned: the forward writes o element by element and stays, the backward steps aside
        _row('bf16_o_off', 'bf16', 3, 8, 21, 124, 'tail', False, 0.1, layout='o_off', fwd=_fwd16(124, False), bwd=GEN_B16),
        # the refusal row: the backward at (512, 512) needs more LDS than a workgroup has
        _row('bf16_refuse_512', 'bf16', 1, 1, 512, 512, None, False, 0.0, fwd=GEN_F16, bwd=''),
    ]
    return out


def _f32_rows():
    out = []
    lq_of = {1: (1, 11, 21, 32), 4: (33, 65, 97, 128)}
    lk_of = {1: (1, 31, 32, 11), 4: (33, 64, 96, 127)}
    n = 0
    for nq in (1, 4):
        for nk in (1, 4):
            for am in (False, True):
                for p in (0.0, (0.1, 0.5)[n % 2]):
                    Lq, Lk = lq_of[nq][n % 4], lk_of[nk][(n // 2) % 4]
                    B, H = _SHAPES[n % len(_SHAPES)]
                    kpm = _KPM[(n + 2) % len(_KPM)]
                    if Lk <= 9 and kpm in ('tail', 'mid', 'tiles'):
                        kpm = None if Lk == 1 else 'one'
                    if kpm == 'tiles' and Lk <= 32:
                        kpm = 'tail'
                    out.append(_row(f'f32_q{Lq}_k{Lk}_{"am" if am else "na"}_p{p}', 'f32', B, H, Lq, Lk, kpm, am, p, 3 if n % 4 == 2 else 1,
                                    fwd=_fwd32(Lk, am, p), bwd=_bwd32(Lq, Lk, am, p)))
                    n += 1
    out += [
        _row('f32_enc_s128', 'f32', 3, 8, 128, 128, 'tiles', False, 0.1, fwd=_fwd32(128, False, 0.1), bwd=_bwd32(128, 128, False, 0.1)),
        _row('f32_dec_cross_q21_k124', 'f32', 3, 8, 21, 124, 'tail', False, 0.1, fwd=_fwd32(124, False, 0.1), bwd=_bwd32(21, 124, False, 0.1)),
        _row('f32_q65_k33_one', 'f32', 5, 3, 65, 33, 'one', True, 0.5, fwd=_fwd32(33, True, 0.5), bwd=_bwd32(65, 33, True, 0.5)),
        _row('f32_gen_q129_k129', 'f32', 3, 3, 129, 129, 'mid', True, 0.1, fwd=GEN_F32, bwd=GEN_B32),
        _row('f32_gen_q21_k129', 'f32', 1, 8, 21, 129, 'tail', False, 0.0, gain=3, fwd=GEN_F32, bwd=GEN_B32),
        _row('f32_gen_stride', 'f32', 3, 3, 33, 65, 'tail', True, 0.1, layout='stride', fwd=GEN_F32, bwd=GEN_B32),
        _row('f32_o_off', 'f32', 3, 8, 21, 124, 'tail', False, 0.1, layout='o_off', fwd=GEN_F32, bwd=GEN_B32),
        _row('f32_refuse_512', 'f32', 1, 1, 512, 512, None, False, 0.0, fwd=GEN_F32, bwd=''),
    ]
    return out


ATTN = _bf16_rows() + _f32_rows()


def all_instances():
    """the 76 kernel instances sedt_attention_fwd / sedt_attention_bwd dispatch to"""
    s = set([GEN_F16, GEN_B16, GEN_F32, GEN_B32])
    for am in ('false', 'true'):
        s.update(f'attn_fwd_mfma_kernel<{nt}, {am}>' for nt in range(1, 9))
        s.update(f'attn_bwd_mfma_kernel<{a}, {b}, {am}>' for a in range(1, 5) for b in range(1, 5))
        for dr in ('false', 'true'):
            s.update(f'attn_f32_fwd_kernel<{nt}, {am}, {dr}>' for nt in (1, 4))
            s.update(f'attn_f32_bwd_kernel<{a}, {b}, {am}, {dr}>' for a in (1, 4) for b in (1, 4))
    assert len(s) == 76
    return s


def kpm_pattern(kind, B, Lk):
    """bool [B][Lk] as nested lists (True = padded); every clip keeps at least one key, neighbouring clips differ"""
    rows = []
    for b in range(B):
        if kind == 'tail':
            r = [j >= Lk - (5 + b) for j in range(Lk)]
        elif kind == 'one':
            r = [j != (7 * b + 3) % Lk for j in range(Lk)]
        elif kind == 'mid':
            r = [Lk // 3 <= j <= Lk // 2 + b for j in range(Lk)]
        elif kind == 'tiles':
            # whole 32-key tiles emptied: even clips keep the first tile only (less its last b keys), odd clips lose the first
            # tile(s) and keep the rest
            first = 32 * (1 + (b // 2) % max(1, (Lk - 1) // 32))
            r = [(j >= 32 - b) if b % 2 == 0 else (j < first) for j in range(Lk)]
        else:
            raise ValueError(kind)
        assert not all(r), (kind, b, Lk)
        rows.append(r)
    return rows


GUARD = 32      # guard columns left of an output (and as many right of it) where the row stride leaves room


def guard_left(W, ld):
    return GUARD if ld >= W + 2 * GUARD else 0


def out_start(c, which):
    """element offset of output `which` ('o', 'dq', 'dk', 'dv') from the start of its (512-byte aligned) allocation: one guard row and
    the left guard columns in front of it, o also its misalignment"""
    lay = layout_of(c)
    return (lay['o_off'] if which == 'o' else 0) + lay['ld_out'] + guard_left(c['H'] * 32, lay['ld_out'])


def layout_of(c):
    """element layout of a row: dict(ld of q/k/v/do, pad columns and element offsets of the outputs) - shared by the GPU test (real
    tensors) and the CPU test (fake pointers).  Offsets are in elements."""
    W = c['H'] * 32
    eb = 2 if c['dt'] == 'bf16' else 4
    if c['layout'] == 'stride':
        odd = 4 if c['dt'] == 'bf16' else 2
        return dict(packed=False, ld_in=W + odd, ld_out=W + odd, o_off=0, eb=eb)
    return dict(packed=True, ld_in=512, ld_out=W + 64, o_off=(8 // eb) if c['layout'] == 'o_off' else 0, eb=eb)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln(dt, D, rows, kind='normal', add=False, dy2=False, dres=False, dres2=False, drop=False):
    name = f'ln_{dt}_d{D}_r{rows}_{kind}' + ''.join(t for t, on in (('_add', add), ('_dy2', dy2), ('_res', dres), ('_res2', dres2), ('_drop', drop)) if on)
    return dict(name=name, dt=dt, D=D, rows=rows, kind=kind, add=add, dy2=dy2, dres=dres, dres2=dres2, drop=drop)


def _ln_rows():
    out = []
    n = 0
    for dt in ('f32', 'bf16'):
        for D in (256, 512):
            for rows in (1, 3, 4, 5, 2047, 2048, 2049, 8195):
                out.append(_ln(dt, D, rows, ('normal', 'steps')[n % 2], add=bool(n & 1), dy2=bool(n & 2), dres=bool(n & 4), dres2=(n % 8) >= 6,
                               drop=(n % 3 == 0)))
                n += 1
            out.append(_ln(dt, D, 2049, 'normal', True, True, True, True, True))
            out.append(_ln(dt, D, 5, 'const', add=True))
            out.append(_ln(dt, D, 2049, 'const', dres=True, drop=True))
            out.append(_ln(dt, D, 8195, 'steps', dy2=True, dres2=True))
    for D in (256, 512):
        out.append(_ln('f32', D, 2049, 'mean100', add=True, dres=True))
        out.append(_ln('f32', D, 5, 'mean100'))
    return out


LN = _ln_rows()
