"""The convolution-form sweep behind tests/golden/g24_conv_forms.npz: which launch form ops.conv_fwd / ops.conv_dgrad give a convolution
(direct 3x3 kernel, stride-2 input gradient by output parity, dilated 3x3 by column halves, or the generic implicit GEMM), the argument
blocks of the grouped forms and the hint a recording (ops.PROFILE) attaches to the nine-tap problem it runs instead.

Everything runs on the CPU: the operands are stand-ins on fake 256-byte aligned addresses (the planner and igemm_args read a tensor's
dtype, address, strides and shape, never its memory), the library's launch entry points are replaced by recorders while a case runs and
the kernel labels come from sedt_igemm_group_describe, which launches nothing.

answer(ops, L, case) drives the two ENTRY POINTS, once without and once with a recording, and returns one JSON string:
  [form, x3, hint, label, blocks]     hint: None | 'conv3x3_c64_kernel' | ['group', label, share]
                                      blocks: per problem of a grouped form every SedtIgemm field, pointers as [operand name, byte offset]
tests/golden/make_golden_conv_forms.py stores them; tests/test_conv_plan_cpu.py compares and holds ops.conv_form to the same record.
"""
import contextlib
import ctypes as C
import json

import torch

NAMES = ['t', 'w', 'out', 'scale', 'bias', 'res', 'mask', 't3', 'w3']
SHIFT = 40
FORM_OF = {'conv3x3_c64': 'direct3x3', 'igemm_group_s2': 's2_parity', 'igemm_group_dil': 'dil_halves'}
SHARE = {'direct3x3': 1.0, 's2_parity': 0.25, 'dil_halves': 2.0 / 3.0, 'gemm': 1.0}
SWITCHES = ('CONV3_DIRECT', 'S2_PARITY', 'DIL_HALVES', 'X3_FAST', 'GEMM_X3')


class T(object):
    """stand-in for a device tensor [rows, cols] with row stride ld, `off` bytes into the fake allocation of its name"""
    is_cuda = True

    def __init__(self, name, rows, cols, dtype, ld=None, off=0):
        self.name, self.shape, self.dtype, self.ld, self.off = name, (rows, cols), dtype, (cols if ld is None else ld), off

    def data_ptr(self):
        return ((NAMES.index(self.name) + 1) << SHIFT) + self.off

    def stride(self, i=None):
        return (self.ld, 1) if i is None else (self.ld, 1)[i]

    def numel(self):
        return self.shape[0] * self.shape[1]

    def view(self, rows, cols):
        assert rows * cols == self.numel() and self.ld == self.shape[1]
        return T(self.name, rows, cols, self.dtype, off=self.off)


def _fake_split3(jobs):
    """ops._split3 without the launch: the images [rows][2 cols] / [rows][3 cols] of (tensor, offset, rows, cols, ld, pattern)"""
    return [T(t.name + '3', rows, (3 if pattern else 2) * cols, torch.bfloat16) for t, _, rows, cols, _, pattern in jobs]


def _block(a):
    out = []
    for name, ty in type(a)._fields_:
        v = getattr(a, name)
        if ty is C.c_void_p:
            v = None if v is None else [NAMES[(v >> SHIFT) - 1], v & ((1 << SHIFT) - 1)]
        elif name == 'btap':
            v = list(v)
        out.append(v)
    return out


class _Recorder(object):
    """the library with its launch entry points replaced: they note what was asked for and return success"""

    def __init__(self, real, L, seen):
        self.real, self.L, self.seen = real, L, seen

    def sedt_conv3x3_c64(self, *args):
        return 0

    def sedt_igemm_group(self, arr, n, code, stream):
        self.seen['blocks'] = [self.L.SedtIgemm.from_buffer_copy(arr[i]) for i in range(n)]
        self.seen['code'] = code
        return 0

    def __getattr__(self, name):
        return getattr(self.real, name)


def _hint_argument(ops, kw):
    return kw.get('hint')


@contextlib.contextmanager
def recording_library(ops, L, seen, hint_of=_hint_argument):
    real = L.load()
    keep = (L.load, L.check, L.stream_ptr, ops._split3, ops.igemm)
    rec = _Recorder(real, L, seen)

    def check(status, what=''):
        assert status == 0
        seen['form'] = FORM_OF[what]

    def igemm(dtype, M, N, K, A, lda, B, ldb, Cout, ldc, **kw):
        seen['form'], seen['hint'] = 'gemm', hint_of(ops, kw)
        seen['gemm'] = (M, N, K, A.name, lda, B.name, ldb, Cout.name, ldc)

    L.load, L.check, L.stream_ptr, ops._split3, ops.igemm = (lambda: rec), check, (lambda: None), _fake_split3, igemm
    try:
        yield
    finally:
        L.load, L.check, L.stream_ptr, ops._split3, ops.igemm = keep


@contextlib.contextmanager
def switches(ops, L, case):
    """the case's compute mode, the switches it turns off and its co-scheduling state, as module attributes; restored on exit"""
    keep = [getattr(L if s == 'GEMM_X3' else ops, s) for s in SWITCHES] + [ops._co['on'], ops.PROFILE]
    try:
        for s in SWITCHES[:4]:
            setattr(ops, s, s not in case['off'])
        L.GEMM_X3 = case['mode'] == 'x3' and 'GEMM_X3' not in case['off']
        ops._co['on'] = case['co']
        yield
    finally:
        for s, v in zip(SWITCHES, keep):
            setattr(L if s == 'GEMM_X3' else ops, s, v)
        ops._co['on'], ops.PROFILE = keep[5], keep[6]


def operands(ops, case):
    """(dtype code, t, B, g, w, out, ep) of the case: t = x (forward) or dY (input gradient), w the packed forward / dgrad operand"""
    Hi, Wi, Ci, Co, k, s, p, d = case['geom']
    g = ops.ConvGeom(Hi, Wi, Ci, Co, k, s, p, d)
    for attr, v in case['gmut'].items():
        setattr(g, attr, v)
    B, tw = case['B'], case['tweak']
    act = torch.bfloat16 if case['mode'] == 'bf16' else torch.float32
    fwd = case['kind'] == 'fwd'
    cin, cout = (Ci, Co) if fwd else (Co, Ci)
    rows_t, rows_o = (B * Hi * Wi, B * g.Ho * g.Wo) if fwd else (B * g.Ho * g.Wo, B * Hi * Wi)
    t = T('t', rows_t, cin, tw.get('t_dtype', act), tw.get('t_ld'), tw.get('t_off', 0))
    w = T('w', cout, k * k * cin, act, tw.get('w_ld'))
    out = T('out', rows_o, cout, tw.get('out_dtype', act), tw.get('out_ld'))
    ep = {}
    for tok in case['ep']:
        if tok == 'bn':
            ep['scale'], ep['bias'] = T('scale', 1, cout, torch.float32), T('bias', 1, cout, torch.float32)
        elif tok in ('scale', 'bias'):
            ep[tok] = T(tok, 1, cout, torch.float32)
        elif tok == 'relu':
            ep['act'] = ops.ACT_RELU
        elif tok == 'sigmoid':
            ep['act'] = ops.ACT_SIGMOID
        elif tok == 'mask':
            ep['mask'], ep['ldm'] = T('mask', rows_o, cout, tw.get('mask_dtype', act)), tw.get('ldm', cout)
        elif tok == 'maskbits':
            ep['mask'], ep['ldm'], ep['mask_bits'] = T('mask', rows_o, cout // 8, torch.uint8), cout // 8, True
        elif tok == 'res':
            ep['res'], ep['ldr'] = T('res', rows_o, cout, tw.get('res_dtype', act)), cout
        elif tok == 'alpha':
            ep['alpha'] = 0.5
        elif tok == 'tile':
            ep['tile'] = (64, 64)
        elif tok == 'tile0':
            ep['tile'] = (0, 0)
        elif tok == 'res_mod':
            ep['res_mod'] = 0
        else:
            raise KeyError(tok)
    return (ops.BF16 if case['mode'] == 'bf16' else ops.F32), t, B, g, w, out, ep


def group_label(L, blocks, code=1):
    buf = C.create_string_buffer(160)
    r = L.load().sedt_igemm_group_describe((L.SedtIgemm * len(blocks))(*blocks), len(blocks), code, buf, 160)
    return buf.value.decode() if r == 0 else None


def run(ops, L, case, hint_of=_hint_argument):
    """(form, x3, hint, label, blocks) of the case through the entry points: what the un-recorded call launches, what the recorded one hints"""
    fn = ops.conv_fwd if case['kind'] == 'fwd' else ops.conv_dgrad
    with switches(ops, L, case):
        dtype, t, B, g, w, out, ep = operands(ops, case)
        seen, rec = {}, {}
        with recording_library(ops, L, seen, hint_of):
            fn(dtype, t, B, g, w, out=out, **ep)
        ops.PROFILE = []
        with recording_library(ops, L, rec, hint_of):
            fn(dtype, t, B, g, w, out=out, **ep)
        # a recorded call runs the generic kernel on the whole problem (all taps), whatever the form
        assert ops.PROFILE == [] and rec['form'] == 'gemm' and rec['gemm'][3::2] == ('t', 'w', 'out')
        assert rec['gemm'][:3] == (out.shape[0], out.shape[1], g.taps * t.shape[1])
        blocks = seen['blocks'] if seen['form'] in ('s2_parity', 'dil_halves') else None
        assert blocks is None or seen['code'] == 1
        x3 = bool(blocks and blocks[0].f32ep)
        label = group_label(L, blocks) if blocks else None
        hint = rec['hint']
    return seen['form'], x3, (list(hint) if isinstance(hint, tuple) else hint), label, (blocks and [_block(a) for a in blocks])


def answer(ops, L, case, hint_of=_hint_argument):
    return json.dumps(run(ops, L, case, hint_of))


# ------------------------------------------------------------------------------------------------ the cases
def case(name, kind, mode, B, geom, ep, off=(), co=False, gmut=None, tweak=None, base=None, expect=None):
    return dict(name=name, kind=kind, mode=mode, B=B, geom=geom, ep=list(ep), off=tuple(off), co=co, gmut=gmut or {}, tweak=tweak or {},
                base=base, expect=expect)


def backbone_geoms(h1):
    """(Hi, Wi, Ci, Co, k, stride, pad, dilation) of every convolution of the ResNet-50 body behind the stem, layer1's map h1 x 16: maps of
    16 / 16 / 8 / 4 / 4 columns, layer4 at stride 1 and dilation 2 (its block 0 still at dilation 1)"""
    out, H, W, cin = [], h1, 16, 64
    for planes, blocks, stride, dil in ((64, 3, 1, 1), (128, 4, 2, 1), (256, 6, 2, 1), (512, 3, 1, 2)):
        for b in range(blocks):
            s, d = (stride, 1) if b == 0 else (1, dil)
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            new = [(H, W, cin, planes, 1, 1, 0, 1), (H, W, planes, planes, 3, s, d, d), (Ho, Wo, planes, 4 * planes, 1, 1, 0, 1)]
            if b == 0:
                new.append((H, W, cin, 4 * planes, 1, s, 0, 1))
            for q in new:
                if q not in out:
                    out.append(q)
            H, W, cin = Ho, Wo, 4 * planes
    return out


H1 = {'C2': 125, 'C3': 124, 'C4': 32, 'C5': 125}       # layer1's map height: 500 / 496 frames, SP-SEDT's 128-frame patches
EP = {'fwd': ('bn', 'relu'), 'dgrad': ('maskbits',)}


def _edges():
    """around each envelope: a base case inside it and cases that differ from the base in exactly ONE clause, which must refuse the form"""
    out = []

    def family(tag, form, kind, mode, B, geom, ep, variants):
        base = '%s %s %s base' % (tag, kind, mode)
        out.append(case(base, kind, mode, B, geom, ep, expect=form))
        for name, kw in variants:
            kw = dict(kw)
            out.append(case('%s %s %s %s' % (tag, kind, mode, name), kind, mode, kw.pop('B', B), kw.pop('geom', geom), kw.pop('ep', ep),
                            base=base, expect=kw.pop('expect', 'gemm'), **kw))

    def gm(**kw):
        return dict(gmut=kw)

    # ---- the direct 3x3 kernel: layer1's conv2 geometry (64 -> 64 channels, 16 columns), contiguous rows, plain epilogues
    c64 = (5, 16, 64, 64, 3, 1, 1, 1)
    flat = dict(t_ld=64, out_ld=64, ldm=64)                  # (so that the channel count alone fails, not the row strides that follow it)
    geo = [('Ci', dict(geom=(5, 16, 128, 64, 3, 1, 1, 1), tweak=flat)), ('Co', dict(geom=(5, 16, 64, 128, 3, 1, 1, 1), tweak=flat)),
           ('Wi=8', dict(geom=(5, 8, 64, 64, 3, 1, 1, 1))),
           ('KH', gm(KH=1)), ('KW', gm(KW=1)), ('sh', gm(sh=2)), ('sw', gm(sw=2)), ('ph', gm(ph=0)), ('pw', gm(pw=0)), ('dh', gm(dh=2)), ('dw', gm(dw=2)),
           ('t stride 72', dict(tweak=dict(t_ld=72))), ('out stride 72', dict(tweak=dict(out_ld=72))), ('switch', dict(off=('CONV3_DIRECT',)))]
    for kind, ep in (('fwd', ('bn', 'relu')), ('dgrad', ('mask',))):
        v = geo + [('tile', dict(ep=ep + ('tile',))), ('key alpha', dict(ep=ep + ('alpha',)))]
        if kind == 'fwd':
            v += [('sigmoid', dict(ep=('bn', 'sigmoid'))), ('mask+relu', dict(ep=('bn', 'relu', 'mask'))), ('ldm', dict(ep=('bn', 'mask'), tweak=dict(ldm=72))),
                  ('mask ok', dict(ep=('bn', 'mask'), expect='direct3x3')), ('tile 0 ok', dict(ep=ep + ('tile0',), expect='direct3x3')),
                  ('plain ok', dict(ep=(), expect='direct3x3')), ('Hi=1 ok', dict(geom=(1, 16, 64, 64, 3, 1, 1, 1), expect='direct3x3'))]
        else:
            v += [('ldm', dict(tweak=dict(ldm=72))), ('mask+relu', dict(ep=('mask', 'relu'))), ('scale', dict(ep=('mask', 'scale'))),
                  ('bias', dict(ep=('mask', 'bias'))), ('plain ok', dict(ep=(), expect='direct3x3')), ('relu ok', dict(ep=('relu',), expect='direct3x3'))]
        family('direct', 'direct3x3', kind, 'bf16', 2, c64, ep, v)
    out.append(case('direct fwd f32', 'fwd', 'f32', 2, c64, ('bn', 'relu'), base='direct fwd bf16 base', expect='gemm'))
    out.append(case('direct dgrad x3', 'dgrad', 'x3', 2, c64, ('mask',), base='direct dgrad bf16 base', expect='gemm'))

    # ---- the stride-2 input gradient by output parity
    s2 = (7, 5, 64, 64, 3, 2, 1, 1)
    v = [('Co % 64', dict(geom=(7, 5, 64, 96, 3, 2, 1, 1))), ('Ci % 8', dict(geom=(7, 5, 68, 64, 3, 2, 1, 1), tweak=dict(out_ld=72))), ('w ld', dict(tweak=dict(w_ld=9 * 64 + 8))),
         ('dy stride', dict(tweak=dict(t_ld=68))), ('out stride', dict(tweak=dict(out_ld=68))), ('key scale', dict(ep=('maskbits', 'res', 'scale'))),
         ('key act', dict(ep=('maskbits', 'res', 'relu'))), ('switch', dict(off=('S2_PARITY',))), ('co', dict(co=True)),
         ('KH', gm(KH=1)), ('KW', gm(KW=1)), ('sh', gm(sh=1)), ('sw', gm(sw=1)), ('ph', gm(ph=0)), ('pw', gm(pw=0)), ('dh', gm(dh=2)), ('dw', gm(dw=2)),
         ('alpha ok', dict(ep=('maskbits', 'res', 'alpha'), expect='s2_parity')), ('plain ok', dict(ep=(), expect='s2_parity')),
         ('Hi=1 ok', dict(B=2, geom=(1, 16, 128, 128, 3, 2, 1, 1), expect='s2_parity')), ('even ok', dict(geom=(64, 8, 256, 256, 3, 2, 1, 1), expect='s2_parity')),
         ('Wi=1 ok', dict(geom=(5, 1, 64, 64, 3, 2, 1, 1), expect='s2_parity'))]
    family('parity', 's2_parity', 'dgrad', 'bf16', 1, s2, ('maskbits', 'res'), v)
    x3v = [('t 8 bytes off', dict(tweak=dict(t_off=8))), ('bf16 res', dict(tweak=dict(res_dtype=torch.bfloat16))),
           ('bf16 mask', dict(ep=('mask', 'res'), tweak=dict(mask_dtype=torch.bfloat16))), ('bf16 t', dict(tweak=dict(t_dtype=torch.bfloat16))),
           ('bf16 out', dict(tweak=dict(out_dtype=torch.bfloat16))), ('X3_FAST', dict(off=('X3_FAST',))), ('GEMM_X3', dict(off=('GEMM_X3',)))]
    family('parity', 's2_parity', 'dgrad', 'x3', 1, s2, ('maskbits', 'res'),
           x3v + [('f32 mask ok', dict(ep=('mask', 'res'), expect='s2_parity')), ('t 16 bytes off ok', dict(tweak=dict(t_off=16), expect='s2_parity'))])
    out.append(case('parity fwd', 'fwd', 'bf16', 1, s2, ('bn', 'relu'), base='parity dgrad bf16 base', expect='gemm'))

    # ---- the dilated 3x3 by column halves: 2 d columns, at least 96 tiles of 128x128 over the two problems
    dil = (32, 4, 512, 512, 3, 1, 2, 2)
    for kind, ep in (('fwd', ('bn', 'relu')), ('dgrad', ('maskbits',))):
        ci = 2 if kind == 'fwd' else 3                        # where the gathered tensor's channels / the output's sit in the geometry tuple

        def ch(cin=512, cout=512, H=32, W=4, p=2, d=2):
            q = [H, W, 0, 0, 3, 1, p, d]
            q[ci], q[5 - ci] = cin, cout
            return tuple(q)

        v = [('95 tiles', dict(B=190, geom=ch(cin=64, cout=128))), ('96 tiles ok', dict(B=192, geom=ch(cin=64, cout=128), expect='dil_halves')),
             ('cout % 128', dict(B=192, geom=ch(cout=192))), ('cin % 64', dict(geom=ch(cin=96))), ('Wi != 2 d', dict(geom=ch(W=8))), ('w ld', dict(tweak=dict(w_ld=9 * 512 + 8))),
             ('t stride', dict(tweak=dict(t_ld=516))), ('out stride', dict(tweak=dict(out_ld=516))), ('key tile', dict(ep=ep + ('tile0',))),
             ('key res_mod', dict(ep=ep + ('res_mod',))), ('switch', dict(off=('DIL_HALVES',))), ('co', dict(co=True)),
             ('KH', gm(KH=1)), ('KW', gm(KW=1)), ('sh', gm(sh=2)), ('sw', gm(sw=2)), ('dw', gm(dw=1)), ('ph', gm(ph=1)), ('pw', gm(pw=1)), ('Ho', gm(Ho=31)), ('Wo', gm(Wo=3)),
             ('d=1 ok', dict(B=768, geom=ch(cout=2048, H=1, W=2, p=1, d=1), expect='dil_halves')), ('odd H ok', dict(geom=ch(H=31), expect='dil_halves')),
             ('res alpha ok', dict(ep=ep + ('res', 'alpha'), expect='dil_halves'))]
        family('halves', 'dil_halves', kind, 'bf16', 64, dil, ep, v)
        family('halves', 'dil_halves', kind, 'x3', 64, dil, ep + ('res',),
               [q for q in x3v if kind == 'dgrad' or q[0] != 'bf16 mask']
               + [('t 16 bytes off ok', dict(tweak=dict(t_off=16), expect='dil_halves'))])
    return out


def cases():
    out = []
    for cfg in ('C2', 'C3', 'C4'):                            # (C5 trains on C2's map)
        for B in (2, 32, 64):
            for geom in backbone_geoms(H1[cfg]):
                for mode in ('bf16', 'f32', 'x3'):
                    for kind in ('fwd', 'dgrad'):
                        out.append(case('%s B%d %s %s %s' % (cfg, B, geom, mode, kind), kind, mode, B, geom, EP[kind]))
    for geom in backbone_geoms(H1['C2']):
        for kind in ('fwd', 'dgrad'):
            for mode, offs in (('bf16', SWITCHES[:3]), ('x3', SWITCHES[1:])):
                for off in offs:
                    out.append(case('C2 B64 %s %s %s %s off' % (geom, mode, kind, off), kind, mode, 64, geom, EP[kind], off=(off,)))
                out.append(case('C2 B64 %s %s %s co-scheduled' % (geom, mode, kind), kind, mode, 64, geom, EP[kind], co=True))
    out += _edges()
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    return out
