"""GPU: the matching, criterion, postprocess, pseudo-label, feature-loss, sum and layer-scaling kernels (csrc/criterion.hip,
csrc/postproc.hip) at the edges of the envelope their entry points accept, against float64 references computed on the CPU at test
time (tests/target_check.py; rows and the work split of every kernel in tests/target_cases.py).  The model is not built: the ops.*
wrappers are called directly.

Per row: every output is a view into one NaN-filled buffer with guard words on both sides (the dense targets are
SetCriterion.dense_views of one packed buffer inside it; the wrappers that allocate their own results are launched a second time
through the C entry point on the same arguments with the outputs redirected into the buffer); no byte outside the outputs changes,
every element is finite where the reference is, index outputs and copied values are exact, values and gradients stay inside the bounds
of tests/target_check.py, and a second launch is bit-identical.  The criterion rows take their dense targets from the reference, so a
matching error cannot hide a loss error or the reverse.  The refused calls return non-zero, sedt_last_error names the entry point and
no byte changes.

Not exercised: a clip with more events than max_targets.  The entry point cannot see the event counts (they are device data) and the
kernel would write past its LDS tile; TargetTables.load refuses such a batch on the host.  A pseudo-label launch above 150 KB of LDS
and every other call the entry points reject before launching are in test_refused_calls.

Kernel findings of this module (fixed in csrc/criterion.hip, set_criterion_kernel).  Row `coincident` (a predicted interval that
shares its start with its target, one that shares its end, one that only touches it): the GIoU gradient took another sub-gradient than
the reference's autograd - min / max gave a tie wholly to one side and the clamp of the overlap passed nothing at 0 (db2 of the first
query -1.0 against -1.1667: 1163 times the bound).  The kernel now splits a tie evenly and lets the clamp pass at 0, as torch does.
Row `no_events` (num_boxes = 0): loss_bbox / loss_giou came out 0 where the reference divides 0 by 0, and the target column of the
class gradient -inf where its autograd forms inf - inf; the kernel now adds 0 * (1 / num_boxes) to those entries: +0 for every finite
value, NaN otherwise; a batch without any strong clip (row `split_0`: split[0] = 0, every row skipped) keeps set losses of 0 and a
finite total.  For every input other than coincident edges and num_boxes = 0 with strong clips present, no output bit changes.

Largest error / bound ratio per kernel and output on an MI355X (pytest -s prints the table), the float32 restatement of
tests/test_target_check_cpu.py in brackets; index outputs and copied values (tc, tidx, assign, tgt_len, tbox, labels, lab_cat, box_cat,
offsets, counters, the hit / matched counts) are exact in both:
  match          gt_weak 0.000124 (0.000124)   coef 0 (0)   wbox 0 (0)
  criterion      out 0.0133 (0.013)   dl 0.00346 (0.00346)   db 0.000263 (0.000263)   db2 0.0119 (0.0119)   dat 0.000872 (0.00116)
                 dat_p 0.000465 (0.000465)
  criterion_bwd  glogits 0.00567 (0.00569)   gboxes 0.0128 (0.0122)   gat 0.00116 (0.00116)   gat_p 0.000573 (0.000459)
  post           scores 0.147 (0.107)   boxes 0.0511 (0.0511)
  feature        out 0.0112 (0.0132)   rowloss 0.0176 (0.0202)   dpred 0.0028 (0.00265)   total 0.0038 (0.00509)
  sum_f32        0.0033 (0.00662)        scale_layers 0.266 (0.266)
Module run time on an MI355X: 3.7 s for the 101 tests (100 table rows and the refused calls; 1.4 s between the first and the last of
them), float64 references included.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gemm_check as GC
import target_cases as TC
import target_check as K

pytestmark = pytest.mark.gpu

RATIOS = collections.defaultdict(float)
T0 = [None]
F = np.float32


def setup_module(module):
    T0[0] = time.time()


def teardown_module(module):
    if RATIOS:
        print('\nlargest error / bound ratio per kernel and output:')
        for k in sorted(RATIOS):
            print(f'  {k:40s} {RATIOS[k]:.3g}')
        print(f'module time {time.time() - T0[0]:.1f} s')


def _note(fam, r, got=None, ref=None):
    for k, v in r.items():
        RATIOS[f'{fam} {k}'] = max(RATIOS[f'{fam} {k}'], v)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    why = {k: K.worst(got[k], ref[k]) for k in bad if got is not None and k in got and k in ref and ref[k] is not None}
    assert not bad, (fam, bad, why)


def _ids(rows):
    return [c.name for c in rows]


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _lib():
    from sound_event_detection_transformer_amd import lib
    return lib


_ESZ = {torch.float32: 4, torch.int32: 4, torch.int64: 8}


class Out(object):
    """the outputs of one row as views of ONE NaN-filled device buffer (layout: target_check.Arena)"""

    def __init__(self):
        self.lay, self.specs, self.written = K.Arena(), {}, {}

    def add(self, name, shape, dtype=torch.float32, written=None):
        """written: the number of leading elements the kernel is to write (default: all)"""
        n = int(np.prod(shape))
        self.specs[name] = (self.lay.add(name, n * _ESZ[dtype]), tuple(shape), dtype, n)
        self.written[name] = (n if written is None else written) * _ESZ[dtype]
        return self

    def build(self):
        self.buf = GC.nan_buffer(self.lay.words, torch.float32)
        self.v = {}
        for name, (o, shape, dtype, n) in self.specs.items():
            self.v[name] = self.buf[o:o + n * _ESZ[dtype] // 4].view(dtype).view(shape)
        self.before = self.image()
        return self

    def __getitem__(self, name):
        return self.v[name]

    def image(self):
        torch.cuda.synchronize()
        return self.buf.view(torch.uint8).cpu().numpy().copy()

    def reset(self):
        self.buf.fill_(float('nan'))

    def check(self, only=None):
        """the image after a launch; nothing outside the written parts of the outputs (`only`: of these outputs) may have changed"""
        img = self.image()
        reg = [(4 * self.specs[k][0], self.written[k]) for k in self.specs if only is None or k in only]
        bad = K.guard_check(self.before, img, reg)
        assert bad is None, f'byte {bad} outside the outputs changed (slots: {self.lay.slots})'
        return img


def _same(a, b):
    """bit-identical tensors (NaN == NaN)"""
    return a is None and b is None or np.array_equal(_np(a).view(np.uint8), _np(b).view(np.uint8))


# ------------------------------------------------------------------------------------------------ matching
def _tables(inp):
    t = K.flat_tables(inp)
    return {k: _dev(v) for k, v in t.items()}


def _split(inp):
    return None if inp['split'] is None else _dev(np.asarray(inp['split'], np.int32))


def _match_call(inp, tables, dense, assign, lg, bx, rand):
    from sound_event_detection_transformer_amd import ops
    ops.match_targets(lg, bx, tables, dense, inp['layer_of'], K.W_CLASS, K.W_BBOX, K.W_GIOU, inp['mt'], assign=assign, fl=inp['fl'],
                      fine_tune=inp['ft'], normalize=inp['norm'], epsilon=inp['eps'], alpha=inp['alpha'], alpha_fl=K.ALPHA_FL,
                      gamma_fl=K.GAMMA_FL, ft_rand=rand if inp['ft'] else None, q0=inp['q0'])


def _dense_out(inp):
    from sound_event_detection_transformer_amd.sedt.sedt import SetCriterion
    L, B, ns, n_lab, Q, Cn = (inp[k] for k in ('L', 'B', 'ns', 'n_lab', 'Q', 'C'))
    n = K.dense_numel(L, ns, Q, n_lab, Cn, B)
    o = Out().add('pack', (n,), written=n - 1).add('assign', (L, ns, Q), torch.int32).build()      # (num_boxes, the last word, is sum_f32's)
    dense = SetCriterion.dense_views(o['pack'], (L, ns, Q, n_lab, Cn, B))
    dense['split'] = _split(inp)
    return o, dense


@pytest.mark.parametrize('c', TC.MATCH, ids=_ids(TC.MATCH))
def test_match_targets(c):
    inp = K.match_inputs(c)
    ref = K.match_ref(inp)
    o, dense = _dense_out(inp)
    args = (inp, _tables(inp), dense, o['assign'], _dev(inp['logits']), _dev(inp['boxes']), _dev(inp['ft_rand']))
    _match_call(*args)
    img = o.check()
    got = {k: _np(dense[k]) for k in ('tc', 'coef', 'wbox', 'tbox', 'tidx', 'tgt_len', 'gt_weak')}
    got['assign'] = _np(o['assign'])
    if c.flags.get('tie'):
        # the assignment need not be scipy's: valid, optimal in float64, and the host solver's ("ties -> lowest column, as host.cpp")
        assert K.check_tie(inp, got['assign']) <= 1e-12
        assert np.array_equal(got['assign'], K.host_assign(inp))
        ref = K.dense_from_assign(inp, got['assign'])
    _note('match', K.check_dense(got, ref, inp), got, ref)
    o.reset()
    _match_call(*args)
    assert np.array_equal(img, o.check()), 'a second launch differs'


# ------------------------------------------------------------------------------------------------ criterion
def _crit_launch(inp):
    """(out, total, state, nonfinite) of ops.set_criterion on the reference's dense targets"""
    from sound_event_detection_transformer_amd import ops
    from sound_event_detection_transformer_amd.sedt.sedt import SetCriterion
    L, B, ns, n_lab, Q, Cn = (inp[k] for k in ('L', 'B', 'ns', 'n_lab', 'Q', 'C'))
    pack = _dev(K.pack_dense(inp['dense'], inp['nb']))
    dense = SetCriterion.dense_views(pack, (L, ns, Q, n_lab, Cn, B))
    if inp['num_boxes'] is None:
        dense['num_boxes'] = None                                   # the kernel sums the final layer's box weights itself
    dense['split'] = _split(inp)
    nonfinite = torch.zeros(1, dtype=torch.int32, device='cuda')
    keep = [_dev(inp['logits']), _dev(inp['boxes']), _dev(inp['at']), _dev(inp['at_p']), _dev(inp['empty_weight']), dense]
    out, total, state = ops.set_criterion(keep[0], keep[1], keep[2], dense, keep[4], inp['layer_of'], inp['w_ce'], inp['w_bbox'],
                                          inp['w_giou'], inp['w_weak'], fl=inp['fl'], alpha_fl=K.ALPHA_FL, gamma_fl=K.GAMMA_FL,
                                          nonfinite=nonfinite, q0=inp['q0'], at_p=keep[3], w_weak_p=inp['w_weak_p'], wp_all=inp['wp_all'])
    return out, total, state, nonfinite, keep


@pytest.mark.parametrize('c', TC.CRITERION, ids=_ids(TC.CRITERION))
def test_set_criterion_and_bwd(c):
    from sound_event_detection_transformer_amd import ops
    lib = _lib()
    inp = K.crit_inputs(c)
    ref = K.criterion_ref(inp)
    L, B, Q, Qs, C1 = inp['L'], inp['B'], inp['Q'], inp['Qs'], inp['C'] + 1
    out, total, state, nonfinite, keep = _crit_launch(inp)
    a, dl, db, db2, dat, dat_p, _ = state
    # the second launch: the same arguments through the C entry point, every output redirected into the guarded buffer
    o = Out().add('out', (4 * L + 6,)).add('total', (1,)).add('dl', (L, B, Q, C1)).add('db', (L, B, Q, 2)).add('db2', (L, B, Q, 2))
    if dat is not None:
        o.add('dat', tuple(dat.shape))
    if dat_p is not None:
        o.add('dat_p', tuple(dat_p.shape))
    o.add('gl', (L, B, Qs, C1)).add('gb', (L, B, Qs, 2))
    if dat is not None:
        o.add('gat', tuple(dat.shape))
    if dat_p is not None:
        o.add('gat_p', tuple(dat_p.shape))
    o.build()
    fwd = [k for k in ('out', 'total', 'dl', 'db', 'db2', 'dat', 'dat_p') if k in o.v]
    a.out, a.total, a.dlogits, a.dboxes, a.dboxes2 = (o[k].data_ptr() for k in ('out', 'total', 'dl', 'db', 'db2'))
    if dat is not None:
        a.dat = o['dat'].data_ptr()
    if dat_p is not None:
        a.dat_p = o['dat_p'].data_ptr()
    nf2 = torch.zeros(1, dtype=torch.int32, device='cuda')
    a.nonfinite = nf2.data_ptr()
    scratch = torch.empty(L * B * Q * 5, device='cuda', dtype=torch.float32)
    assert lib.load().sedt_set_criterion(a, _p(scratch), lib.stream_ptr()) == 0, lib.load().sedt_last_error()
    o.check(only=fwd)
    for x, k in ((out, 'out'), (dl, 'dl'), (db, 'db'), (db2, 'db2'), (dat, 'dat'), (dat_p, 'dat_p')):
        assert _same(x, o.v.get(k)), f'{k}: a second launch differs'
    assert _same(total.reshape(1), o['total']) and _same(o['total'], o['out'][4 * L + 3:4 * L + 4])
    bad_total = not np.isfinite(ref['out'][K.SLOTS(L)['total']])
    assert nonfinite.item() == nf2.item() == int(bad_total)
    got = {k: _np(o.v.get(k)) for k in ('dl', 'db', 'db2', 'dat', 'dat_p')}
    _note('criterion', K.check_criterion(_np(o['out']), got, ref, inp), dict(got, out=_np(o['out'])), dict(ref['terms'], out=ref['out']))
    # backward: through the loss vector, through the separately returned total, through both
    g, gtot = _dev(inp['g']), _dev(np.asarray([inp['gtotal']], F))
    bw = [k for k in ('gl', 'gb', 'gat', 'gat_p') if k in o.v]
    for mode, (gv, gt) in (('g', (g, None)), ('gtotal', (None, gtot)), ('both', (g, gtot))):
        first = ops.set_criterion_bwd(state, gv, gt)
        for k in bw:
            o[k].fill_(float('nan'))
        assert lib.load().sedt_set_criterion_bwd(a, _p(gv), _p(gt), _p(o['gl']), _p(o['gb']), _p(o.v.get('gat')), _p(o.v.get('gat_p')),
                                                 lib.stream_ptr()) == 0, lib.load().sedt_last_error()
        o.check(only=fwd + bw)
        second = tuple(o.v.get(k) for k in ('gl', 'gb', 'gat', 'gat_p'))
        assert all(_same(x, y) for x, y in zip(first, second)), f'bwd {mode}: a second launch differs'
        names = ('glogits', 'gboxes', 'gat', 'gat_p')
        _note('criterion_bwd', K.check_bwd(tuple(_np(x) for x in second), ref['bwd'][mode], inp),
              dict(zip(names, (_np(x) for x in second))), dict(zip(names, ref['bwd'][mode])))


# ------------------------------------------------------------------------------------------------ postprocess
@pytest.mark.parametrize('c', TC.POST, ids=_ids(TC.POST))
def test_postprocess(c):
    from sound_event_detection_transformer_amd import ops
    lib = _lib()
    inp = K.post_inputs(c)
    ref = K.post_ref(inp)
    B, Q, Cn = c.shape['B'], c.shape['Q'], c.shape['C']
    lg, bx, tg, sz = _dev(inp['logits']), _dev(inp['boxes']), _dev(inp['tags']), _dev(inp['sizes'])
    first = ops.postprocess(lg, bx, sizes=sz, tags=tg, at_m=inp['at_m'], is_semi=inp['semi'], threshold=inp['threshold'])
    o = Out().add('scores', (B, Q)).add('labels', (B, Q), torch.int64).add('boxes', (B, Q, 2)).build()
    assert lib.load().sedt_postprocess(_p(lg), _p(bx), _p(tg), _p(sz), B, Q, Cn, inp['at_m'], inp['threshold'], int(inp['semi']),
                                       _p(o['scores']), _p(o['labels']), _p(o['boxes']), lib.stream_ptr()) == 0
    o.check()
    assert all(_same(x, o[k]) for x, k in zip(first, ('scores', 'labels', 'boxes'))), 'a second launch differs'
    got = {k: _np(o[k]) for k in ('scores', 'labels', 'boxes')}
    _note('post', K.check_post(got, ref, inp), got, ref)


# ------------------------------------------------------------------------------------------------ pseudo labels
@pytest.mark.parametrize('c', TC.PSEUDO, ids=_ids(TC.PSEUDO))
def test_pseudo_labels(c):
    from sound_event_detection_transformer_amd import ops
    inp = K.pseudo_inputs(c)
    ref = K.pseudo_ref(inp)
    B, Cn, cap, n = inp['B'], inp['C'], inp['cap'], int(ref['off'][-1])
    # lab_cat[:cap] / box_cat[:cap] are views of a larger NaN-filled buffer: a write past cap, or past the kept events, is seen
    o = (Out().add('lab_cat', (cap,), torch.int64, written=n).add('box_cat', (cap, 2), written=2 * n)
         .add('lab_off', (B + 1,), torch.int32).add('box_off', (B + 1,), torch.int32).add('counter', (Cn,), torch.int32).build())
    tables = {k: o[k] for k in ('lab_cat', 'box_cat', 'lab_off', 'box_off')}
    lg, bx, at, thr = _dev(inp['logits']), _dev(inp['boxes']), _dev(inp['at']), _dev(inp['thr'])

    def run():
        ops.pseudo_labels(lg, bx, at, thr, inp['min_len'], tables, counter=o['counter'], del_overlap=inp['nms'])
    o['counter'].zero_()
    run()
    img = o.check()
    got = dict(lab_cat=_np(o['lab_cat'])[:n], box_cat=_np(o['box_cat'])[:n], lab_off=_np(o['lab_off']), box_off=_np(o['box_off']),
               hist=_np(o['counter']))
    _note('pseudo', K.check_pseudo(got, ref))
    run()                                                    # the counter accumulates over calls
    assert np.array_equal(_np(o['counter']), 2 * ref['hist'])
    o.reset()
    o['counter'].zero_()
    run()
    assert np.array_equal(img, o.check()), 'a second launch differs'


# ------------------------------------------------------------------------------------------------ feature loss, sum, scale
@pytest.mark.parametrize('c', TC.FEATURE, ids=_ids(TC.FEATURE))
def test_feature_loss(c):
    from sound_event_detection_transformer_amd import ops
    lib = _lib()
    inp = K.feature_inputs(c)
    ref = K.feature_ref(inp)
    L, B, ns, Q, P, Fd = (inp[k] for k in ('L', 'B', 'ns', 'Q', 'P', 'F'))
    pred, gt, wbox, tidx = _dev(inp['pred']), _dev(inp['gt']), _dev(inp['wbox']), _dev(inp['tidx'])
    nb, w, base = _dev(np.asarray([inp['num_boxes']], F)), _dev(inp['w']), None if inp['base'] is None else _dev(np.asarray([inp['base']], F))
    first = ops.feature_loss(pred, gt, {'wbox': wbox, 'tidx': tidx, 'ns': ns, 'L': L}, inp['layer_of'], nb, w=w, base=base)
    o = Out().add('rowloss', (L, ns, Q)).add('out', (L + 1,)).add('dpred', (L, B, Q, Fd))
    if base is not None:
        o.add('total', (1,))
    o.build()
    lay = (C.c_int32 * L)(*inp['layer_of'])
    assert lib.load().sedt_feature_loss(_p(pred), _p(gt), _p(wbox), _p(tidx), _p(nb), lay, _p(w), L, B, ns, Q, P, Fd, _p(o['rowloss']),
                                        _p(o['out']), _p(o['dpred']), None, _p(base), _p(o.v.get('total')), lib.stream_ptr()) == 0
    o.check()
    assert _same(first[0], o['out']) and _same(first[1], o['dpred']) and (base is None or _same(first[2].reshape(1), o['total']))
    got = dict(out=_np(o['out']), rowloss=_np(o['rowloss']), dpred=_np(o['dpred']), total=None if base is None else _np(o['total'])[0])
    _note('feature', K.check_feature(got, ref), got, ref)


@pytest.mark.parametrize('n', TC.SUM_N)
def test_sum_f32(n):
    from sound_event_detection_transformer_amd import ops
    lib = _lib()
    x = K.sum_input(n)
    o = Out().add('x', (max(n, 1),)).add('out', (1,)).build()
    if n:
        o['x'].copy_(_dev(x))
        xin = o['x']
        o.before = o.image()
        ops.sum_f32(xin, out=o['out'])
    else:                                                    # an empty tensor has no pointer to give: the entry point itself, n = 0
        assert lib.load().sedt_sum_f32(_p(o['x']), 0, _p(o['out']), lib.stream_ptr()) == 0
    img = o.check(only=('out',))
    r = K.check_sum(_np(o['out'])[0], x)
    RATIOS['sum_f32'] = max(RATIOS['sum_f32'], r)
    assert r <= 1, (n, _np(o['out']), x.astype(np.float64).sum())
    o['out'].fill_(float('nan'))
    assert lib.load().sedt_sum_f32(_p(o['x']), n, _p(o['out']), lib.stream_ptr()) == 0
    assert np.array_equal(img, o.check(only=('out',))), 'a second launch differs'


@pytest.mark.parametrize('c', TC.SCALE, ids=_ids(TC.SCALE))
def test_scale_layers(c):
    from sound_event_detection_transformer_amd import ops
    inp = K.scale_inputs(c)
    o = Out().add('x', inp['x'].shape).build()
    g, gtot, w, x0 = _dev(inp['g']), _dev(inp['gtot']), _dev(inp['w']), _dev(inp['x'])
    o['x'].copy_(x0)
    ops.scale_layers(o['x'], g, gtot, w, idx=inp['idx'])
    img = o.check()
    r = K.check_scale(_np(o['x']), inp)
    RATIOS['scale_layers'] = max(RATIOS['scale_layers'], r)
    assert r <= 1, (c.name, r, K.worst(_np(o['x']), K.scale_ref(inp)))
    o['x'].copy_(x0)
    ops.scale_layers(o['x'], g, gtot, w, idx=inp['idx'])
    assert np.array_equal(img, o.check()), 'a second launch differs'


# ------------------------------------------------------------------------------------------------ refused calls
def _match_args(inp, tables, dense, assign, lg, bx, rand):
    """the SedtMatch of a row, as ops.match_targets fills it"""
    lib = _lib()
    a = lib.SedtMatch()
    a.logits, a.boxes = lg.data_ptr(), bx.data_ptr()
    for k in ('lab_cat', 'lab_off', 'box_cat', 'box_off'):
        setattr(a, k, tables[k].data_ptr())
    for k in ('tc', 'coef', 'wbox', 'tbox', 'tidx', 'tgt_len', 'gt_weak'):
        setattr(a, k, dense[k].data_ptr())
    a.assign = assign.data_ptr()
    a.L, a.B, a.ns, a.Q, a.C, a.n_lab, a.max_targets, a.Qs, a.q0 = (inp[k] for k in ('L', 'B', 'ns', 'Q', 'C', 'n_lab', 'mt', 'Qs', 'q0'))
    for i, l in enumerate(inp['layer_of']):
        a.layer_of[i] = l
    a.w_class, a.w_bbox, a.w_giou, a.alpha_fl, a.gamma_fl, a.epsilon, a.alpha = K.W_CLASS, K.W_BBOX, K.W_GIOU, K.ALPHA_FL, K.GAMMA_FL, 1.0, 1.0
    a.ft_rand = rand.data_ptr()
    return a


def test_refused_calls():
    """calls the entry points reject before launching: non-zero, sedt_last_error names the entry point, no byte changes"""
    from sound_event_detection_transformer_amd import ops
    lib = _lib()
    l = lib.load()

    def untouched(o, entry):
        torch.cuda.synchronize()
        assert np.array_equal(o.before, o.image()), f'{entry}: a refused call wrote'

    def refused(rc, entry, why, o):
        """why: a fragment of the reason this call is to be refused for, so that a refusal for another reason does not pass"""
        msg = l.sedt_last_error()
        assert rc != 0 and msg.startswith(entry.encode() + b':') and why.encode() in msg, (entry, why, rc, msg)
        untouched(o, entry)

    # ---- match_targets
    c = next(c for c in TC.MATCH if c.name == 'ratio_mt63')
    inp = K.match_inputs(c)
    o, dense = _dense_out(inp)
    tables = _tables(inp)
    args = (inp, tables, dense, o['assign'], _dev(inp['logits']), _dev(inp['boxes']), _dev(inp['ft_rand']))
    for what, why in ((dict(Q=64, Qs=64), 'Q=64 (<=63)'), (dict(C=64), 'C=64'), (dict(L=9), 'L=9'), (dict(max_targets=0), 'max_targets=0'),
                      (dict(max_targets=64), 'max_targets=64'), (dict(q0=1), 'query window'), (dict(fine_tune=1), 'fine_tune'),
                      (dict(ns=inp['B'] + 1), f"ns={inp['B'] + 1}")):
        a = _match_args(*args)
        if 'fine_tune' in what:                               # fine-tune with ratios and without normalize: undefined in the reference
            a.ratio_cat = tables['ratio_cat'].data_ptr()
        for k, v in what.items():
            setattr(a, k, v)
        refused(l.sedt_match_targets(a, lib.stream_ptr()), 'match_targets', why, o)
    # ---- set_criterion / set_criterion_bwd
    ci = K.crit_inputs(next(c for c in TC.CRITERION if c.name == 'l1'))
    out, total, state, nonfinite, keep = _crit_launch(ci)
    a = state[0]
    L, B, Q, C1 = ci['L'], ci['B'], ci['Q'], ci['C'] + 1
    o = Out().add('out', (4 * L + 6,)).add('total', (1,)).add('dl', (L, B, Q, C1)).add('db', (L, B, Q, 2)).add('db2', (L, B, Q, 2)) \
        .add('dat', (ci['Bat'], ci['C'])).add('gl', (L, B, Q, C1)).add('gb', (L, B, Q, 2)).build()
    a.out, a.total, a.dlogits, a.dboxes, a.dboxes2, a.dat = (o[k].data_ptr() for k in ('out', 'total', 'dl', 'db', 'db2', 'dat'))
    scratch = torch.empty(9 * B * Q * 5, device='cuda', dtype=torch.float32)
    g = _dev(ci['g'])
    for what, why in ((dict(L=9), 'L=9'), (dict(L=1, B=8193), 'L*B = 8193 exceeds'), (dict(q0=1), 'query window'), (dict(C=64), 'C=64'),
                      (dict(L=0), 'L=0')):
        old = {k: getattr(a, k) for k in what}
        for k, v in what.items():
            setattr(a, k, v)
        refused(l.sedt_set_criterion(a, _p(scratch), lib.stream_ptr()), 'set_criterion', why, o)
        if 'L' in what and 'B' not in what:
            refused(l.sedt_set_criterion_bwd(a, _p(g), None, _p(o['gl']), _p(o['gb']), None, None, lib.stream_ptr()), 'set_criterion_bwd',
                    why, o)
        for k, v in old.items():
            setattr(a, k, v)
    # ---- pseudo_labels: B Q whose LDS exceeds 150 KB ((2 B + 1 + 3 B Q + C) words: B = 198 at Q = 64 needs 150.06 KB)
    Bq, Qq, Cq = 198, 64, 10
    assert (2 * Bq + 1 + 3 * Bq * Qq + Cq) * 4 > 150 * 1024 >= (2 * (Bq - 1) + 1 + 3 * (Bq - 1) * Qq + Cq) * 4
    o = Out().add('lab_cat', (Bq * Qq,), torch.int64).add('box_cat', (Bq * Qq, 2)).add('lab_off', (Bq + 1,), torch.int32) \
        .add('box_off', (Bq + 1,), torch.int32).build()
    lg, bx, thr = torch.zeros(Bq, Qq, Cq + 1, device='cuda'), torch.zeros(Bq, Qq, 2, device='cuda'), torch.zeros(Cq, device='cuda')
    with pytest.raises(RuntimeError, match="pseudo_labels: B\\*Q = 12672 is too large for one workgroup's LDS"):
        ops.pseudo_labels(lg, bx, None, thr, 0.05, {k: o[k] for k in ('lab_cat', 'box_cat', 'lab_off', 'box_off')})
    untouched(o, 'pseudo_labels')
    # ---- feature_loss: F % 4 != 0
    fi = K.feature_inputs(next(c for c in TC.FEATURE if c.name == 'f4_rows5'))
    o = Out().add('rowloss', (5,)).add('out', (2,)).add('dpred', (1, 1, 5, 6)).build()
    t = [_dev(np.zeros((1, 1, 5, 6), F)), _dev(np.zeros((3, 6), F)), _dev(fi['wbox']), _dev(fi['tidx']), _dev(np.ones(1, F))]
    rc = l.sedt_feature_loss(*(_p(x) for x in t), (C.c_int32 * 1)(0), None, 1, 1, 1, 5, 3, 6, _p(o['rowloss']), _p(o['out']), _p(o['dpred']),
                             None, None, None, lib.stream_ptr())
    refused(rc, 'feature_loss', 'F=6', o)
    # ---- scale_layers: per_layer % 4 != 0
    o = Out().add('x', (2, 6)).build()
    with pytest.raises(RuntimeError, match='scale_layers: per_layer=6 must be a multiple of 4'):
        ops.scale_layers(o['x'], _dev(np.ones(2, F)), None, None)
    untouched(o, 'scale_layers')
