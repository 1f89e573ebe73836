"""Inputs, float64 references and comparators for the kernels that decide what the model is trained towards (csrc/criterion.hip:
match_targets, set_criterion, set_criterion_bwd; csrc/postproc.hip: postprocess, pseudo_labels, feature_loss, sum_f32, scale_layers).
A helper of tests/test_target_envelope_gpu.py and tests/test_target_check_cpu.py, not a conftest; the rows are in
tests/target_cases.py.  Everything here runs on the host: numpy, torch on the CPU, scipy and oracle.criterion_oracle.

References (all take the float32 inputs and compute in float64; ``dt=float32`` turns each into the float32 restatement the CPU
module feeds to the comparators):

matching      cost = w_bbox L1 + w_class class cost + w_giou (-GIoU) on (centre, length) intervals, class cost -softmax or the focal
              form of HungarianMatcher, solved by scipy.optimize.linear_sum_assignment; fine-tune re-matching with the injected
              uniforms (the k-th candidate query of a clip, ascending, takes the k-th), normalize and positional ratios as the matcher
              hands them out; then the dense targets exactly as SetCriterion.prepare lays them out (dense layer 0 = the final decoder
              layer; a clip at or beyond the split's strong count gets "no target" rows).
criterion     the oracle SetCriterion's own loss functions under a float64 default dtype, fed per dense layer with the targets and
              index pairs the dense tables describe; per-term gradients and the gradient of the weighted total by autograd.  The
              backward launches with a gradient on single entries of the loss vector combine the per-term gradients linearly.
postprocess   softmax, the per-class best query (first maximum) lifted to the threshold (at_m 2, 3), the tag product (at_m 1, 2), the
              best class (first maximum), boxes as (onset, offset) x duration or left alone (is_semi).
pseudo labels tag gate, score >= threshold of the best class and length > min_len, survivors by descending score (or in query order
              without overlap removal), an event dropped when a kept one of its class shares a non-empty interval with it, kept events
              counted per class only when overlaps are removed; offsets clamp at cap and the tail is dropped.
feature loss  |normalize(s) - normalize(t)|^2 / num_boxes over the matched rows (x / max(|x|, 1e-12)), gradient by autograd.

Bounds.  Index outputs (tc, tidx, assign, tgt_len, labels, offsets, counters, kept events) and copied values (tbox, pseudo-label
boxes) are compared bit for bit.  coef / wbox are a copied ratio, 1, or ONE float32 division 1 / count: 2 u relative (u = 2^-24; a
division is charged one ulp).  gt_weak adds at most n ratios in float32: (n + 1) u times the sum.  Loss values: 1e-5 relative to
max(1, |ref|), 2e-5 for the focal variants; gradients 1e-5 + 1e-4 max|ref| per tensor; feature loss 1e-7 + 1e-5 |ref|, its gradient
1e-6 + 1e-4 max|ref| per (layer, clip, query) row; postprocess scores and boxes rtol 2e-6, atol 1e-7: the numbers tests/test_criterion_gpu.py and
tests/test_criterion_variants_gpu.py hold the same kernels to.  The longest sums of the table (C = 63: 64 terms per row; L B = 8192:
1024 rows per layer, 16 per lane and a 6-step wave reduction, about 22 roundings) stay below these: 22 u = 1.3e-6 relative, and the
float32 restatements of tests/test_target_check_cpu.py confirm it, so no row needs a wider bound.  sum_f32: (ceil(n / 256) + 9) u
times the sum of magnitudes; scale_layers: 2 u (|g| + |gtot w|) |x| for the factor, whose terms may cancel, and u |ref| for the product.  A reference value that is
not finite (the row without any event divides by zero) must be met by the same inf / NaN; a finite one by a finite result.
"""
import contextlib

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from oracle.criterion_oracle import build_oracle_criterion

F = np.float32
U = 2.0 ** -24
W_CLASS, W_BBOX, W_GIOU = 1.0, 5.0, 2.0
ALPHA_FL, GAMMA_FL = 0.5, 1.0
EOS = float(F(0.1))
GUARD = 64                       # guard elements (4 bytes each) on both sides of every output
REL_LOSS, REL_FOCAL = 1e-5, 2e-5


def np_dt(dt):
    return np.float64 if dt in (np.float64, torch.float64) else np.float32


def t_dt(dt):
    return torch.float64 if dt in (np.float64, torch.float64) else torch.float32


# ------------------------------------------------------------------------------------------------ comparators
def cmp_exact(got, ref):
    """0 when equal bit for bit (same shape, same values), inf otherwise"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return float('inf')
    return 0.0 if np.array_equal(got, ref.astype(got.dtype), equal_nan=True) else float('inf')


def cmp_bound(got, ref, bound):
    """largest |got - ref| / bound; inf where the finite / inf / NaN pattern differs"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return float('inf')
    if got.size == 0:
        return 0.0
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin) or not np.array_equal(np.isnan(got), np.isnan(ref)):
        return float('inf')
    inf = np.isinf(ref)
    if inf.any() and not np.array_equal(got[inf], ref[inf]):
        return float('inf')
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / bound[fin]))


def cmp_loss(got, ref, rel=REL_LOSS):
    ref = np.asarray(ref, np.float64)
    return cmp_bound(got, ref, rel * np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 1.0))))


def cmp_grad(got, ref, a=1e-5, r=1e-4):
    ref = np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    return cmp_bound(got, ref, a + r * (np.abs(ref[fin]).max() if fin.any() else 0.0))


def cmp_close(got, ref, rtol=2e-6, atol=1e-7):
    ref = np.asarray(ref, np.float64)
    return cmp_bound(got, ref, atol + rtol * np.abs(np.where(np.isfinite(ref), ref, 1.0)))


def worst(got, ref):
    """index and values of the largest difference (for messages)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or got.size == 0:
        return f'shapes {got.shape} {ref.shape}'
    d = np.abs(got - ref)
    d[~np.isfinite(d)] = np.inf
    d[np.isnan(got) & np.isnan(ref)] = 0
    d[np.isinf(got) & (got == ref)] = 0
    i = np.unravel_index(np.argmax(d), d.shape)
    return f'at {tuple(int(k) for k in i)}: got {got[i]!r} ref {ref[i]!r}'


def guard_check(before, after, regions):
    """first changed byte outside the written regions [(first byte, bytes)], or None.  before / after: uint8 images of one buffer"""
    before, after = np.asarray(before, np.uint8), np.asarray(after, np.uint8)
    assert before.shape == after.shape
    free = np.ones(before.size, bool)
    for o, n in regions:
        free[o:o + n] = False
    bad = np.nonzero(free & (before != after))[0]
    return None if bad.size == 0 else int(bad[0])


class Arena(object):
    """layout of the outputs of one row in ONE buffer of 4-byte words: every output gets GUARD words before and after and starts on a
    multiple of 16 words.  add() returns the first word; regions() the written byte ranges."""

    def __init__(self):
        self.slots, self.words = {}, GUARD

    def add(self, name, nbytes):
        o = (self.words + 15) // 16 * 16
        self.slots[name] = (o, nbytes)
        self.words = o + (nbytes + 3) // 4 + GUARD
        return o

    def regions(self, only=None):
        return [(4 * o, n) for k, (o, n) in self.slots.items() if only is None or k in only]


# ------------------------------------------------------------------------------------------------ matching: inputs
def dense_numel(L, ns, Q, n_lab, C, B):
    return 6 * L * ns * Q + n_lab * C + B + 1


def match_inputs(c):
    s, f = c.shape, c.flags
    rng = np.random.default_rng(c.seed)
    L, B, ns, n_lab, Q, Qs, q0, C = (s[k] for k in ('L', 'B', 'ns', 'n_lab', 'Q', 'Qs', 'q0', 'C'))
    logits = (rng.standard_normal((L, B, Qs, C + 1)) * 2).astype(F)
    boxes = np.stack([rng.uniform(0.1, 0.9, (L, B, Qs)), rng.uniform(0.02, 0.5, (L, B, Qs))], -1).astype(F)
    labels, tboxes, ratios = [], [], []
    for b in range(B):
        n = s['n'][b % len(s['n'])] if b < ns else (int(rng.integers(1, 4)) if b < n_lab else 0)
        ln = rng.uniform(0.02, 0.5, n)
        labels.append(rng.integers(0, C, n).astype(np.int64))
        tboxes.append(np.stack([ln / 2 + rng.uniform(0, 1, n) * (1 - ln), ln], -1).astype(F).reshape(n, 2))
        ratios.append(rng.uniform(0.2, 1.0, n).astype(F))
    if f.get('tie'):                      # queries 0 and 1 identical, targets 0 and 1 identical, in every layer and clip
        logits[:, :, q0 + 1] = logits[:, :, q0]
        boxes[:, :, q0 + 1] = boxes[:, :, q0]
        for b in range(ns):
            labels[b][1], tboxes[b][1] = labels[b][0], tboxes[b][0]
    if f.get('special') == 'coincident':
        # dyadic numbers, exact in float32 and float64.  target 0 [0.125, 0.375] / query 0 [0.125, 0.3125]: equal starts;
        # target 1 [0.5, 0.75] / query 1 [0.5625, 0.75]: equal ends; target 2 [0.8125, 0.9375] / query 2 [0.6875, 0.8125]: touching
        labels[0][:] = (0, 1, 2)
        tboxes[0][:] = ((0.25, 0.25), (0.625, 0.25), (0.875, 0.125))
        boxes[0, 0, q0:q0 + 3] = ((0.21875, 0.1875), (0.65625, 0.1875), (0.75, 0.125))
        boxes[0, 0, q0 + 3] = (0.0625, 0.0625)
        logits[0, 0, q0:q0 + 4] = 0
        for i in range(3):
            logits[0, 0, q0 + i, i] = 6
        logits[0, 0, q0 + 3, C] = 6
    inp = dict(s, logits=logits, boxes=boxes, labels=labels, tboxes=[tboxes[b] for b in range(ns)],
               ratios=ratios if f.get('ratio') else None, layer_of=[L - 1] + list(range(L - 1)),
               ft_rand=rng.uniform(0, 1, (max(ns, 1), Q)).astype(F), fl=bool(f.get('fl')), ft=bool(f.get('ft')),
               norm=bool(f.get('norm')), eps=float(f.get('eps', 1.0)), alpha=float(f.get('alpha', 1.0)))
    inp['ns_eff'] = ns if s['split'] is None else min(s['split'][0], ns)
    inp['n_lab_eff'] = n_lab if s['split'] is None else min(s['split'][1], n_lab)
    return inp


def flat_tables(inp):
    """the flat tables of TargetTables: lab_cat int64, lab_off int32 [B + 1], box_cat f32 [N, 2], box_off int32 [ns + 1], ratio_cat"""
    B, ns = inp['B'], inp['ns']
    lab_off = np.concatenate([[0], np.cumsum([len(l) for l in inp['labels']])]).astype(np.int32)
    box_off = np.concatenate([[0], np.cumsum([len(t) for t in inp['tboxes']])]).astype(np.int32)
    cat = lambda xs, dt, tail: np.concatenate([np.asarray(x, dt).reshape((-1,) + tail) for x in xs] + [np.zeros((1,) + tail, dt)])
    return dict(lab_cat=cat(inp['labels'], np.int64, ()), lab_off=lab_off, box_cat=cat(inp['tboxes'], F, (2,)), box_off=box_off,
                ratio_cat=None if inp['ratios'] is None else cat(inp['ratios'], F, ()))


# ------------------------------------------------------------------------------------------------ matching: reference
def _se(box):
    return box[..., 0] - box[..., 1] / 2, box[..., 0] + box[..., 1] / 2


def cost_matrices(x, qbox, lab, tbox, fl, dt=np.float64):
    """(cost, loc) [Q, n] of one problem: x [Q, C + 1] logits, qbox [Q, 2], lab [n], tbox [n, 2]"""
    dt = np_dt(dt)
    x, qbox, tbox = x.astype(dt), qbox.astype(dt), tbox.astype(dt)
    if fl:
        p = 1 / (1 + np.exp(-x))
        neg = dt(1 - ALPHA_FL) * p ** dt(GAMMA_FL) * (-np.log(1 - p + dt(1e-8)))
        pos = dt(ALPHA_FL) * (1 - p) ** dt(GAMMA_FL) * (-np.log(p + dt(1e-8)))
        cc = (pos - neg)[:, lab]
    else:
        e = np.exp(x - x.max(-1, keepdims=True))
        cc = -(e / e.sum(-1, keepdims=True))[:, lab]
    s1, e1 = (v[:, None] for v in _se(qbox))
    s2, e2 = (v[None, :] for v in _se(tbox))
    l1 = np.abs(s1 - s2) + np.abs(e1 - e2)
    inter = np.maximum(np.minimum(e1, e2) - np.maximum(s1, s2), 0)
    uni = (e1 - s1) + (e2 - s2) - inter
    hull = np.maximum(np.maximum(e1, e2) - np.minimum(s1, s2), 0)
    giou = inter / uni - (hull - uni) / hull
    loc = dt(W_BBOX) * l1 - dt(W_GIOU) * giou
    return loc + dt(W_CLASS) * cc, loc


def _problem(inp, d, b):
    ml, q0, Q = inp['layer_of'][d], inp['q0'], inp['Q']
    n = len(inp['tboxes'][b])
    return inp['logits'][ml, b, q0:q0 + Q], inp['boxes'][ml, b, q0:q0 + Q], inp['labels'][b][:n], inp['tboxes'][b]


def solve(cost):
    """assignment [Q] (target index or -1) of one cost matrix [Q, n]"""
    asg = -np.ones(cost.shape[0], np.int32)
    if cost.shape[1]:
        r, col = linear_sum_assignment(cost)
        asg[r] = col
    return asg


def match_ref(inp, dt=np.float64, margins=None):
    """dense targets + assign of a row.  margins (a list) collects how far the fine-tune comparisons sit from their thresholds"""
    L, B, ns, n_lab, Q, C = (inp[k] for k in ('L', 'B', 'ns', 'n_lab', 'Q', 'C'))
    tc = np.full((L, ns, Q), C, F)
    coef, wbox, tidx = np.ones((L, ns, Q), F), np.zeros((L, ns, Q), F), np.zeros((L, ns, Q), F)
    tbox = np.full((L, ns, Q, 2), 0.5, F)
    assign = -np.ones((L, ns, Q), np.int32)
    for d in range(L):
        for b in range(min(inp['ns_eff'], ns)):
            x, qb, lab, tb = _problem(inp, d, b)
            n = len(tb)
            if n == 0:
                continue
            cost, loc = cost_matrices(x, qb, lab, tb, inp['fl'], dt)
            asg = solve(cost)
            cf = np.ones(Q, F)
            if inp['ft'] and d == 0:
                near_t, near_c = loc.argmin(1), loc.min(1)
                hung, close = asg >= 0, near_c < inp['eps']
                extra = np.nonzero(close & ~hung)[0]
                u = inp['ft_rand'][b][:len(extra)]
                keep_p = inp['alpha'] * int(hung.sum()) / Q
                if margins is not None:
                    margins += [np.abs(near_c - inp['eps']).min(), np.abs(u.astype(np.float64) - keep_p).min() if len(u) else 1.0,
                                np.ptp(np.partition(loc, 1, axis=1)[:, :2], axis=1).min() if n > 1 else 1.0]
                new = np.where(hung & close, asg, -1)
                add = extra[~(u > keep_p)]
                new[add] = near_t[add]
                asg = new.astype(np.int32)
                if inp['norm']:
                    cnt = (asg[:, None] == asg[None, :]).sum(1)
                    cf = (F(1) / np.maximum(cnt, 1).astype(F)).astype(F)
            elif not (inp['norm'] and d == 0) and inp['ratios'] is not None:
                m = asg >= 0
                kth = np.cumsum(m) - m                       # matched queries before this one
                r = inp['ratios'][b]
                cf = r[np.minimum(kth, len(r) - 1)]
            m = asg >= 0
            a = np.clip(asg, 0, None)
            assign[d, b] = asg
            tc[d, b] = np.where(m, lab[a], C)
            coef[d, b] = np.where(m, cf, 1)
            wbox[d, b] = np.where(m, cf, 0)
            tbox[d, b] = np.where(m[:, None], tb[a], 0.5)
            tidx[d, b] = a
    tgt_len = np.asarray([len(l) for l in inp['labels']], F)
    gt_weak = np.zeros((n_lab, C), np_dt(dt))
    for b in range(min(inp['n_lab_eff'], n_lab)):
        r = inp['ratios'][b] if inp['ratios'] is not None else np.ones(len(inp['labels'][b]), F)
        np.add.at(gt_weak[b], inp['labels'][b], r.astype(np_dt(dt)))
    return dict(tc=tc, coef=coef, wbox=wbox, tbox=tbox, tidx=tidx, assign=assign, tgt_len=tgt_len, gt_weak=np.clip(gt_weak, 0, 1))


def assignment_stable(inp):
    """every problem of the row: scipy on the float64 costs and on their float32 roundings gives the same assignment"""
    for d in range(inp['L']):
        for b in range(min(inp['ns_eff'], inp['ns'])):
            x, qb, lab, tb = _problem(inp, d, b)
            if len(tb) == 0:
                continue
            cost, _ = cost_matrices(x, qb, lab, tb, inp['fl'])
            if not np.array_equal(solve(cost), solve(cost.astype(F).astype(np.float64))):
                return False
    return True


def host_assign(inp):
    """the host solver's assignment (csrc/host.cpp, sedt_hungarian_batch) on the float32 roundings of the float64 costs"""
    from sound_event_detection_transformer_amd import lib
    L, ns, Q = inp['L'], inp['ns'], inp['Q']
    sizes = np.asarray([len(t) for t in inp['tboxes']], np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    Nt = int(sizes.sum())
    cost = np.zeros((L, ns, Q, Nt), F)
    for d in range(L):
        for b in range(ns):
            if sizes[b]:
                cost[d, b, :, off[b]:off[b] + sizes[b]] = cost_matrices(*_problem(inp, d, b), inp['fl'])[0].astype(F)
    assign = -np.ones((L, ns, Q), np.int32)
    rc = lib.load().sedt_hungarian_batch(cost.ctypes.data, L, ns, Q, Nt, off.ctypes.data, sizes.ctypes.data, assign.ctypes.data)
    assert rc == 0, lib.load().sedt_last_error()
    return assign


def check_tie(inp, assign):
    """a tie row: every assignment is one-to-one, complete, and as cheap (in float64) as scipy's optimum.  Returns the largest relative
    cost excess (must be ~0) or inf"""
    worst_ = 0.0
    for d in range(inp['L']):
        for b in range(inp['ns']):
            x, qb, lab, tb = _problem(inp, d, b)
            cost, _ = cost_matrices(x, qb, lab, tb, inp['fl'])
            a = np.asarray(assign[d, b])
            m = a >= 0
            if m.sum() != min(cost.shape) or len(set(a[m].tolist())) != m.sum() or a.max() >= cost.shape[1]:
                return float('inf')
            r, col = linear_sum_assignment(cost)
            opt, got = cost[r, col].sum(), cost[np.nonzero(m)[0], a[m]].sum()
            worst_ = max(worst_, abs(got - opt) / max(1.0, abs(opt)))
    return worst_


def check_dense(got, ref, inp, tie=False):
    """{output: ratio} of the dense targets.  tie rows: assign-dependent outputs are compared by the caller against the host solver"""
    n = max([len(l) for l in inp['labels']] + [1])
    r = {k: cmp_exact(got[k], ref[k]) for k in ('tc', 'tidx', 'assign', 'tgt_len', 'tbox')}
    r['coef'] = cmp_bound(got['coef'], ref['coef'], 2 * U * np.abs(ref['coef']) + 1e-30)
    r['wbox'] = cmp_bound(got['wbox'], ref['wbox'], 2 * U * np.abs(ref['wbox']) + 1e-30)
    r['gt_weak'] = cmp_bound(got['gt_weak'], ref['gt_weak'], (n + 1) * U * n + 1e-30)
    return r


def dense_from_assign(inp, assign):
    """the dense targets a given assignment implies (plain rows without ratios / normalize: tie rows)"""
    ref = match_ref(inp)
    out = {k: v.copy() for k, v in ref.items()}
    for d in range(inp['L']):
        for b in range(inp['ns']):
            a = np.asarray(assign[d, b])
            m, ac = a >= 0, np.clip(a, 0, None)
            lab, tb = inp['labels'][b], inp['tboxes'][b]
            out['assign'][d, b] = a
            out['tc'][d, b] = np.where(m, lab[ac], inp['C'])
            out['wbox'][d, b] = m
            out['tbox'][d, b] = np.where(m[:, None], tb[ac], 0.5)
            out['tidx'][d, b] = ac
    return out


def pack_dense(dn, num_boxes=0.0):
    """the packed buffer SetCriterion.dense_views cuts into views"""
    return np.concatenate([dn['tc'].ravel(), dn['coef'].ravel(), dn['wbox'].ravel(), dn['tbox'].ravel(), dn['tidx'].ravel(),
                           dn['gt_weak'].astype(F).ravel(), dn['tgt_len'], np.asarray([num_boxes], F)]).astype(F)


# ------------------------------------------------------------------------------------------------ criterion
@contextlib.contextmanager
def default_dtype(dt):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


def crit_inputs(c):
    inp = match_inputs(c)
    rng = np.random.default_rng(c.seed + 1000)
    L, C = inp['L'], inp['C']
    inp['dense'] = match_ref(inp)
    inp['at'] = None if not c.shape['Bat'] else rng.uniform(0.05, 0.95, (c.shape['Bat'], C)).astype(F)
    inp['at_p'] = None if not c.shape['Bp'] else rng.uniform(0.05, 0.95, (c.shape['Bp'], C)).astype(F)
    inp['wp_all'] = bool(c.flags.get('wp_all'))
    inp['w_ce'] = [1.0 + 0.25 * d for d in range(L)]
    inp['w_bbox'] = [5.0 - 0.5 * d for d in range(L)]
    inp['w_giou'] = [2.0 + 0.125 * d for d in range(L)]
    inp['w_weak'], inp['w_weak_p'] = 0.75, 0.5
    inp['empty_weight'] = np.concatenate([np.ones(C, F), [F(EOS)]]).astype(F)
    nb = F(inp['dense']['wbox'][0].astype(np.float64).sum())
    inp['num_boxes'] = F(nb + F(0.5)) if c.flags.get('nb_given') else None        # given: not the sum, so that a kernel ignoring it shows
    inp['nb'] = float(inp['num_boxes']) if inp['num_boxes'] is not None else float(nb)
    inp['g'] = rng.standard_normal(4 * L + 6).astype(F)
    inp['gtotal'] = F(1.5)
    return inp


SLOTS = lambda L: dict(hit=4 * L, cnt=4 * L + 1, weak=4 * L + 2, total=4 * L + 3, class_error=4 * L + 4, weak_p=4 * L + 5)


def criterion_ref(inp, dt=torch.float64):
    """out [4 L + 6], the per-term gradients (dl, db, db2 in the compact [L, B, Q] layout, dat, dat_p) and the gradients of the head
    outputs for the three backward launches: {'g', 'gtotal', 'both'} -> (glogits, gboxes, gat, gat_p)"""
    dt = t_dt(dt)
    L, B, Q, Qs, q0, C = (inp[k] for k in ('L', 'B', 'Q', 'Qs', 'q0', 'C'))
    ns_eff, n_lab_eff, dn, fl = inp['ns_eff'], inp['n_lab_eff'], inp['dense'], inp['fl']
    with default_dtype(dt):
        crit = build_oracle_criterion(num_classes=C, dec_layers=L, eos_coef=EOS)
        crit.empty_weight = torch.from_numpy(inp['empty_weight']).to(dt)
        lg = torch.from_numpy(inp['logits']).to(dt).requires_grad_(True)
        bx = torch.from_numpy(inp['boxes']).to(dt).requires_grad_(True)
        at = None if inp['at'] is None else torch.from_numpy(inp['at']).to(dt).requires_grad_(True)
        at_p = None if inp['at_p'] is None else torch.from_numpy(inp['at_p']).to(dt).requires_grad_(True)
        nb = torch.tensor([inp['nb']], dtype=dt)
        real = [{'labels': torch.from_numpy(l), **({'ratio': torch.from_numpy(inp['ratios'][b]).to(dt)} if inp['ratios'] is not None else {})}
                for b, l in enumerate(inp['labels'])]
        zero = lambda: torch.zeros((), dtype=dt)
        ce, l1, gi, card = [], [], [], []
        for d in range(L):
            ml = inp['layer_of'][d]
            o = {'pred_logits': lg[ml][:, q0:q0 + Q], 'pred_boxes': bx[ml][:, q0:q0 + Q]}
            tg, idx, cf = [], [], []
            for b in range(ns_eff):
                src = np.nonzero(dn['wbox'][d, b] > 0)[0]
                tg.append({'labels': torch.from_numpy(dn['tc'][d, b, src].astype(np.int64)),
                           'boxes': torch.from_numpy(dn['tbox'][d, b, src]).to(dt).reshape(-1, 2)})
                idx.append((torch.from_numpy(src), torch.arange(len(src))))
                cf.append(torch.from_numpy(dn['coef'][d, b, src]))
            if ns_eff:
                ce.append(crit.loss_labels(o, tg, idx, nb, slice(ns_eff), None, cf, log=False, fl=fl)['loss_ce'])
                lb = crit.loss_boxes(o, tg, idx, nb, slice(ns_eff), None, cf)
                l1.append(lb['loss_bbox'])
                gi.append(lb['loss_giou'])
            else:
                ce.append(zero()), l1.append(zero()), gi.append(zero())
            card.append(crit.loss_cardinality(o, real, None, nb, None, None, None)['cardinality_error'])
        weak, weak_p = zero(), zero()
        if at is not None:
            wm = None if inp['wp_all'] else slice(ns_eff, n_lab_eff)
            lw = crit.loss_weak({'at': at, **({'at_p': at_p} if at_p is not None else {})}, real, None, nb, slice(ns_eff), wm, None, fl=fl)
            weak, weak_p = lw['loss_weak'], lw.get('loss_weak_p', zero())
        x0 = inp['logits'][inp['layer_of'][0], :ns_eff, q0:q0 + Q].astype(np.float64)
        m0 = dn['wbox'][0, :ns_eff] > 0
        cnt = float(m0.sum())
        hit = float(((x0.argmax(-1) == dn['tc'][0, :ns_eff]) & m0).sum())
        total = sum(inp['w_ce'][d] * ce[d] + inp['w_bbox'][d] * l1[d] + inp['w_giou'][d] * gi[d] for d in range(L)) \
            + inp['w_weak'] * weak + inp['w_weak_p'] * weak_p
        out = np.zeros(4 * L + 6)
        for d in range(L):
            out[4 * d:4 * d + 4] = ce[d].item(), l1[d].item(), gi[d].item(), card[d].item()
        s = SLOTS(L)
        out[s['hit']], out[s['cnt']], out[s['weak']], out[s['total']] = hit, cnt, float(weak.detach()), float(total.detach() if torch.is_tensor(total) else total)
        out[s['class_error']], out[s['weak_p']] = 100.0 - 100.0 * hit / max(cnt, 1.0), float(weak_p.detach())

        def grad(y, x):
            if x is None:
                return None
            if not (torch.is_tensor(y) and y.requires_grad):
                return np.zeros(tuple(x.shape))
            g = torch.autograd.grad(y, x, retain_graph=True, allow_unused=True)[0]
            return np.zeros(tuple(x.shape)) if g is None else g.numpy().astype(np.float64)

        full = dict(dl=grad(sum(ce), lg), db=grad(sum(l1), bx), db2=grad(sum(gi), bx), dat=grad(weak, at), dat_p=grad(weak_p, at_p))
        terms = dict(dl=full['dl'][:, :, q0:q0 + Q], db=full['db'][:, :, q0:q0 + Q], db2=full['db2'][:, :, q0:q0 + Q],
                     dat=full['dat'], dat_p=full['dat_p'])
        g, gt_ = inp['g'].astype(np.float64), float(inp['gtotal'])
        inv = np.argsort(inp['layer_of'])                    # model layer -> dense layer

        def combine(gv, gtot):
            gtot = gtot + (gv[s['total']] if gv is not None else 0.0)      # the loss vector's total entry is the weighted total too
            k = lambda slot, w: np.asarray([(gv[4 * d + slot] if gv is not None else 0.0) + gtot * w[d] for d in inv])

            def lay(t, kv):
                with np.errstate(invalid='ignore'):
                    return t * kv.reshape((L,) + (1,) * (t.ndim - 1))
            gl = lay(full['dl'], k(0, inp['w_ce']))
            gb = lay(full['db'], k(1, inp['w_bbox'])) + lay(full['db2'], k(2, inp['w_giou']))
            ga = None if at is None else full['dat'] * ((gv[s['weak']] if gv is not None else 0.0) + gtot * inp['w_weak'])
            gp = None if at_p is None else full['dat_p'] * ((gv[s['weak_p']] if gv is not None else 0.0) + gtot * inp['w_weak_p'])
            return gl, gb, ga, gp
        bwd = {'g': combine(g, 0.0), 'both': combine(g, gt_),
               'gtotal': tuple(None if x is None else grad(total, x) * gt_ for x in (lg, bx, at, at_p))}
    return dict(out=out, terms=terms, bwd=bwd)


def check_criterion(got_out, got_terms, ref, inp):
    L, rel = inp['L'], REL_FOCAL if inp['fl'] else REL_LOSS
    s = SLOTS(L)
    exact = [s['hit'], s['cnt']]                                                 # integer counts
    vals = [i for i in range(4 * L + 6) if i not in exact]
    r = {'out': cmp_loss(np.asarray(got_out)[vals], ref['out'][vals], rel),
         'out counts': cmp_exact(np.asarray(got_out, np.float64)[exact], ref['out'][exact])}
    for k, v in ref['terms'].items():
        if v is not None:
            r[k] = cmp_grad(got_terms[k], v)
    return r


def check_bwd(got, ref, inp):
    """got / ref: (glogits, gboxes, gat, gat_p) in the layout of the head outputs; the rows outside the window must be exactly zero"""
    q0, Q, Qs = inp['q0'], inp['Q'], inp['Qs']
    r = {}
    for k, a, b in zip(('glogits', 'gboxes', 'gat', 'gat_p'), got, ref):
        if b is None:
            continue
        r[k] = cmp_grad(a, b)
        if k in ('glogits', 'gboxes'):
            out = np.ones(Qs, bool)
            out[q0:q0 + Q] = False
            if np.any(np.asarray(a)[:, :, out] != 0):
                r[k] = float('inf')
    return r


# ------------------------------------------------------------------------------------------------ postprocess
def post_inputs(c):
    rng = np.random.default_rng(c.seed)
    B, Q, C = c.shape['B'], c.shape['Q'], c.shape['C']
    logits = (rng.standard_normal((B, Q, C + 1)) * 2).astype(F)
    if c.flags['lane63']:
        logits[:, :, C // 2] -= 6                     # class C // 2 is unlikely everywhere, least so in the last lane: its best query, below
        logits[:, Q - 1] = 0                          # the threshold, so at_m 2 / 3 lift it there
    boxes = np.stack([rng.uniform(0.1, 0.9, (B, Q)), rng.uniform(0.02, 0.5, (B, Q))], -1).astype(F)
    tags = None if c.flags['at_m'] is None else rng.integers(0, 2, (B, C)).astype(F)
    return dict(logits=logits, boxes=boxes, tags=tags, sizes=rng.uniform(5, 10, B).astype(F), at_m=c.flags['at_m'] or 2,
                semi=c.flags['semi'], threshold=0.5)


def post_ref(inp, dt=np.float64):
    dt = np_dt(dt)
    x = inp['logits'].astype(dt)
    e = np.exp(x - x.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True))[..., :-1].copy()
    B, Q, C = prob.shape
    if inp['tags'] is not None:
        tags = inp['tags'].astype(dt)
        if inp['at_m'] in (2, 3):
            for b in range(B):
                for cl in range(C):
                    q = prob[b, :, cl].argmax()
                    if prob[b, q, cl] < inp['threshold'] and (inp['at_m'] == 2 or tags[b, cl] != 0):
                        prob[b, q, cl] = inp['threshold']
        if inp['at_m'] in (1, 2):
            prob = prob * tags[:, None, :]
    bx = inp['boxes'].astype(dt)
    if not inp['semi']:
        sz = inp['sizes'].astype(dt)[:, None]
        bx = np.stack([(bx[..., 0] - bx[..., 1] / 2) * sz, (bx[..., 0] + bx[..., 1] / 2) * sz], -1)
    return dict(scores=prob.max(-1), labels=prob.argmax(-1).astype(np.int64), boxes=bx)


def check_post(got, ref, inp):
    return {'scores': cmp_close(got['scores'], ref['scores']), 'labels': cmp_exact(got['labels'], ref['labels']),
            'boxes': cmp_exact(got['boxes'], inp['boxes']) if inp['semi'] else cmp_close(got['boxes'], ref['boxes'])}


# ------------------------------------------------------------------------------------------------ pseudo labels
def pseudo_inputs(c):
    rng = np.random.default_rng(c.seed)
    B, Q, C = c.shape['B'], c.shape['Q'], c.shape['C']
    logits = (rng.standard_normal((B, Q, C + 1)) * 3).astype(F)
    boxes = np.stack([rng.uniform(0.1, 0.9, (B, Q)), rng.uniform(0.0, 0.5, (B, Q))], -1).astype(F)
    at = rng.uniform(0, 1, (B, C)).astype(F)
    thr = rng.uniform(0.3, 0.5, C).astype(F)
    # clip 0: every query survives the filter (its own class where C allows, far above the threshold, long enough); clip 1: none does
    # (zero lengths); clip 2: every query is a class-0 event over the same stretch: overlap removal keeps one
    logits[0] = 0
    for q in range(Q):
        logits[0, q, q % C] = 8 + F(0.03125) * q
    at[0] = 1
    boxes[0, :, 1] = np.maximum(boxes[0, :, 1], F(0.1))
    boxes[1, :, 1] = 0
    logits[2] = 0
    logits[2, :, 0] = 6 + F(0.0625) * np.arange(Q, dtype=F)
    at[2, 0] = 1
    boxes[2, :, 0], boxes[2, :, 1] = 0.5, F(0.4) + F(0.0009765625) * np.arange(Q, dtype=F)
    inp = dict(logits=logits, boxes=boxes, at=at if c.flags['at'] else None, thr=thr, min_len=0.05, nms=c.flags['nms'], B=B, Q=Q, C=C,
               cap=1 << 30)
    cnt = pseudo_ref(inp)['cnt']
    off = np.concatenate([[0], np.cumsum(cnt)])
    total = int(off[-1])
    if c.flags['cap'] == 'mid':
        k = next(b for b in range(1, B) if cnt[b] >= 2)
        cap = int(off[k]) + 1
    elif c.flags['cap'] == 'boundary':
        k = next(b for b in range(B // 2, B) if 0 < off[b] < total and cnt[b] > 0)
        cap = int(off[k])
    else:
        cap = {'big': total + 7, 'total': total, 'minus1': total - 1}[c.flags['cap']]
    inp['cap'] = cap
    return inp


def pseudo_ref(inp, dt=np.float64):
    dt = np_dt(dt)
    B, Q, C = inp['B'], inp['Q'], inp['C']
    x = inp['logits'].astype(dt)
    e = np.exp(x - x.max(-1, keepdims=True))
    prob = (e / e.sum(-1, keepdims=True))[..., :-1]
    thr = inp['thr'].astype(dt)
    if inp['at'] is not None:
        prob = prob * (inp['at'] >= inp['thr'][None, :])[:, None, :]
    score, label = prob.max(-1), prob.argmax(-1)
    bx = inp['boxes'].astype(dt)
    on, off_ = bx[..., 0] - bx[..., 1] / 2, bx[..., 0] + bx[..., 1] / 2
    ok = (score >= thr[label]) & (bx[..., 1] > dt(inp['min_len']))
    labs, boxes, cnt, hist, surv = [], [], [], np.zeros(C, np.int64), []
    for b in range(B):
        qs = np.nonzero(ok[b])[0]
        surv.append(score[b, qs])
        if inp['nms']:
            qs = qs[np.argsort(-score[b, qs], kind='stable')]
            kept = []
            for q in qs:
                if not any(label[b, k] == label[b, q] and max(min(off_[b, k], off_[b, q]) - max(on[b, k], on[b, q]), 0) != 0 for k in kept):
                    kept.append(q)
            np.add.at(hist, label[b, kept], 1)
        else:
            kept = list(qs)
        labs += [label[b, q] for q in kept]
        boxes += [inp['boxes'][b, q] for q in kept]
        cnt.append(len(kept))
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n = min(int(off[-1]), inp['cap'])
    return dict(lab_cat=np.asarray(labs[:n], np.int64), box_cat=np.asarray(boxes[:n], F).reshape(n, 2),
                off=np.minimum(off, inp['cap']).astype(np.int32), hist=hist.astype(np.int32), cnt=np.asarray(cnt), survivors=surv)


def check_pseudo(got, ref):
    """got: lab_cat / box_cat (the first off[-1] entries), lab_off, box_off, hist"""
    return {'lab_cat': cmp_exact(got['lab_cat'], ref['lab_cat']), 'box_cat': cmp_exact(got['box_cat'], ref['box_cat']),
            'lab_off': cmp_exact(got['lab_off'], ref['off']), 'box_off': cmp_exact(got['box_off'], ref['off']),
            'counter': cmp_exact(got['hist'], ref['hist'])}


# ------------------------------------------------------------------------------------------------ feature loss, sum, scale
def feature_inputs(c):
    rng = np.random.default_rng(c.seed)
    L, B, ns, Q, P, Fd = (c.shape[k] for k in ('L', 'B', 'ns', 'Q', 'P', 'F'))
    pred = rng.standard_normal((L, B, Q, Fd)).astype(F)
    gt = rng.standard_normal((ns * P, Fd)).astype(F)
    wbox = (rng.uniform(0, 1, (L, ns, Q)) * (rng.uniform(0, 1, (L, ns, Q)) < 0.6)).astype(F)
    tidx = rng.integers(0, P, (L, ns, Q)).astype(F)
    layer_of = [L - 1] + list(range(L - 1))
    if c.flags['zero'] == 'pred':
        wbox[0, 0, 0] = 1
        pred[layer_of[0], 0, 0] = 0                   # a live prediction row of zero norm
    if c.flags['zero'] == 'target':
        wbox[1, 1, 1] = 1
        tidx[1, 1, 1] = 2
        gt[1 * P + 2] = 0                             # a zero-norm target row that a live row points at
    wbox[0, 0, Q - 1] = 0.5                           # at least one live row
    return dict(pred=pred, gt=gt, wbox=wbox, tidx=tidx, layer_of=layer_of, L=L, B=B, ns=ns, Q=Q, P=P, F=Fd,
                num_boxes=F(max((wbox[0] > 0).sum(), 1)), w=(1 + 0.25 * np.arange(L)).astype(F),
                base=F(3.25) if c.flags['base'] else None)


def feature_ref(inp, dt=torch.float64):
    dt = t_dt(dt)
    L, ns, P = inp['L'], inp['ns'], inp['P']
    pred = torch.from_numpy(inp['pred']).to(dt).requires_grad_(True)
    gt = torch.from_numpy(inp['gt']).to(dt)
    out, rows = [], np.zeros((L, ns, inp['Q']))
    for d in range(L):
        ml = inp['layer_of'][d]
        b, q = np.nonzero(inp['wbox'][d] > 0)
        sf = torch.nn.functional.normalize(pred[ml][b, q], dim=1)
        tf = torch.nn.functional.normalize(gt[torch.from_numpy(b * P + inp['tidx'][d, b, q].astype(np.int64))], dim=1)
        rl = ((sf - tf) ** 2).sum(1) / float(inp['num_boxes'])
        rows[d, b, q] = rl.detach().numpy()
        out.append(rl.sum())
    dpred = torch.autograd.grad(sum(out), pred)[0].numpy().astype(np.float64)
    o = np.asarray([v.item() for v in out])
    tot = float((inp['w'].astype(np.float64) * o).sum())
    return dict(out=np.concatenate([o, [tot]]), dpred=dpred, rowloss=rows, total=None if inp['base'] is None else tot + float(inp['base']))


def check_feature(got, ref):
    """values: 1e-7 + 1e-5 |ref| (the row losses are divided by num_boxes and sit far below 1).  dpred: 1e-6 + 1e-4 of the largest
    reference magnitude of the SAME (layer, clip, query) row, so that the 1e12-sized gradient of a zero-norm prediction row does not
    widen the bound of any other row, and a row that must be zero faces 1e-6"""
    val = lambda a, b: cmp_close(a, b, rtol=1e-5, atol=1e-7)
    rd = np.asarray(ref['dpred'], np.float64)
    r = {'out': val(got['out'], ref['out']), 'rowloss': val(got['rowloss'], ref['rowloss']),
         'dpred': cmp_bound(got['dpred'], rd, 1e-6 + 1e-4 * np.abs(rd).max(-1, keepdims=True))}
    if ref['total'] is not None:
        r['total'] = val(got['total'], ref['total'])
    return r


def sum_input(n):
    return (np.random.default_rng(200 + n).standard_normal(n) * 3).astype(F)


def check_sum(got, x):
    x = x.astype(np.float64)
    return cmp_bound(got, x.sum(), 2 * (-(-len(x) // 256) + 9) * U * np.abs(x).sum() + 1e-30)


def scale_inputs(c):
    rng = np.random.default_rng(c.seed)
    L = c.shape['L']
    return dict(x=rng.standard_normal((L, c.shape['per'])).astype(F), g=rng.standard_normal(L).astype(F) if c.flags['mode'] != 'gtot' else None,
                gtot=rng.standard_normal(1).astype(F) if c.flags['mode'] != 'g' else None, w=rng.uniform(0.5, 2, L).astype(F), idx=c.flags['idx'])


def scale_k(inp, dt=np.float64):
    dt = np_dt(dt)
    L = inp['x'].shape[0]
    idx = list(range(L)) if inp['idx'] is None else inp['idx']
    return np.asarray([(dt(inp['g'][d]) if inp['g'] is not None else dt(0)) +
                       (dt(inp['gtot'][0]) * dt(inp['w'][d]) if inp['gtot'] is not None else dt(0)) for d in idx], dt)


def scale_ref(inp, dt=np.float64):
    return inp['x'].astype(np_dt(dt)) * scale_k(inp, dt)[:, None]


def check_scale(got, inp):
    """k = g + gtot w rounds its product and its sum (2 u of the magnitudes of both terms: they may cancel), x k once more"""
    kabs = scale_k(dict(inp, g=None if inp['g'] is None else np.abs(inp['g']), gtot=None if inp['gtot'] is None else np.abs(inp['gtot'])))
    ref = scale_ref(inp)
    return cmp_bound(got, ref, 2 * U * (2 * np.abs(inp['x']) * kabs[:, None] + np.abs(ref)) + 1e-30)
