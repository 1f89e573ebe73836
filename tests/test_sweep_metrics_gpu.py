"""GPU: the event-based and clip-level counts at every operating point (csrc/sweep.hip through ops.event_sweep_update,
utilities/operating_points.SweepEventMetrics and the predict steps' ``sweep=``), the class-wise decode (csrc/decode.hip:
sedt_decode_events_classwise) and the thresholds chosen from the counts, against the restatement (tests/sweep_ref.py) applied to the
rows predictions.unpack gives for the SAME records, and against the device yardstick EventMetrics at each threshold.  Every count
comparison is exact integer equality; B = 8 throughout."""
import numpy as np
import pytest
import torch

import event_metrics_ref as ER
import sweep_ref as SR
from test_psds_gpu import C2_CLASSES, GRID9, _batches, _c2_model, _clips, _envelope_case, _records

pytestmark = pytest.mark.gpu

B = 8
GRID9_F32 = np.asarray(GRID9, np.float64).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _table(reference):
    """the device reference table of ops.event_sweep_update: per clip [(class index, onset, offset)] or None -> (table, n_clips,
    max_ref)"""
    off, cls, on, end = [0], [], [], []
    for ev in reference:
        for c, a, b in (ev or ()):
            cls.append(c), on.append(a), end.append(b)
        off.append(len(cls))
    t = {'present': torch.tensor([ev is not None for ev in reference], dtype=torch.int32), 'off': torch.tensor(off, dtype=torch.int32),
         'cls': torch.tensor(cls or [0], dtype=torch.int32), 'on': torch.tensor(on or [0.0], dtype=torch.float64),
         'end': torch.tensor(end or [0.0], dtype=torch.float64)}
    return {k: v.cuda() for k, v in t.items()}, len(reference), int(np.diff(off).max())


def _unpack(records):
    from sound_event_detection_transformer_amd.utilities.predictions import unpack
    return unpack(records.cpu().numpy(), (records.shape[2] - 1) // 5)


def _update(records, clip_idx, reference, C, n_fusion=2, fusion=1, **kw):
    """one event_sweep_update launch into row ``fusion`` of fresh counters -> (ev, tag) [K, C, 3] as numpy; the other rows stay zero"""
    from sound_event_detection_transformer_amd import ops
    table, n_clips, max_ref = _table(reference)
    ev = torch.zeros((n_fusion, records.shape[0], C, 3), dtype=torch.int64).cuda()
    tag = torch.zeros_like(ev)
    ops.event_sweep_update(records, torch.tensor(clip_idx, dtype=torch.int32).cuda(), table, n_clips, max_ref, C, ev, tag, fusion, **kw)
    ev, tag = ev.cpu().numpy(), tag.cpu().numpy()
    assert not np.delete(ev, fusion, axis=0).any() and not np.delete(tag, fusion, axis=0).any()
    return ev[fusion], tag[fusion]


def _named(reference, labels):
    return [None if ev is None else [(labels[c], on, off) for c, on, off in ev] for ev in reference]


# ---------------------------------------------------------------------------------------------------------------- hand-made clip
@pytest.mark.parametrize('del_overlap', [True, False])
def test_hand_worked_clip(del_overlap):
    """clip 0 of a batch of 8 (the others hold nothing), C = 4, thresholds (0.5, 0.95), every score 0.9, t_collar = pct = 0.2:
      class 0  reference onset 0.25 - 0.2 (exact in float64), estimate onset 0.25f: |on_r - on_e| == 0.2, a hit at exactly the collar;
      class 1  the same reference, estimate onset one float32 ulp later: a miss;
      class 2  two estimates that do not overlap each other both hit the one reference event: tp 1 either way, n_sys 2;
      class 3  R1 hits E1 and E2, R2 hits E1 only: the greedy pass gives E1 to R1 and finds nothing for R2 (tp 1), the maximum
               matching pairs R1 - E2, R2 - E1 (tp 2).
    At 0.95 nothing is decoded: every reference event is missed."""
    x = np.float32(0.25)
    beyond = np.nextafter(x, np.float32(1))
    ron = 0.25 - 0.2
    assert abs(ron - float(x)) == 0.2 and abs(ron - float(beyond)) > 0.2
    clip = [(0, float(x), 2.0, 0.9), (1, float(beyond), 2.0, 0.9),
            (2, 4.85, 5.125, 0.9), (2, 5.125, 5.45, 0.9),
            (3, 6.825, 7.05, 0.9), (3, 7.05, 7.3, 0.9)]
    reference = [[(0, ron, 2.0), (1, ron, 2.0), (2, 5.0, 5.3), (3, 7.0, 7.2), (3, 6.7, 6.9)]] + [[]] * (B - 1)
    S, L, X = _clips([clip] + [[]] * (B - 1), 8)
    rec = _records(S, L, X, [0.5, 0.95], 4, del_overlap=del_overlap)
    events = _unpack(rec)
    assert len(events[0]['cls']) == 6 and len(events[1]['cls']) == 0                       # nothing was deleted as an overlap
    idx = list(range(B))
    missed = [[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 2, 0]]
    for optimal, class3 in ((True, 2), (False, 1)):
        ev, tag = _update(rec, idx, reference, 4, optimal=optimal)
        assert ev[0].tolist() == [[1, 1, 1], [0, 1, 1], [1, 1, 2], [class3, 2, 2]], (optimal, ev[0])
        assert ev[1].tolist() == missed
        assert tag[0].tolist() == [[1, 0, 0]] * 4 and tag[1].tolist() == [[0, 0, 1]] * 4
        want = SR.counts(events, idx, reference, 4, optimal=optimal)
        assert np.array_equal(ev, want[0]) and np.array_equal(tag, want[1])


# ---------------------------------------------------------------------------------------------------------------- envelope edges
@pytest.mark.parametrize('Q,C,K,max_ref', [(1, 1, 1, 1), (21, 10, 9, 5), (64, 63, 9, 64)])
def test_envelope_edges(Q, C, K, max_ref):
    """the cases of tests/test_psds_gpu.py at the edges of the kernel's envelope (Q = 64 decodes with del_overlap off: clip 0 keeps
    all 64 queries at the lowest threshold; max_ref = 64: 64 reference events in clip 0).  So that the comparison is not vacuous, the
    restatement's own counts hold a true positive and non-zero clip-level tp, fp and fn at every threshold."""
    reference, S, L, X = _envelope_case(Q, C, max_ref, B, seed=100 + Q)
    assert max(len(e) for e in reference) == max_ref == len(reference[0])
    rec = _records(S, L, X, GRID9 if K == 9 else [0.5], C, del_overlap=Q != 64)
    assert rec.shape == (K, B, 1 + 5 * Q)
    if Q == 64:
        assert int(rec[0, 0, 0]) == 64
    idx = list(range(B))
    want_ev, want_tag = SR.counts(_unpack(rec), idx, reference, C)
    for k in range(K):
        assert want_ev[k, :, 0].sum() > 0, k
        assert all(want_tag[k, :, i].sum() > 0 for i in range(3)), (k, want_tag[k].sum(0))
    ev, tag = _update(rec, idx, reference, C)
    assert np.array_equal(ev, want_ev), np.argwhere(ev != want_ev)[:10]
    assert np.array_equal(tag, want_tag), np.argwhere(tag != want_tag)[:10]


# ---------------------------------------------------------------------------------------------------------------- the device yardstick
@pytest.mark.parametrize('optimal', [True, False])
@pytest.mark.parametrize('del_overlap', [True, False])
def test_every_point_equals_event_metrics_at_that_threshold(optimal, del_overlap):
    """for every k, ev[k] and tag[k] are what EventMetrics(threshold=grid[k]) counts on the same batch; clip 3 has clip_idx -1 and
    clip 5 is given as None in the reference: both count at clip level only"""
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    Q, C = 21, 10
    labels = [f'c{i}' for i in range(C)]
    reference, S, L, X = _envelope_case(Q, C, 5, B, seed=100 + Q)
    reference[5] = None
    idx = [0, 1, 2, -1, 4, 5, 6, 7]
    rec = _records(S, L, X, GRID9, C, del_overlap=del_overlap)
    ev, tag = _update(rec, idx, reference, C, optimal=optimal)
    dev = tuple(torch.from_numpy(t).cuda() for t in (S, L, X))
    seen = 0
    for k, t in enumerate(GRID9_F32):
        m = EventMetrics(labels, 10.0, threshold=float(t), del_overlap=del_overlap, optimal=optimal).set_reference(_named(reference, labels))
        m.update({1: dev}, None, idx)
        want_ev, want_tag = m.counts()
        assert np.array_equal(ev[k], want_ev[0]) and np.array_equal(tag[k], want_tag[0]), k
        seen += int(want_ev[0][:, 0].sum())
    assert seen > 0
    # the two clips outside the table: nothing event-based, their decoded classes as clip-level false positives
    ev2, tag2 = _update(rec[:, [3, 5]].contiguous(), [-1, 5], reference, C, optimal=optimal)
    assert not ev2.any() and not tag2[:, :, 0].any() and not tag2[:, :, 2].any() and tag2[0, :, 1].sum() > 0


# ---------------------------------------------------------------------------------------------------------------- class-wise decode
BAD_LABELS = (-1, 10, 2 ** 40)


def _with_bad_labels(S, L, X, C):
    """queries 2, 9 and 16 of every clip get a label that is no class, a score nothing fails and a long enough box"""
    assert C == BAD_LABELS[1]
    L, S, X = L.copy(), S.copy(), X.copy()
    for q, bad in zip((2, 9, 16), BAD_LABELS):
        L[:, q], S[:, q], X[:, q] = bad, 0.99, (1.0, 3.0)
    return S, L, X


def _rows(events_k, Bn):
    """one threshold of predictions.unpack -> per clip [(class, onset, offset, score, query)]"""
    out = [[] for _ in range(Bn)]
    for b, c, on, off, s, q in zip(events_k['clip'].tolist(), events_k['cls'].tolist(), events_k['onset'].tolist(),
                                   events_k['offset'].tolist(), events_k['score'].tolist(), events_k['query'].tolist()):
        out[b].append((c, on, off, s, q))
    return out


@pytest.mark.parametrize('del_overlap', [True, False])
def test_class_wise_decode(del_overlap):
    """a seeded [K, C] table on the (21, 10, 9, 5) case with labels -1, C and 2^40 among the queries: the records are the
    restatement's; the bad labels are dropped under both entry points; a table whose rows are constant gives the [K] entry point's
    records bit for bit"""
    Q, C = 21, 10
    _, S, L, X = _envelope_case(Q, C, 5, B, seed=100 + Q)
    S, L, X = _with_bad_labels(S, L, X, C)
    table = np.random.default_rng(5).choice(GRID9_F32, size=(9, C)).astype(np.float32)
    table[0] = GRID9_F32[0]                                           # one row lets everything through
    assert len(np.unique(table[1])) > 1
    rec = _records(S, L, X, table, C, del_overlap=del_overlap)
    assert rec.shape == (9, B, 1 + 5 * Q)
    events = _unpack(rec)
    n = 0
    for k in range(9):
        got = _rows(events[k], B)
        for b in range(B):
            want = SR.decode_strong(S[b], L[b], X[b], table[k], del_overlap=del_overlap, max_len=10.0)
            assert got[b] == want, (k, b)
            assert not {e[4] for e in got[b]} & {2, 9, 16}
            n += len(want)
    assert n > 9 * B
    uniform = _records(S, L, X, GRID9, C, del_overlap=del_overlap)
    assert not any({q for q in e['query'].tolist()} & {2, 9, 16} for e in _unpack(uniform))
    constant = np.repeat(GRID9_F32.reshape(-1, 1), C, axis=1)
    assert torch.equal(_records(S, L, X, constant, C, del_overlap=del_overlap), uniform)
    assert not torch.equal(rec, uniform)


def test_tuned_thresholds_deliver_the_promised_f1():
    """the (21, 10, 9, 5) case: the uniform sweep's counts choose one threshold per class; a K = 1 sweep on a class-wise decoder at
    that row counts, for every class c, exactly ev[index[c], c] of the uniform sweep, and its macro F1 is best_class_wise()['f1'].
    The restatement's own counts say the choice matters here (class-wise above the best uniform point, several distinct indices),
    and the device's selection is the host's."""
    from sound_event_detection_transformer_amd.utilities.operating_points import SweepEventMetrics, select_class_wise
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    Q, C = 21, 10
    labels = [f'c{i}' for i in range(C)]
    reference, S, L, X = _envelope_case(Q, C, 5, B, seed=100 + Q)
    dev = {1: tuple(torch.from_numpy(t).cuda() for t in (S, L, X))}
    idx = list(range(B))
    d = EventDecoder(labels, 10.0, thresholds=GRID9)
    sweep = SweepEventMetrics(d).set_reference(_named(reference, labels))
    decoded = d.decode(dev, None)
    sweep.update(decoded, idx)
    # the restatement, from the rows of the same records
    want_ev, want_tag = SR.counts(_unpack(decoded[0]['dev'][1]), idx, reference, C)
    host = select_class_wise(want_ev, GRID9_F32)
    f = SR.f1_table(want_ev)
    present = (want_ev[:, :, 1] > 0) | (want_tag[:, :, 0] + want_tag[:, :, 1] > 0)
    uniform = max(float(np.mean(f[k][present[k]])) for k in range(9))
    assert abs(uniform - 0.1703) < 5e-4 and abs(host['f1'] - 0.2345) < 5e-4              # the figures of this seeded case
    assert host['f1'] > uniform and len(set(host['index'].tolist())) >= 2
    assert all(f[host['index'][c], c] == f[:, c].max() for c in range(C)) and (host['index'] >= 0).all()
    # the device's counts and selection are the host's
    res = sweep.compute()[1]
    assert np.array_equal(res.ev, want_ev) and np.array_equal(res.tag, want_tag)
    got = res.best_class_wise()
    assert got['index'].tolist() == host['index'].tolist() and got['thresholds'].tolist() == host['thresholds'].tolist()
    assert got['f1'] == host['f1'] and got['class_f1'].tolist() == host['class_f1'].tolist()
    k, t, best = res.best_uniform()
    assert best == uniform and t == float(GRID9_F32[k])
    # a class-wise decoder at the chosen row delivers it
    tuned = EventDecoder(labels, 10.0, thresholds=[got['thresholds']], class_wise=True)
    assert tuned.K == 1 and tuned.threshold_values.shape == (1, C) and tuned.operating_points() == [tuple(got['thresholds'].tolist())]
    one = SweepEventMetrics(tuned).set_reference(_named(reference, labels))
    one.update(tuned.decode(dev, None), idx)
    ev1, _ = one.counts()
    for c in range(C):
        assert ev1[0, 0, c].tolist() == want_ev[got['index'][c], c].tolist(), c
    r1 = one.compute()[1]
    assert r1.thresholds == [tuple(got['thresholds'].tolist())] and r1.f1[0] == got['f1']
    assert r1.best_uniform() == (0, r1.thresholds[0], got['f1'])


def test_class_wise_decoder_grids():
    """[K] is broadcast over the classes, [K, C] is taken as it is, NaN and other shapes are refused; set_thresholds keeps K"""
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    d = EventDecoder(['a', 'b', 'c'], 10.0, thresholds=[0.2, 0.9], class_wise=True)
    assert d.K == 2 and tuple(d.thresholds.shape) == (2, 3) and d.threshold_values.dtype == np.float32
    assert d.thresholds.cpu().tolist() == [[float(np.float32(0.2))] * 3, [float(np.float32(0.9))] * 3]
    d.set_thresholds([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    assert d.thresholds.cpu().numpy().tolist() == d.threshold_values.tolist() == np.asarray([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], np.float32).tolist()
    assert d.operating_points()[1] == tuple(float(np.float32(v)) for v in (0.4, 0.5, 0.6))
    assert d.prediction_sets()[1].thresholds == d.operating_points()
    for bad, msg in (([[0.1, 0.2], [0.3, 0.4]], 'class-wise'), ([0.1, float('nan')], 'NaN'), ([0.1], 'decoder was built with')):
        with pytest.raises(ValueError, match=msg):
            d.set_thresholds(bad)
    with pytest.raises(ValueError, match='NaN'):
        EventDecoder(['a'], 10.0, thresholds=[[float('nan')]], class_wise=True)
    plain = EventDecoder(['a', 'b'], 10.0, thresholds=[0.2, 0.9])
    assert tuple(plain.thresholds.shape) == (2,) and plain.operating_points() == [float(np.float32(0.2)), float(np.float32(0.9))]


# ---------------------------------------------------------------------------------------------------------------- arguments, counters
def test_arguments_are_checked_on_the_host():
    from sound_event_detection_transformer_amd import lib, ops
    rec = torch.zeros((1, 2, 1 + 5 * 4), dtype=torch.int32).cuda()
    table, n_clips, _ = _table([[(0, 1.0, 2.0)], []])
    idx = torch.zeros(2, dtype=torch.int32).cuda()
    cnt = lambda C, K=1, nf=1: torch.zeros((nf, K, C, 3), dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError, match='reference events'):
        ops.event_sweep_update(rec, idx, table, n_clips, 65, 3, cnt(3), cnt(3), 0)
    with pytest.raises(RuntimeError, match='C=64'):
        ops.event_sweep_update(rec, idx, table, n_clips, 1, 64, cnt(64), cnt(64), 0)
    with pytest.raises(RuntimeError, match='Q=65'):
        ops.event_sweep_update(torch.zeros((1, 2, 1 + 5 * 65), dtype=torch.int32).cuda(), idx, table, n_clips, 1, 3, cnt(3), cnt(3), 0)
    with pytest.raises(RuntimeError, match='thresholds'):
        ops.event_sweep_update(torch.zeros((1025, 2, 21), dtype=torch.int32).cuda(), idx, table, n_clips, 1, 3, cnt(3, 1025), cnt(3, 1025), 0)
    with pytest.raises(RuntimeError, match='fusion 2 of 2'):
        ops.event_sweep_update(rec, idx, table, n_clips, 1, 3, cnt(3, nf=2), cnt(3, nf=2), 2)
    with pytest.raises(AssertionError):                               # records of another K than the counters
        ops.event_sweep_update(rec, idx, table, n_clips, 1, 3, cnt(3, 2), cnt(3, 2), 0)
    ev, tag = cnt(3), cnt(3)
    p = lambda t: t.data_ptr()
    # the C entry point itself: a table without its arrays
    rc = lib.load().sedt_event_sweep_update(p(rec), p(idx), p(table['present']), p(table['off']), None, None, None, n_clips, 1, 2, 4, 3, 1,
                                            1, 0, 0.2, 0.2, 1, p(ev), p(tag), None)
    assert rc != 0 and b'reference table missing' in lib.load().sedt_last_error()
    c = cnt(3, nf=4), cnt(3, nf=4)
    ops.event_sweep_update(rec[:, :0].contiguous(), idx[:0], table, n_clips, 1, 3, *c, 0)          # B == 0: nothing launched
    # a record that decode_events cannot have written - a count outside 0 .. Q - is skipped; a class outside 0 .. C - 1 is not counted
    bad = rec.clone()
    bad[0, 0, 0], bad[0, 1, 0] = 5, 1
    bad[0, 1, 1:6] = torch.tensor([7, 0, 0, 0, 0], dtype=torch.int32)
    bad[0, 1, 2:4] = torch.tensor([1.0, 2.0]).view(torch.int32)
    ops.event_sweep_update(bad, torch.tensor([1, 1], dtype=torch.int32).cuda(), table, n_clips, 1, 3, *c, 0)
    assert not c[0].cpu().numpy().any() and not c[1].cpu().numpy().any()
    # thresholds [K, C] must hold the C of the call
    with pytest.raises(AssertionError):
        ops.decode_events(torch.zeros((2, 4)).cuda(), torch.zeros((2, 4), dtype=torch.int64).cuda(), torch.zeros((2, 4, 2)).cuda(),
                          torch.zeros((1, 2)).cuda(), 3)


def test_batches_accumulate_reset_and_ignore_their_order():
    """two batches of 8 through EventDecoder.decode -> SweepEventMetrics.update: the counters hold the sum of their counts, the other
    order gives identical counters, reset() zeroes in place; set_reference makes EventMetrics' refusals"""
    from sound_event_detection_transformer_amd.utilities.operating_points import SweepEventMetrics
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    Q, C = 21, 10
    labels = [f'c{i}' for i in range(C)]
    ref_a, *a = _envelope_case(Q, C, 5, B, seed=7)
    ref_b, *b = _envelope_case(Q, C, 5, B, seed=8)
    reference = ref_a + ref_b
    reference[3] = None
    d = EventDecoder(labels, 10.0, thresholds=GRID9)
    m = SweepEventMetrics(d, optimal=False).set_reference(_named(reference, labels))
    parts = [(a, list(range(B))), (b, list(range(B, 2 * B)))]
    want = []
    for (S, L, X), idx in parts:
        decoded = d.decode({1: tuple(torch.from_numpy(t).cuda() for t in (S, L, X))}, None)
        m.update(decoded, idx)
        want.append(SR.counts(_unpack(decoded[0]['dev'][1]), idx, reference, C, optimal=False))
        ev, tag = m.counts()
        assert np.array_equal(ev[0], sum(w[0] for w in want)) and np.array_equal(tag[0], sum(w[1] for w in want))
    assert want[0][0].any() and want[1][0].any() and not np.array_equal(want[0][0], want[1][0])
    first = m.counts()
    ptrs = [t.data_ptr() for t in m.counters()]
    assert not m.reset().counts()[0].any() and not m.counts()[1].any() and [t.data_ptr() for t in m.counters()] == ptrs
    for (S, L, X), idx in parts[::-1]:
        m.update(d.decode({1: tuple(torch.from_numpy(t).cuda() for t in (S, L, X))}, None), idx)
    again = m.counts()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    res = m.compute()[1]
    assert res.class_f1.shape == (9, C) and res.f1.shape == res.clip_f1.shape == (9,) and res.f1.max() > 0 and len(res.thresholds) == 9
    fresh = SweepEventMetrics(d)
    for bad, msg in (([[(10, 0.0, 1.0)]], 'not one of'), ([[('c0', 0.0, float('inf'))]], 'non-finite'),
                     ([[('c0', 0.0, 1.0)] * 65], 'reference events')):
        with pytest.raises(ValueError, match=msg):
            fresh.set_reference(bad)
    with pytest.raises(RuntimeError, match='set_reference'):
        fresh.update(decoded, list(range(B)))
    gen = fresh.set_reference([[('c0', 0.0, 1.0)], None]).generation
    assert fresh.set_reference([[('c1', 0.0, 2.0)], None]).generation == gen and fresh.set_reference([[], None, []]).generation > gen
    with pytest.raises(ValueError, match='outside'):
        fresh.host_clip_index([3])


# ---------------------------------------------------------------------------------------------------------------- predict steps
def test_predict_steps_with_sweep():
    """the small C2 model of tests/test_psds_gpu.py (f32 mode, B 8, fusion strategies 1 and 2): the eager step, the graphed step and
    get_sedt_predictions give identical counters, equal to the restatement on the rows they fetched; a replay follows set_thresholds;
    tune_thresholds returns the host selection"""
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, get_sedt_predictions, predict_step, tune_thresholds
    from sound_event_detection_transformer_amd.utilities.operating_points import SweepEventMetrics, select_class_wise
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    model, crit, post = _c2_model()
    fusion = (1, 2)
    batches = _batches(2, B, 300)
    labels = [f'c{i}' for i in range(C2_CLASSES)]
    # a fresh seeded model scores low: the grids are quantiles of its own scores, the reference is its own events moved a little
    eager = [predict_step(model, crit, post, x, tg, fusion_strategy=fusion)[2][1] for x, tg in batches]
    all_scores = torch.cat([r[0] for r in eager]).cpu().numpy()
    grid_a = [float(np.quantile(all_scores, q)) for q in (0.5, 0.7, 0.9)]
    grid_b = [float(np.quantile(all_scores, q)) for q in (0.6, 0.8, 0.95)]
    rng = np.random.default_rng(11)
    reference = []
    for sc, lb, bx in ((t.cpu().numpy() for t in r) for r in eager):
        for b in range(B):
            dec = ER.decode_strong(sc[b], lb[b], bx[b], threshold=grid_a[1], max_len=10.0)[:int(rng.integers(0, 6))]
            reference.append(None if rng.random() < 0.1 else
                             [((c + int(rng.random() < 0.3)) % C2_CLASSES, float(on) + float(rng.choice([0.0, 0.1, 0.25])),
                               float(end) + float(rng.uniform(-0.1, 0.1))) for c, on, end, _ in dec])
    d = EventDecoder(labels, 10.0, thresholds=grid_a, fusion_strategy=fusion)
    m = SweepEventMetrics(d).set_reference(_named(reference, labels))
    x0, t0 = batches[0]
    idx0, idx1 = list(range(B)), list(range(B, 2 * B))

    def restated(events, idx):
        return {f: SR.counts(events[f], idx, reference, C2_CLASSES) for f in fusion}

    def same(idx, events):
        ev, tag = m.counts()
        want = restated(events, idx)
        for i, f in enumerate(fusion):
            assert np.array_equal(ev[i], want[f][0]) and np.array_equal(tag[i], want[f][1]), f
        return ev, tag

    # 1. sweep= without its decoder, or with another one, or without clip indices, is refused
    other = EventDecoder(labels, 10.0, thresholds=grid_a, fusion_strategy=fusion)
    for dec in (None, other):
        with pytest.raises(ValueError, match='decoder'):
            predict_step(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=dec, sweep=m, clip_idx=idx0)
        with pytest.raises(ValueError, match='decoder'):
            GraphedPredictStep(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=dec, sweep=m)
        with pytest.raises(ValueError, match='decoder'):
            get_sedt_predictions(model, crit, post, [], other if dec is None else dec, [], sweep=m)
    with pytest.raises(ValueError, match='clip_idx'):
        predict_step(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=d, sweep=m)

    # 2. the eager step: the restatement's counts of the records it fetched, with hits and misses among them
    _, events = predict_step(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=d, sweep=m, clip_idx=idx0)[3].rows()
    eager_counts = same(idx0, events)
    assert eager_counts[0][0, 0, :, 0].sum() > 0 and eager_counts[0][0, 0, :, 0].sum() < eager_counts[0][0, 0, :, 2].sum()

    # 3. building the graphed step leaves the counters as they were; a replay on the same batch gives the eager step's counters
    g = GraphedPredictStep(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=d, sweep=m)
    after = m.counts()
    assert np.array_equal(after[0], eager_counts[0]) and np.array_equal(after[1], eager_counts[1])
    m.reset()
    _, events = g(x0, t0, idx0)[3].rows()
    graphed_counts = same(idx0, events)
    assert np.array_equal(graphed_counts[0], eager_counts[0]) and np.array_equal(graphed_counts[1], eager_counts[1])
    # ... and the next replay follows set_thresholds
    d.set_thresholds(grid_b)
    m.reset()
    _, events = g(*batches[1], idx1)[3].rows()
    moved = same(idx1, events)
    assert moved[0][0, 0, :, 2].sum() > moved[0][0, 2, :, 2].sum()
    with pytest.raises(ValueError, match='clip indices'):
        g(*batches[0])

    # 4. get_sedt_predictions resets the counters and replays the same step over both batches: the counters are the sum of the
    # per-batch restatements; tune_thresholds makes the same pass and returns the host selection on those counts
    d.set_thresholds(grid_a)
    loader = [(batches[0][0], batches[0][1], idx0), (batches[1][0], batches[1][1], idx1)]
    filenames = [f'clip{i}.wav' for i in range(2 * B)]
    _, sets = get_sedt_predictions(model, crit, post, loader, d, filenames, sweep=m, step=g)
    ev, tag = m.counts()
    clip_of, class_of = {f: i for i, f in enumerate(filenames)}, {l: i for i, l in enumerate(labels)}
    grid32 = np.asarray(grid_a, np.float64).astype(np.float32)
    for i, f in enumerate(fusion):
        assert sets[f].thresholds == [float(t) for t in grid32]
        rows = [{'clip': np.array([clip_of[r[4]] for r in sets[f].to_rows(k)], np.int64),
                 'cls': np.array([class_of[r[0]] for r in sets[f].to_rows(k)], np.int64),
                 'onset': np.array([r[1] for r in sets[f].to_rows(k)]), 'offset': np.array([r[2] for r in sets[f].to_rows(k)])}
                for k in range(3)]
        want = SR.counts(rows, list(range(2 * B)), reference, C2_CLASSES)
        assert np.array_equal(ev[i], want[0]) and np.array_equal(tag[i], want[1]), f
    tuned = tune_thresholds(model, crit, post, loader, d, m, step=g)
    ev2, _ = m.counts()
    assert np.array_equal(ev2, ev) and set(tuned) == set(fusion)
    for i, f in enumerate(fusion):
        host = select_class_wise(ev[i], grid32)
        assert tuned[f]['index'].tolist() == host['index'].tolist() and tuned[f]['thresholds'].tolist() == host['thresholds'].tolist()
        assert tuned[f]['f1'] == host['f1']
    assert (tuned[1]['index'] >= 0).any() and tuned[1]['f1'] > 0
    runtime.set_compute_dtype('bf16')
