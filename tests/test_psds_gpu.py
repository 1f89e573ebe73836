"""GPU: the device PSDS counts (csrc/psds.hip through ops.psds_update, utilities/psds.PsdsMetrics and the predict steps' ``psds=``)
against the from-scratch restatement (tests/psds_ref.py) applied to the rows predictions.unpack gives for the SAME records.  Counts are
compared as integers, exactly; the scores of the host finish to 1e-12."""
import numpy as np
import pytest
import torch

import event_metrics_ref as ER
import psds_ref as R
from oracle import sedt_oracle as O
from oracle.criterion_oracle import synthetic_targets

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- helpers
def _records(S, L, X, thresholds, C, max_len=10.0, del_overlap=True):
    """one decode launch on host arrays -> the packed records on the device"""
    from sound_event_detection_transformer_amd import ops
    thr = torch.tensor(np.asarray(thresholds, dtype=np.float64), dtype=torch.float32).cuda()
    return ops.decode_events(torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).cuda(),
                             torch.from_numpy(np.ascontiguousarray(L, dtype=np.int64)).cuda(),
                             torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), thr, C, max_len=max_len,
                             del_overlap=del_overlap)[0]


def _table(reference, durations):
    """the device reference table of ops.psds_update: per clip [(class index, onset, offset)] or None -> (table, n_clips, max_ref)"""
    off, cls, on, end = [0], [], [], []
    for ev in reference:
        for c, a, b in (ev or ()):
            cls.append(c), on.append(a), end.append(b)
        off.append(len(cls))
    t = {'present': torch.tensor([ev is not None for ev in reference], dtype=torch.int32), 'off': torch.tensor(off, dtype=torch.int32),
         'cls': torch.tensor(cls or [0], dtype=torch.int32), 'on': torch.tensor(on or [0.0], dtype=torch.float64),
         'end': torch.tensor(end or [0.0], dtype=torch.float64), 'dur': torch.tensor(durations, dtype=torch.float64)}
    return {k: v.cuda() for k, v in t.items()}, len(reference), int(np.diff(off).max())


def _rows(records, clip_idx):
    """the packed records (device) -> per threshold [(clip index, class, onset, offset)] through predictions.unpack"""
    from sound_event_detection_transformer_amd.utilities.predictions import unpack
    Q = (records.shape[2] - 1) // 5
    idx = np.asarray(clip_idx)
    return [list(zip(idx[e['clip']].tolist(), e['cls'].tolist(), e['onset'].tolist(), e['offset'].tolist()))
            for e in unpack(records.cpu().numpy(), Q)]


def _update(records, clip_idx, reference, durations, C, n_fusion=2, fusion=1, **crit):
    """one psds_update launch into row ``fusion`` of fresh counters -> counts [K, C, C + 1] as numpy; the other rows stay zero"""
    from sound_event_detection_transformer_amd import ops
    table, n_clips, max_ref = _table(reference, durations)
    counts = torch.zeros((n_fusion, records.shape[0], C, C + 1), dtype=torch.int64).cuda()
    ops.psds_update(records, torch.tensor(clip_idx, dtype=torch.int32).cuda(), table, n_clips, max_ref, C, counts, fusion, **crit)
    got = counts.cpu().numpy()
    assert not np.delete(got, fusion, axis=0).any()
    return got[fusion]


def _clips(events, Q):
    """per clip [(class, onset, offset, score)] -> (scores [B, Q], labels, boxes), padded with score-0 queries"""
    S, L, X = np.zeros((len(events), Q), np.float32), np.zeros((len(events), Q), np.int64), np.zeros((len(events), Q, 2), np.float32)
    for b, ev in enumerate(events):
        for i, (c, on, off, sc) in enumerate(ev):
            S[b, i], L[b, i], X[b, i] = sc, c, (on, off)
    return S, L, X


# ---------------------------------------------------------------------------------------------------------------- hand-made clips
@pytest.mark.parametrize('del_overlap', [True, False])
def test_hand_worked_case_on_the_device(del_overlap):
    """the case of tests/test_psds_cpu.py: thresholds (0.8, 0.5) are its operating points 0 and 1; b [5, 7] and a [0, 4] sit exactly
    on the 0.5 criteria and must pass"""
    S, L, X = _clips([[(0, 1.0, 3.0, 0.9), (1, 5.0, 7.0, 0.6), (0, 6.0, 8.0, 0.6)], [(0, 0.0, 4.0, 0.6)]], 4)
    reference = [[(0, 1.0, 3.0), (1, 5.0, 9.0)], [(0, 2.0, 4.0)]]
    rec = _records(S, L, X, [0.8, 0.5], 2, del_overlap=del_overlap)
    got = _update(rec, [0, 1], reference, [10.0, 10.0], 2)
    assert got.tolist() == [[[1, 0, 0], [0, 0, 0]], [[2, 1, 1], [0, 1, 0]]]
    assert got.tolist() == R.counts(_rows(rec, [0, 1]), reference, [10.0, 10.0], ['a', 'b'])
    # just above the values the two events sit on, they fail
    assert _update(rec, [0, 1], reference, [10.0, 10.0], 2, gtc=0.5000001)[1].tolist() == [[2, 1, 1], [0, 0, 0]]
    assert _update(rec, [0, 1], reference, [10.0, 10.0], 2, dtc=0.5000001)[1].tolist() == [[1, 1, 2], [0, 1, 0]]


EDGE = {    # name: (detections [(class, onset, offset, score)], reference [(class, onset, offset)] or None, clip duration)
    # clipped to [10, 10]: counts nowhere; the zero-length reference event of class 1 makes nothing a true positive
    'zero length': ([(0, 10.5, 12.0, 0.9), (1, 4.5, 5.5, 0.9)], [(0, 9.0, 10.0), (1, 5.0, 5.0)], 10.0),
    # D_k = 4: (2, 3, 8) lies 1 / 5 = 0.2 < 0.3 inside the clip: no false positive; (1, 1, 5) lies 3 / 4 inside: one
    'short clip': ([(2, 3.0, 8.0, 0.9), (1, 1.0, 5.0, 0.9)], [(3, 0.0, 0.5)], 4.0),
    # half inside class 1's event and half inside class 2's: two cross triggers and a false positive
    'two cross triggers': ([(0, 2.0, 6.0, 0.9)], [(1, 2.0, 4.0), (2, 4.0, 6.0)], 10.0),
    'empty reference': ([(0, 1.0, 2.0, 0.9), (3, 4.0, 5.0, 0.9)], [], 10.0),
    # each detection lies inside the reference event (DTC 1); only together do they cover half of it (GTC 0.25 + 0.25)
    'two halves': ([(3, 1.0, 2.0, 0.9), (3, 2.0, 3.0, 0.9)], [(3, 1.0, 5.0)], 10.0),
    'absent': ([(0, 1.0, 2.0, 0.9), (1, 1.0, 2.0, 0.9)], None, 10.0),
}
EDGE_WANT = {   # (class row, column) cells that are 1 at threshold 0.5 (C = 4, column 4 = world); everything else 0
    'zero length': {(1, 4)}, 'short clip': {(1, 4)}, 'two cross triggers': {(0, 1), (0, 2), (0, 4)}, 'empty reference': {(0, 4), (3, 4)},
    'absent': set(), 'two halves': {(3, 3)},
}


@pytest.mark.parametrize('del_overlap', [True, False])
def test_edge_cases_against_the_restatement(del_overlap):
    """the clips of EDGE in one batch of 9 (Q = 8, C = 4, K = 2), the last three entries outside the table: the clip given as None,
    index -1 and an index >= n_clips; then the three alone: they add nothing"""
    C, labels, names = 4, ['a', 'b', 'c', 'd'], list(EDGE)
    dets = [EDGE[n][0] for n in names] + [EDGE['two cross triggers'][0]] * 2
    reference, durations = [EDGE[n][1] for n in names], [EDGE[n][2] for n in names]
    idx = list(range(len(names))) + [-1, 99]
    assert reference[idx[-3]] is None
    S, L, X = _clips(dets, 8)
    rec = _records(S, L, X, [0.5, 0.95], C, del_overlap=del_overlap)
    got = _update(rec, idx, reference, durations, C)
    rows = _rows(rec, idx)
    assert len(rows[0]) == sum(len(d) for d in dets) and len(rows[1]) == 0          # every detection decoded (one of zero length)
    assert got.tolist() == R.counts(rows, reference, durations, labels)
    assert not got[1].any()
    # what the cases are there for, spelled out (pins the restatement; the kernel is pinned to it above)
    total = np.zeros((C, C + 1), np.int64)
    for i, n in enumerate(names):
        one = np.array(R.counts([[r for r in rows[0] if r[0] == i]], reference, durations, labels)[0])
        assert {tuple(c) for c in np.argwhere(one == 1).tolist()} == EDGE_WANT[n] and one.sum() == len(EDGE_WANT[n]), (n, one)
        total += one
    assert np.array_equal(got[0], total)
    assert not _update(rec[:, -3:].contiguous(), idx[-3:], reference, durations, C).any()


# ---------------------------------------------------------------------------------------------------------------- envelope edges
GRID9 = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


def _envelope_case(Q, C, max_ref, B, seed):
    """seeded clips: clip 0 holds max_ref reference events and Q queries that all pass the lowest threshold; the queries are a mix
    of reference events jittered (true positives), reference intervals under another class (cross triggers) and free intervals
    (false positives); every duration is >= 0.3 s"""
    rng = np.random.default_rng(seed)
    reference, S, L, X = [], np.zeros((B, Q), np.float32), np.zeros((B, Q), np.int64), np.zeros((B, Q, 2), np.float32)
    for b in range(B):
        n = max_ref if b == 0 else int(rng.integers(0, min(max_ref, 6) + 1))
        on = np.round(rng.uniform(0, 9.0, n) / 0.05) * 0.05
        ev = [(int(rng.integers(0, C)), float(a), float(a + rng.choice([0.3, 0.5, 1.0, 2.0, 3.0]))) for a in on]
        reference.append(ev)
        for q in range(Q):
            mode = rng.random()
            if ev and mode < 0.7:
                c, a, e = ev[int(rng.integers(0, n))]
                a, e = a + float(rng.choice([0.0, 0.1, -0.1, 0.4])), e + float(rng.choice([0.0, 0.2, -0.1]))
                if mode >= 0.4 and C > 1:
                    c = (c + 1 + int(rng.integers(0, C - 1))) % C
            else:
                c, a = int(rng.integers(0, C)), float(rng.uniform(-0.3, 9.5))
                e = a + float(rng.choice([0.3, 0.5, 1.5, 4.0]))
            S[b, q], L[b, q], X[b, q] = rng.uniform(0.15 if b == 0 else 0.02, 1.0), c, (a, max(e, a + 0.3))
    return reference, S, L, X


@pytest.mark.parametrize('Q,C,K,max_ref', [(1, 1, 1, 1), (21, 10, 9, 5), (64, 63, 9, 64)])
def test_envelope_edges(Q, C, K, max_ref):
    """B = 8 at the edges of the kernel's envelope.  Q = 64 decodes with del_overlap off and clip 0 keeps all 64 queries at the lowest
    threshold; max_ref = 64 has 64 reference events in clip 0.  So that the comparison is not vacuous, the restatement's own counts
    hold a non-zero diagonal entry, a non-zero off-diagonal entry (where there is one: not at C = 1) and a non-zero world entry at
    no fewer than half of the thresholds."""
    B = 8
    reference, S, L, X = _envelope_case(Q, C, max_ref, B, seed=100 + Q)
    assert max(len(e) for e in reference) == max_ref == len(reference[0])
    thresholds = GRID9 if K == 9 else [0.5]
    rec = _records(S, L, X, thresholds, C, del_overlap=Q != 64)
    assert rec.shape == (K, B, 1 + 5 * Q)
    if Q == 64:
        assert int(rec[0, 0, 0]) == 64
    idx = list(range(B))
    rows = _rows(rec, idx)
    want = np.array(R.counts(rows, reference, [10.0] * B, [f'c{i}' for i in range(C)]))
    diag = np.eye(C, C + 1, dtype=bool)
    world = np.zeros((C, C + 1), bool)
    world[:, C] = True
    kinds = {'diagonal': diag, 'world': world}
    if C > 1:
        kinds['off-diagonal'] = ~diag & ~world
    for name, cells in kinds.items():
        assert 2 * sum(int(want[k][cells].any()) for k in range(K)) >= K, name
    got = _update(rec, idx, reference, [10.0] * B, C)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


def test_arguments_are_checked_on_the_host():
    from sound_event_detection_transformer_amd import ops
    rec = torch.zeros((1, 2, 1 + 5 * 4), dtype=torch.int32).cuda()
    table, n_clips, _ = _table([[(0, 1.0, 2.0)], []], [10.0, 10.0])
    idx = torch.zeros(2, dtype=torch.int32).cuda()
    counts = lambda C, K=1, nf=1: torch.zeros((nf, K, C, C + 1), dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError, match='reference events'):
        ops.psds_update(rec, idx, table, n_clips, 65, 3, counts(3), 0)
    with pytest.raises(RuntimeError, match='C=64'):
        ops.psds_update(rec, idx, table, n_clips, 1, 64, counts(64), 0)
    with pytest.raises(RuntimeError, match='Q=65'):
        ops.psds_update(torch.zeros((1, 2, 1 + 5 * 65), dtype=torch.int32).cuda(), idx, table, n_clips, 1, 3, counts(3), 0)
    with pytest.raises(RuntimeError, match='thresholds'):
        ops.psds_update(torch.zeros((1025, 2, 21), dtype=torch.int32).cuda(), idx, table, n_clips, 1, 3, counts(3, 1025), 0)
    with pytest.raises(RuntimeError, match='NaN'):
        ops.psds_update(rec, idx, table, n_clips, 1, 3, counts(3), 0, dtc=float('nan'))
    c = counts(3, nf=4)
    ops.psds_update(rec[:, :0].contiguous(), idx[:0], table, n_clips, 1, 3, c, 0)          # B == 0: nothing launched
    # a record that decode_events cannot have written - a count outside 0 .. Q, a class outside 0 .. C - 1 - is skipped
    bad = rec.clone()
    bad[0, 0, 0], bad[0, 1, 0] = 5, 1
    bad[0, 1, 1:6] = torch.tensor([7, 0, 0, 0, 0], dtype=torch.int32)
    bad[0, 1, 2:4] = torch.tensor([1.0, 2.0]).view(torch.int32)
    ops.psds_update(bad, idx, table, n_clips, 1, 3, c, 0)
    assert not c.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------- PsdsMetrics
def test_batches_accumulate_and_reset():
    """two batches of 8 through EventDecoder.decode -> PsdsMetrics.update: the counters hold the sum of their counts; reset() zeroes"""
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
    Q, C, B = 21, 10, 8
    labels = [f'c{i}' for i in range(C)]
    ref_a, *a = _envelope_case(Q, C, 5, B, seed=7)
    ref_b, *b = _envelope_case(Q, C, 5, B, seed=8)
    reference = [[(labels[c], on, off) for c, on, off in ev] for ev in ref_a + ref_b]
    reference[3] = None
    durations = [10.0] * (2 * B)
    d = EventDecoder(labels, 10.0, thresholds=GRID9)
    m = PsdsMetrics(d).set_reference(reference)
    assert m.n_gt.tolist() == R.constants(reference, durations, labels)[0] and m.total_dur == 10.0 * (2 * B - 1)
    want = []
    for (S, L, X), idx in ((a, list(range(B))), (b, list(range(B, 2 * B)))):
        dev = tuple(torch.from_numpy(t).cuda() for t in (S, L, X))
        decoded = d.decode({1: dev}, None)
        m.update(decoded, idx)
        want.append(np.array(R.counts(_rows(decoded[0]['dev'][1], idx), reference, durations, labels)))
        assert np.array_equal(m.counts_host()[0], sum(want))
    assert want[0].any() and want[1].any() and not np.array_equal(want[0], want[1])
    res = m.compute()[1]
    n_gt, gt_dur, total = R.constants(reference, durations, labels)
    for s, v in res['psds'].items():
        assert abs(v - R.score(sum(want).tolist(), n_gt, gt_dur, total, *s)) <= 1e-12 and 0.0 <= v <= 1.0
    assert res['psds'][(0, 0, 100)] > 0.0
    assert res['tpr'].shape == (9, C) and res['ctr'].shape == (9, C, C) and len(res['thresholds']) == 9
    x, y = res.curve((0, 0, 100))
    assert x.shape == y.shape and (np.diff(x) > 0).all() and (np.diff(y) >= 0).all()
    assert not m.reset().counts_host().any()


def test_set_reference_refusals():
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
    m = PsdsMetrics(EventDecoder(['a', 'b'], 10.0))
    for bad, msg in (([[(2, 0.0, 1.0)]], 'not one of'), ([[('a', 0.0, float('inf'))]], 'non-finite'),
                     ([[('a', 0.0, 1.0)] * 65], 'reference events')):
        with pytest.raises(ValueError, match=msg):
            m.set_reference(bad)
    for dur in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='duration'):
            m.set_reference([[('a', 0.0, 1.0)]], [dur])
    with pytest.raises(ValueError, match='durations'):
        m.set_reference([[('a', 0.0, 1.0)]], [10.0, 10.0])
    gen = m.set_reference([[('a', 0.0, 1.0)], None]).generation
    assert m.set_reference([[('b', 0.0, 2.0)], None]).generation == gen                  # same shape: a captured step stays valid
    assert m.set_reference([[('b', 0.0, 2.0)], None, []]).generation > gen
    with pytest.raises(RuntimeError, match='set_reference'):
        PsdsMetrics(EventDecoder(['a'], 10.0)).compute()


# ---------------------------------------------------------------------------------------------------------------- predict steps
C2_CLASSES = 10


def _c2_model():
    from sound_event_detection_transformer_amd import runtime, sedt
    runtime.set_compute_dtype('f32')
    runtime.manual_seed(5)
    model, crit, post = sedt.build_model(sedt.default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), 2020))
    model.cuda().eval()
    crit.cuda()
    return model, crit, post['bbox']


def _batches(n, B, seed):
    out = []
    for s in range(n):
        x = torch.randn(B, 1, 500, 64, generator=torch.Generator().manual_seed(seed + s)).cuda()
        tg = synthetic_targets(B, seed + 100 + s, C2_CLASSES)
        for t in tg:
            t['orig_size'] = torch.tensor(10.0)
        out.append((x, [{k: v.cuda() for k, v in t.items()} for t in tg]))
    return out


def test_predict_steps_with_psds():
    """the smallest model of the decode tests (C2: enc_layers 3, Q 10, audio tags; f32 mode, B 8, fusion strategies 1 and 2): the
    graphed step replayed on two different batches with set_thresholds in between, then get_sedt_predictions over three batches, the
    last one short.  See the comments below for what is checked."""
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, predict_step, get_sedt_predictions
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
    model, crit, post = _c2_model()
    B, fusion = 8, (1, 2)
    batches = _batches(3, B, 300)
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
                             [(labels[(c + int(rng.random() < 0.3)) % C2_CLASSES], float(on) + float(rng.choice([0.0, 0.1, 0.25])),
                               float(end) + float(rng.uniform(-0.3, 0.3))) for c, on, end, _ in dec])
    durations = [10.0] * len(reference)
    d = EventDecoder(labels, 10.0, thresholds=grid_a, fusion_strategy=fusion)
    m = PsdsMetrics(d).set_reference(reference)

    # 1. psds= without its decoder, or with another one, is refused
    x0, t0 = batches[0]
    other = EventDecoder(labels, 10.0, thresholds=grid_a, fusion_strategy=fusion)
    for dec in (None, other):
        with pytest.raises(ValueError, match='decoder'):
            predict_step(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=dec, psds=m, clip_idx=list(range(B)))
        with pytest.raises(ValueError, match='decoder'):
            GraphedPredictStep(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=dec, psds=m)
        with pytest.raises(ValueError, match='decoder'):
            get_sedt_predictions(model, crit, post, [], other if dec is None else dec, [], psds=m)
    with pytest.raises(ValueError, match='clip_idx'):
        predict_step(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=d, psds=m)

    # 2. building the step leaves the counters as they were; every replay adds the restatement's counts of the records it fetched
    g = GraphedPredictStep(model, crit, post, x0, t0, fusion_strategy=fusion, decoder=d, psds=m)
    assert not m.counts_host().any()
    graph = g.graph
    for n, grid in ((0, grid_a), (1, grid_b)):
        d.set_thresholds(grid)                                          # between the replays: the graph follows the device vector
        m.reset()
        idx = list(range(n * B, (n + 1) * B))
        _, events = g(*batches[n], idx)[3].rows()
        got = m.counts_host()
        for i, f in enumerate(fusion):
            rows = [list(zip(np.asarray(idx)[e['clip']].tolist(), e['cls'].tolist(), e['onset'].tolist(), e['offset'].tolist()))
                    for e in events[f]]
            want = np.array(R.counts(rows, reference, durations, labels))
            assert np.array_equal(got[i], want), (n, f)
            if f == 1:                                                  # the grids and the reference come from strategy 1's outputs
                assert want[0].trace() > 0 and want[0][:, C2_CLASSES].sum() > 0, (n, want[0])     # hits and false positives
    assert g.graph is graph
    with pytest.raises(ValueError, match='clip indices'):
        g(*batches[0])

    # 3. get_sedt_predictions resets the counters, replays the same step on two batches and sends the short third one through the
    # eager predict_step: the counters equal the restatement applied to the returned PredictionSets, the scores its finish
    d.set_thresholds(grid_a)
    x3, t3 = batches[2]
    loader = [(x, tg, list(range(n * B, (n + 1) * B))) for n, (x, tg) in enumerate(batches[:2])] + [(x3[:5], t3[:5], [20, 17, 18, 19, 16])]
    filenames = [f'clip{i}.wav' for i in range(3 * B)]
    _, sets = get_sedt_predictions(model, crit, post, loader, d, filenames, psds=m, step=g)
    got = m.counts_host()
    res = m.compute()
    n_gt, gt_dur, total = R.constants(reference, durations, labels)
    clip_of, class_of = {f: i for i, f in enumerate(filenames)}, {l: i for i, l in enumerate(labels)}
    for i, f in enumerate(fusion):
        rows = [[(clip_of[name], class_of[lab], on, off) for lab, on, off, _, name in sets[f].to_rows(k)] for k in range(3)]
        assert {r[0] for r in rows[0]} >= {16, 20}                      # the short batch's clips are there
        want = R.counts(rows, reference, durations, labels)
        assert np.array_equal(got[i], np.array(want)), f
        assert set(res[f]['psds']) == {(0, 0, 100), (1, 0, 100), (0, 1, 100)}
        for s, v in res[f]['psds'].items():
            assert abs(v - R.score(want, n_gt, gt_dur, total, *s)) <= 1e-12, (f, s)
            assert 0.0 <= v <= 1.0
    runtime.set_compute_dtype('bf16')
