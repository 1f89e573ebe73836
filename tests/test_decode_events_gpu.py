"""GPU: the device decode (csrc/decode.hip through ops.decode_events, utilities/predictions.EventDecoder and the predict steps'
``decoder=``) against the reference's own decode_strong (fixtures G18 and G23: bit for bit), against the CPU restatement
(tests/event_metrics_ref.py) on hand-made edge cases and on a graphed C2 model's own outputs, and against the metrics kernel's
counters (csrc/metrics.hip repeats the same keep / sort / overlap pass).  Events are compared exactly: counts, classes and order as
integers, onsets / offsets / scores as float32 values."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import event_metrics_ref as R
from oracle import sedt_oracle as O
from oracle.criterion_oracle import synthetic_targets

pytestmark = pytest.mark.gpu

INF = float('inf')


def _decode(S, L, X, thresholds, C, max_len, del_overlap, min_duration=0.2):
    """one launch on host arrays -> (packed, count, cls, times, score, query) as numpy"""
    from sound_event_detection_transformer_amd import ops
    thr = torch.tensor(np.asarray(thresholds, dtype=np.float64), dtype=torch.float32).cuda()
    out = ops.decode_events(torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(L, dtype=np.int64)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(), thr, C, min_duration=min_duration,
                            max_len=max_len, del_overlap=del_overlap)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_records(got, k, S, L, X, want_rows, clipped):
    """threshold k of one launch against want_rows [(clip, class, onset, offset, score)] in output order: the whole record of every
    clip - count, live slots, filler - and the query column against the inputs"""
    packed, count, cls, times, score, query = got
    B, Q = S.shape
    want = [[] for _ in range(B)]
    for b, c, on, off, sc in want_rows:
        want[int(b)].append((int(c), np.float32(on), np.float32(off), np.float32(sc)))
    for b in range(B):
        n = len(want[b])
        assert count[k, b] == n, (k, b, count[k, b], n)
        assert cls[k, b, :n].tolist() == [e[0] for e in want[b]], (k, b)
        for j, col in ((1, times[k, b, :n, 0]), (2, times[k, b, :n, 1]), (3, score[k, b, :n])):
            w = np.array([e[j] for e in want[b]], dtype=np.float32)
            if clipped:
                assert np.array_equal(col, w), (k, b, j, col, w)
            else:
                assert np.array_equal(col.view(np.int32), w.view(np.int32)), (k, b, j, col, w)        # bit for bit
        q = query[k, b, :n]
        assert len(set(q.tolist())) == n and (q >= 0).all() and (q < Q).all()
        assert np.array_equal(L[b][q], cls[k, b, :n]) and np.array_equal(S[b][q].view(np.int32), score[k, b, :n].view(np.int32))
        if not clipped:
            assert np.array_equal(X[b][q].view(np.int32), times[k, b, :n].view(np.int32))
        # slots at or past n: {-1, 0, 0, 0, -1}
        assert (cls[k, b, n:] == -1).all() and (query[k, b, n:] == -1).all()
        assert not packed[k, b, 1:].reshape(Q, 5)[n:, 1:4].any()


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize('Q', [10, 20])
@pytest.mark.parametrize('del_overlap', [1, 0])
def test_g18_on_the_device(Q, del_overlap):
    """the reference's decode_strong at threshold 0.5 on 200 clips per query count: every clip, no clip (max_len = inf)"""
    g = np.load(os.path.join(GOLDEN, 'g18_decode_strong.npz'))
    S, L, X, want = g[f'q{Q}_scores'], g[f'q{Q}_labels'], g[f'q{Q}_boxes'], g[f'q{Q}_del{del_overlap}']
    got = _decode(S, L, X, [0.5], 10, INF, bool(del_overlap))
    assert got[0].shape == (1, len(S), 1 + 5 * Q) and got[0].dtype == np.int32
    assert int(got[1].sum()) == len(want) > 100
    _check_records(got, 0, S, L, X, want, clipped=False)


@pytest.mark.parametrize('Q,C', [(1, 1), (21, 10), (64, 63)])
@pytest.mark.parametrize('del_overlap', [1, 0])
def test_g23_on_the_device(Q, C, del_overlap):
    """the reference's decode_strong at thresholds 0.1 .. 0.9 in ONE launch, on scores on / next to float32(threshold), at the
    envelope's edges (Q 1 and 64, C 1 and 63): every clip and threshold, no clip (max_len = inf)"""
    g = np.load(os.path.join(GOLDEN, 'g23_decode_sweep.npz'))
    S, L, X = g[f'q{Q}c{C}_scores'], g[f'q{Q}c{C}_labels'].astype(np.int64), g[f'q{Q}c{C}_boxes']
    thr = g['thresholds']
    got = _decode(S, L, X, thr, C, INF, bool(del_overlap))
    assert got[0].shape == (len(thr), len(S), 1 + 5 * Q)
    for k in range(len(thr)):
        want = g[f'q{Q}c{C}_del{del_overlap}_t{k}']
        assert int(got[1][k].sum()) == len(want)
        _check_records(got, k, S, L, X, want, clipped=False)


# ---------------------------------------------------------------------------------------------------------------- edge cases
def _clip(events, Q):
    """[(class, onset, offset, score)] -> one clip's arrays, padded to Q with score-0 queries"""
    s, l, b = np.zeros(Q, np.float32), np.zeros(Q, np.int64), np.zeros((Q, 2), np.float32)
    for i, (c, on, off, sc) in enumerate(events):
        s[i], l[i], b[i] = sc, c, (on, off)
    return s, l, b


def _restated(S, L, X, thresholds, C, del_overlap, max_len=10.0):
    """per threshold the rows the restatement gives (labels outside 0 .. C - 1 dropped, as the kernels drop them: such a label is a
    group of its own in decode_strong, so dropping it before or after is the same)"""
    return [[(b, c, on, off, sc) for b in range(len(S))
             for c, on, off, sc in R.decode_strong(S[b], L[b], X[b], threshold=float(t), del_overlap=del_overlap, max_len=max_len)
             if 0 <= c < C] for t in thresholds]


def _edge_clips(Q=64, C=10):
    f02 = np.float32(0.2)
    chain = [(3, 0.1 * i, 0.1 * i + 0.45, 0.55 + 0.4 * ((i * 37) % 64) / 64) for i in range(64)]      # 64 kept events of one class
    clips = {
        'longest chain': chain,
        'rising chain': [(0, 0.1 * i, 0.1 * i + 0.5, 0.5 + i / 256) for i in range(64)],              # every event removes the last
        'nothing kept': [(1, 1.0, 2.0, 0.1), (2, 1.0, 1.1, 0.9), (3, 5.0, 4.0, 0.9)],
        # queries 0 and 2 tie: 0 first -> 2 falls to it and 3 after it ({0}); 2 first would leave {2, 3}
        'onset tie': [(2, 1.0, 3.0, 0.6), (4, 0.0, 0.5, 0.9), (2, 1.0, 1.2, 0.6), (2, 2.0, 2.5, 0.5)],
        # class 5's first kept query (0) falls to query 2; class 5 still comes before class 1
        'first kept deleted': [(5, 1.0, 3.0, 0.6), (1, 0.0, 1.0, 0.9), (5, 2.0, 4.0, 0.9), (1, 5.0, 6.0, 0.7), (5, 6.0, 7.0, 0.55)],
        'minimum length': [(0, 0.0, f02, 0.9), (1, 0.0, np.nextafter(f02, np.float32(0)), 0.9), (2, 1.0, 1.2, 0.9), (3, 1.0, 1.19, 0.9)],
        'outside the clip': [(0, -1.0, 0.5, 0.9), (1, 9.5, 11.0, 0.9), (2, 10.5, 12.0, 0.9), (3, -2.0, -1.0, 0.9), (4, -1.0, 12.0, 0.6)],
        'label out of range': [(C, 1.0, 2.0, 0.9), (-1, 1.0, 2.0, 0.9), (C - 1, 1.5, 2.5, 0.8), (2 ** 40, 3.0, 4.0, 0.9), (0, 3.0, 4.0, 0.9)],
        'nan score': [(0, 1.0, 2.0, float('nan')), (0, 1.5, 2.5, 0.7), (1, float('nan'), 2.0, 0.9), (1, 1.0, float('nan'), 0.9)],
    }
    names = list(clips)
    S, L, X = (np.stack(a) for a in zip(*[_clip(clips[n], Q) for n in names]))
    return names, S, L, X


@pytest.mark.parametrize('del_overlap', [True, False])
def test_edge_cases_against_the_restatement(del_overlap):
    """hand-made clips (see _edge_clips) at Q = 64, decoded with max_len = 10 at K = 1 and at K = 64 thresholds in one launch each"""
    C = 10
    names, S, L, X = _edge_clips(64, C)
    grid = np.concatenate([np.linspace(0.0, 1.0, 59), [0.5, 0.55, 0.6, 0.7, 0.9]])
    assert len(grid) == 64
    for thr in ([0.5], grid):
        got = _decode(S, L, X, thr, C, 10.0, del_overlap)
        want = _restated(S, L, X, thr, C, del_overlap)
        for k in range(len(thr)):
            _check_records(got, k, S, L, X, want[k], clipped=True)
    at = lambda name, k=0: [e[1:] for e in want[k] if e[0] == names.index(name)]
    want = _restated(S, L, X, [0.5], C, del_overlap)
    # what the cases are there for, spelled out at threshold 0.5 (the restatement is pinned by G18 / G23; these pin the cases)
    assert len(at('nothing kept')) == 0 and len(at('nan score')) == 1
    assert [e[0] for e in at('label out of range')] == [C - 1, 0]
    assert [e[0] for e in at('minimum length')] == [0, 2]
    assert [(e[1], e[2]) for e in at('outside the clip')][:4] == [(0.0, 0.5), (9.5, 10.0), (10.0, 10.0), (0.0, 0.0)]   # zero length stays
    if del_overlap:
        assert len(at('longest chain')) < 64 and len(at('rising chain')) == 1
        assert [e[0] for e in at('first kept deleted')] == [5, 5, 1, 1] and at('first kept deleted')[0][1] == 2.0
        assert [(e[0], e[2]) for e in at('onset tie')] == [(2, 3.0), (4, 0.5)]          # the lower query of the tie stands first
    else:
        assert len(at('longest chain')) == 64 and len(at('first kept deleted')) == 5


@pytest.mark.parametrize('del_overlap', [True, False])
def test_one_query_and_three_clips(del_overlap):
    """Q = 1 (one live lane), and B = 3 at K = 1 and K = 64"""
    S = np.array([[0.5], [0.4], [0.9]], np.float32)
    L = np.array([[0], [0], [2]], np.int64)
    X = np.array([[[1.0, 2.0]], [[1.0, 2.0]], [[-0.5, 0.1]]], np.float32)
    for thr in ([0.5], np.linspace(0.0, 1.0, 64)):
        got = _decode(S, L, X, thr, 3, 10.0, del_overlap)
        want = _restated(S, L, X, thr, 3, del_overlap)
        for k in range(len(thr)):
            _check_records(got, k, S, L, X, want[k], clipped=True)
    assert got[1][0].tolist() == [1, 1, 1] and got[1][63].tolist() == [0, 0, 0]


def test_arguments_are_checked_on_the_host():
    from sound_event_detection_transformer_amd import ops
    s, l, x = torch.zeros(2, 4).cuda(), torch.zeros(2, 4, dtype=torch.int64).cuda(), torch.zeros(2, 4, 2).cuda()
    thr = torch.tensor([0.5]).cuda()
    for bad in (dict(max_len=0.1), dict(max_len=-1.0), dict(max_len=float('nan')), dict(n_classes=64), dict(n_classes=0)):
        kw = dict(n_classes=3, max_len=10.0)
        kw.update(bad)
        with pytest.raises(RuntimeError, match='decode_events'):
            ops.decode_events(s, l, x, thr, kw['n_classes'], max_len=kw['max_len'])
    with pytest.raises(RuntimeError, match='thresholds'):
        ops.decode_events(s, l, x, torch.zeros(ops.DECODE_MAX_THRESHOLDS + 1).cuda(), 3)
    with pytest.raises(RuntimeError, match='Q=65'):
        ops.decode_events(torch.zeros(1, 65).cuda(), torch.zeros(1, 65, dtype=torch.int64).cuda(), torch.zeros(1, 65, 2).cuda(), thr, 3)


# ---------------------------------------------------------------------------------------------------------------- the two kernels
def test_decoded_events_score_like_the_metrics_kernel():
    """random batches of B = 8, Q = 20 and a reference set: the events this kernel writes at threshold t, scored on the host
    (tests/event_metrics_ref), equal the counters EventMetrics(threshold=t) accumulates from the same tensors - the two kernels'
    keep / sort / overlap passes agree, and so do their clips to [0, max_len]"""
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    C, B, Q, N = 10, 8, 20, 24
    rng = np.random.default_rng(23)
    refs = []
    for k in range(N):
        u = rng.random()
        refs.append(None if u < 0.1 else [(int(rng.integers(0, C)), on, on + float(rng.choice([0.2, 0.5, 1.0, 3.0])))
                                          for on in (np.round(rng.uniform(0, 9.5, 0 if u < 0.2 else int(rng.integers(1, 8))) / 0.05) * 0.05).tolist()])
    thresholds = (0.3, 0.5, 0.7)
    batches = []
    for s in range(0, N, B):
        S = rng.choice(np.array([0.3, 0.5, 0.5, 0.7, 0.9], np.float32), (B, Q)).astype(np.float32)
        S = np.where(rng.random((B, Q)) < 0.5, S, rng.uniform(0.2, 1.0, (B, Q))).astype(np.float32)
        L = rng.integers(0, 4, (B, Q))
        on = np.round(rng.uniform(-0.5, 9.8, (B, Q)) / 0.05) * 0.05
        X = np.stack([on, on + rng.choice([0.1, 0.2, 0.2, 0.5, 1.5, 3.0], (B, Q))], -1).astype(np.float32)
        for b in range(B):                                   # a share of the queries on a reference event of the clip: hits
            for i, (c, r_on, r_end) in enumerate((refs[s + b] or [])[:Q // 2]):
                L[b, i], X[b, i] = c, (r_on + rng.choice([0.0, 0.2, -0.2, 0.1]), r_end + rng.choice([0.0, 0.2, -0.3]))
        batches.append((list(range(s, s + B)), S, L.astype(np.int64), X, rng.integers(0, 2, (B, C))))
    for del_overlap in (True, False):
        ms = [EventMetrics([f'c{i}' for i in range(C)], 10.0, threshold=t, del_overlap=del_overlap).set_reference(
            [None if e is None else [(f'c{c}', on, end) for c, on, end in e] for e in refs]) for t in thresholds]
        ev = np.zeros((len(thresholds), C, 3), np.int64)
        tag = np.zeros((len(thresholds), C, 3), np.int64)
        for idx, S, L, X, tags in batches:
            dev = (torch.from_numpy(S).cuda(), torch.from_numpy(L).cuda(), torch.from_numpy(X).cuda())
            for m in ms:
                m.update({1: dev}, torch.from_numpy(tags).cuda(), idx)
            _, count, cls, times, _, _ = _decode(S, L, X, thresholds, C, 10.0, del_overlap)
            for k in range(len(thresholds)):
                for b, clip in enumerate(idx):
                    n = count[k, b]
                    ests = [(int(cls[k, b, j]), float(times[k, b, j, 0]), float(times[k, b, j, 1])) for j in range(n)]
                    if refs[clip] is not None:
                        ev[k] += R.clip_event_counts(refs[clip], ests, C)
                    tag[k] += R.clip_tag_counts({e[0] for e in (refs[clip] or [])}, {e[0] for e in ests}, C)
        for k, m in enumerate(ms):
            got_ev, got_tag = m.counts()
            assert got_ev[0, :, 0].sum() > 0 and got_ev[0, :, 2].sum() > got_ev[0, :, 0].sum()          # there were hits and misses
            assert np.array_equal(got_ev[0], ev[k]), (del_overlap, k, np.argwhere(got_ev[0] != ev[k])[:10])
            assert np.array_equal(got_tag[0], tag[k]), (del_overlap, k)


# ---------------------------------------------------------------------------------------------------------------- graphed step
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


def _rows_of(events):
    """unpack()'s per-threshold dicts -> [[(clip, class, onset, offset, score)]]"""
    return [list(zip(e['clip'].tolist(), e['cls'].tolist(), e['onset'].tolist(), e['offset'].tolist(), e['score'].tolist())) for e in events]


def _want_rows(res, thresholds):
    S, L, X = (t.cpu().numpy() for t in res)
    return _restated(S, L, X, thresholds, C2_CLASSES, True)


def test_graphed_predict_step_with_decoder():
    """C2 (enc_layers 3, Q 10, audio tags), f32 mode, B 8, fusion strategies 1 and 2, two batches plus a short one.  See the
    comments below for what is checked."""
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, predict_step, evaluate_events, get_sedt_predictions
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    model, crit, post = _c2_model()
    B, fusion = 8, (1, 2)
    batches = _batches(3, B, 300)
    labels = [f'c{i}' for i in range(C2_CLASSES)]
    # a fresh seeded model scores low: the grids are quantiles of its own scores
    eager = [predict_step(model, crit, post, x, tg, fusion_strategy=fusion)[2][1] for x, tg in batches]
    all_scores = torch.cat([r[0] for r in eager]).cpu().numpy()
    grid_a = [float(np.quantile(all_scores, q)) for q in (0.5, 0.7, 0.9)]
    grid_b = [float(np.quantile(all_scores, q)) for q in (0.6, 0.8, 0.95)]
    thr = grid_a[1]
    rng = np.random.default_rng(11)
    refs = []
    for sc, lb, bx in ((t.cpu().numpy() for t in r) for r in eager):
        for b in range(B):
            dec = R.decode_strong(sc[b], lb[b], bx[b], threshold=thr, max_len=10.0)[:int(rng.integers(0, 6))]
            refs.append(None if rng.random() < 0.1 else
                        [(c, on + float(rng.choice([0.0, 0.1, 0.25])), end + float(rng.uniform(-0.3, 0.3))) for c, on, end, _ in dec])
    m = EventMetrics(labels, 10.0, threshold=thr, fusion_strategy=fusion).set_reference(refs)
    d = EventDecoder(labels, 10.0, thresholds=grid_a, fusion_strategy=fusion)
    plain = GraphedPredictStep(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=fusion)
    g = GraphedPredictStep(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=fusion, metrics=m, decoder=d)

    def one_pass(grid, compare_plain):
        rows = []
        for n, (x, tg) in enumerate(batches):
            idx = list(range(n * B, (n + 1) * B))
            gl, gt, gr, fetched = g(x, tg, idx)
            tags, events = fetched.rows()
            if compare_plain:
                # 1. losses, tags and PostProcess tensors are bit-identical to a step built without a decoder
                gl, gt, gr = {k: v.clone() for k, v in gl.items()}, gt.clone(), {k: tuple(t.clone() for t in v) for k, v in gr.items()}
                pl, pt, pr = plain(x, tg)
                torch.cuda.synchronize()
                assert torch.equal(gt, pt) and all(torch.equal(gl[k], pl[k]) for k in pl)
                assert all(torch.equal(a, b) for f in fusion for a, b in zip(gr[f], pr[f]))
            # 2. the rows equal the restatement fed with the step's own PostProcess outputs, at every threshold of the grid
            assert np.array_equal(tags, gt.cpu().numpy()) and set(events) == set(fusion)
            for f in fusion:
                got = _rows_of(events[f])
                assert got == [[tuple(r) for r in w] for w in _want_rows(gr[f], grid)], (n, f)
            rows.append({f: _rows_of(events[f]) for f in fusion})
        return rows

    first = one_pass(grid_a, True)
    assert sum(len(r[1][0]) for r in first) > sum(len(r[1][2]) for r in first) >= 0 and sum(len(r[1][0]) for r in first) > 10
    # 3. after set_thresholds the next replay follows the new grid: no rebuild
    graph = g.graph
    d.set_thresholds(grid_b)
    other = one_pass(grid_b, False)
    assert other != first and g.graph is graph
    # 4. a second pass at the first grid returns the same rows (no slot shows an earlier batch)
    d.set_thresholds(grid_a)
    assert one_pass(grid_a, False) == first

    # 5. get_sedt_predictions: two full batches through a new graph, then the third as a short batch through the eager predict_step
    x3, t3 = batches[2]
    loader = [(x, tg, list(range(n * B, (n + 1) * B))) for n, (x, tg) in enumerate(batches[:2])] + [(x3[:5], t3[:5], [20, 17, 18, 19, 16])]
    filenames = [f'clip{i}.wav' for i in range(3 * B)]
    want = {f: [[] for _ in grid_a] for f in fusion}
    want_tags = []
    for x, tg, idx in loader:
        if x.shape[0] == B:
            _, t, r = plain(x, tg)
        else:
            _, t, r = predict_step(model, crit, post, x, tg, fusion_strategy=fusion)
        t = t.cpu().numpy()
        want_tags += [(labels[c], filenames[idx[b]], 0, 0) for b in range(len(idx)) for c in range(C2_CLASSES) if t[b, c] == 1]
        for f in fusion:
            for k, rows in enumerate(_want_rows(r[f], grid_a)):
                want[f][k] += [(labels[c], on, off, sc, filenames[idx[b]]) for b, c, on, off, sc in rows]
    tag_table, sets = get_sedt_predictions(model, crit, post, loader, d, filenames, metrics=m)
    assert set(sets) == set(fusion) and tag_table.to_rows() == want_tags
    for f in fusion:
        assert len(sets[f]) == 3 and [t.threshold for t in sets[f]] == [float(np.float32(t)) for t in grid_a]
        for k in range(3):
            assert sets[f].to_rows(k) == want[f][k], (f, k)
    assert len(sets[1].at(0)) > 10 and {r[4] for r in sets[1].to_rows(0)} <= set(filenames)
    # 6. with metrics= the same pass filled the counters: the scores evaluate_events gives
    scored = m.compute()
    assert scored == evaluate_events(model, crit, post, loader, m) and 0.0 < scored[1]['f1'] < 1.0
    runtime.set_compute_dtype('bf16')
