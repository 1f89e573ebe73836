"""GPU: the segment-based counts of csrc/metrics.hip (through utilities/metrics.EventMetrics(time_resolution=...) and
engine.GraphedPredictStep(metrics=...)) against the CPU restatement of sed_eval's SegmentBasedMetrics (tests/segment_metrics_ref.py)
fed with the same f32 tensors.  Counters are integers and must be EQUAL, not close."""
import numpy as np
import pytest
import torch

import event_metrics_ref as R
import segment_metrics_ref as S
from oracle import sedt_oracle as O
from oracle.criterion_oracle import synthetic_targets

pytestmark = pytest.mark.gpu

C = 10


def _grid(rng, r, lo, hi):
    """a time on the decimal grid of r (0.3 at r = 0.1: the quotient falls just below an integer in float64)"""
    return round(int(rng.integers(int(lo / r), int(hi / r))) * r, 6)


def _reference(rng, n, r):
    """n clips: ~10 % without a reference row (None), some with an empty row, else 1-8 events with onsets / offsets on the decimal
    grid of r or free; some offsets past max_len = 10 s"""
    refs = []
    for _ in range(n):
        u = rng.random()
        if u < 0.1:
            refs.append(None)
            continue
        ev = []
        for _ in range(0 if u < 0.15 else int(rng.integers(1, 9))):
            on = _grid(rng, r, 0, 9.5) if rng.random() < 0.6 else float(rng.uniform(0, 9.5))
            off = on + (_grid(rng, r, 0.2, 3) if rng.random() < 0.6 else float(rng.uniform(0.2, 3)))
            ev.append((int(rng.integers(0, C)), on, round(off, 6) if rng.random() < 0.5 else off))
        refs.append(ev)
    return refs


def _edge(rng, t):
    """t in f32, or one f32 ulp either side: on a segment edge, just below it, just above it"""
    t = np.float32(t)
    return [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))][int(rng.integers(0, 3))]


def _adversarial_batch(rng, refs, clip_idx, Q, r):
    """PostProcess-like outputs: a share of the queries on a reference event of the clip or on segment edges of the grid (exact in
    decimal, or one f32 ulp off), others free; some wholly outside [0, 10] (zero length after the clip); scores on 0.5"""
    B = len(clip_idx)
    Sc = rng.choice(np.array([0.3, 0.5, 0.5, 0.7, 0.9], np.float32), (B, Q)).astype(np.float32)
    Sc = np.where(rng.random((B, Q)) < 0.5, Sc, rng.uniform(0.2, 1.0, (B, Q))).astype(np.float32)
    L = rng.integers(0, C, (B, Q))
    on = rng.uniform(-0.5, 9.8, (B, Q))
    X = np.stack([on, on + rng.choice([0.1, 0.2, 0.5, 1.5, 3.0], (B, Q))], -1).astype(np.float32)
    for b, k in enumerate(clip_idx):
        ev = refs[k] if k >= 0 and refs[k] is not None else []
        for i in range(Q):
            u = rng.random()
            if i < len(ev) and u < 0.6:
                c, r_on, r_end = ev[i]
                L[b, i], X[b, i] = c, (_edge(rng, r_on), _edge(rng, r_end))
            elif u < 0.8:
                a = _grid(rng, r, 0, 9.5)
                X[b, i] = (_edge(rng, a), _edge(rng, a + _grid(rng, r, 0.2, 2)))
            elif u < 0.85:
                X[b, i] = (-0.7, -0.2) if rng.random() < 0.5 else (10.3, 10.9)
    return Sc, L, X


def _dev(Sc, L, X):
    return (torch.from_numpy(Sc).cuda(), torch.from_numpy(np.asarray(L, np.int64)).cuda(), torch.from_numpy(X).cuda())


@pytest.mark.parametrize('B,Q', [(64, 10), (32, 20)])
@pytest.mark.parametrize('del_overlap', [True, False])
@pytest.mark.parametrize('r', [1.0, 0.1])
def test_segment_counters_equal_the_restatement(B, Q, del_overlap, r):
    """three fusion strategies, two batches, a clip outside the table in each: the segment counters equal the restatement; the
    event-based and tag counters are bit-identical with segment scoring on and off; one launch per fusion strategy either way"""
    from sound_event_detection_transformer_amd import lib
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    rng = np.random.default_rng(B + Q + 10 * del_overlap + int(100 * r))
    N, fusion = 2 * B, (1, 2, 3)
    refs = _reference(rng, N, r)
    labels = [f'c{i}' for i in range(C)]
    table = [None if e is None else [(f'c{c}', on, end) for c, on, end in e] for e in refs]
    m = EventMetrics(labels, 10.0, del_overlap=del_overlap, fusion_strategy=fusion, time_resolution=r).set_reference(table)
    plain = EventMetrics(labels, 10.0, del_overlap=del_overlap, fusion_strategy=fusion).set_reference(table)
    assert m.n_seg_words == (1 if r == 1.0 else 2)
    h = S.HostSegmentMetrics(C, refs, 10.0, r, n_fusion=3, del_overlap=del_overlap)
    order = rng.permutation(N)
    for s in range(0, N, B):
        idx = [int(k) for k in order[s:s + B]]
        idx[0] = -1                                                       # a clip outside the reference table
        res, hostres = {}, {}
        for m_ in fusion:
            hostres[m_] = _adversarial_batch(rng, refs, idx, Q, r)
            res[m_] = _dev(*hostres[m_])
        tags = rng.integers(0, 2, (B, C))
        with lib.launch_log() as log:
            m.update(res, torch.from_numpy(tags).cuda(), idx)
        assert log['event_segment_metrics_update'] == 3 and log['event_metrics_update'] == 0
        with lib.launch_log() as log:
            plain.update(res, torch.from_numpy(tags).cuda(), idx)
        assert log['event_metrics_update'] == 3 and log['event_segment_metrics_update'] == 0
        for i, m_ in enumerate(fusion):
            h.update(i, *hostres[m_], idx, at_tags=tags if i == 0 else None)
    torch.cuda.synchronize()
    ev, tag = m.counts()
    seg, sdi = m.segment_counts()
    assert seg[:, :, 0].sum() > 50 and (sdi > 0).all()                 # hits, substitutions, deletions and insertions occurred
    assert np.array_equal(seg, h.seg), np.argwhere(seg != h.seg)[:10]
    assert np.array_equal(sdi, h.sdi), (sdi, h.sdi)
    assert np.array_equal(ev, h.ev) and np.array_equal(tag, h.tag)
    ev0, tag0 = plain.counts()
    assert np.array_equal(ev, ev0) and np.array_equal(tag, tag0)


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
        tg = synthetic_targets(B, seed + 100 + s, C)
        for t in tg:
            t['orig_size'] = torch.tensor(10.0)
        out.append((x, [{k: v.cuda() for k, v in t.items()} for t in tg]))
    return out


def test_graphed_predict_step_with_segment_metrics():
    """C2 (enc_layers 3, Q 10, audio tags), f32 mode, B 64, fusion strategies 1 and 2, three batches, r = 1.0 (the reference's):
    building the step leaves every counter at zero; the counters the graph accumulates equal the restatement fed with the graph's own
    outputs; reset() plus a second pass gives the same integers; evaluate_events (graph + an eager short last batch) gives the
    segment scores and the summary row of finalize() on the restatement's counters."""
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, predict_step, evaluate_events
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics, finalize, summary
    model, crit, post = _c2_model()
    B, fusion = 64, (1, 2)
    batches = _batches(3, B, 500)
    rng = np.random.default_rng(13)
    eager = [predict_step(model, crit, post, x, tg, fusion_strategy=fusion)[2][1] for x, tg in batches]
    thr = float(np.quantile(torch.cat([r[0] for r in eager]).cpu().numpy(), 0.7))
    refs = []
    for sc, lb, bx in ((t.cpu().numpy() for t in r) for r in eager):
        for b in range(B):
            if rng.random() < 0.1:
                refs.append(None)
                continue
            dec = R.decode_strong(sc[b], lb[b], bx[b], threshold=thr, max_len=10.0)[:int(rng.integers(0, 6))]
            refs.append([(c, on + float(rng.choice([0.0, 0.5, 1.0])), end + float(rng.uniform(0.0, 1.5))) for c, on, end, _ in dec])
    labels = [f'c{i}' for i in range(C)]
    m = EventMetrics(labels, 10.0, threshold=thr, fusion_strategy=fusion, time_resolution=1.0)
    m.set_reference(refs)
    g = GraphedPredictStep(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=fusion, metrics=m)
    assert not any(t.any() for t in m._read())                          # building the step leaves the counters alone
    h = S.HostSegmentMetrics(C, refs, 10.0, 1.0, n_fusion=2, threshold=thr)
    for n, (x, tg) in enumerate(batches):
        idx = list(range(n * B, (n + 1) * B))
        _, gt, gr = g(x, tg, idx)
        torch.cuda.synchronize()
        for f in fusion:
            h.update(fusion.index(f), *(t.cpu().numpy() for t in gr[f]), idx, at_tags=gt.cpu().numpy() if f == fusion[0] else None)
    seg, sdi = m.segment_counts()
    assert seg[:, :, 0].sum() > 10 and sdi.sum() > 0
    assert np.array_equal(seg, h.seg), np.argwhere(seg != h.seg)[:10]
    assert np.array_equal(sdi, h.sdi), (sdi, h.sdi)
    assert all(np.array_equal(a, b) for a, b in zip(m.counts(), (h.ev, h.tag)))
    m.reset()
    for n, (x, tg) in enumerate(batches):
        g(x, tg, list(range(n * B, (n + 1) * B)))
    seg2, sdi2 = m.segment_counts()
    assert np.array_equal(seg2, seg) and np.array_equal(sdi2, sdi)
    # evaluate_events: two full batches through a new graph, then the third as two short batches through the eager predict_step
    x3, t3 = batches[2]
    loader = [(x, tg, list(range(n * B, (n + 1) * B))) for n, (x, tg) in enumerate(batches[:2])]
    loader += [(x3[:40], t3[:40], list(range(2 * B, 2 * B + 40))), (x3[40:], t3[40:], list(range(2 * B + 40, 3 * B)))]
    h2 = S.HostSegmentMetrics(C, refs, 10.0, 1.0, n_fusion=2, threshold=thr)
    for x, tg, idx in loader:
        if x.shape[0] == B:
            _, t, r = g(x, tg, idx)                     # (counts into m as well: evaluate_events resets it first)
        else:
            _, t, r = predict_step(model, crit, post, x, tg, fusion_strategy=fusion)
        for f in fusion:
            h2.update(fusion.index(f), *(v.cpu().numpy() for v in r[f]), idx, at_tags=t.cpu().numpy() if f == fusion[0] else None)
    got = evaluate_events(model, crit, post, loader, m)
    want = finalize(h2.ev, h2.tag, labels, fusion, seg=h2.seg, sdi=h2.sdi)
    assert got == want
    assert 0.0 < got[1]['segment']['f1'] < 1.0 and got[1]['segment']['overall']['error_rate'] > 0.0
    assert m.summary(got) == summary(want) and set(summary(got)) == {1, 2}
    runtime.set_compute_dtype('bf16')
