"""GPU: the device validation scores (csrc/metrics.hip through utilities/metrics.EventMetrics and engine.GraphedPredictStep(metrics=...))
against the CPU restatement of decode_strong + sed_eval (tests/event_metrics_ref.py) fed with the same f32 tensors.  Counters are
integers and must be EQUAL, not close."""
import numpy as np
import pytest
import torch

import event_metrics_ref as R
from oracle import sedt_oracle as O
from oracle.criterion_oracle import synthetic_targets

pytestmark = pytest.mark.gpu

C = 10


def _reference(rng, n):
    """n clips: ~10 % without a reference row (None), some with an empty row, else 1-12 events; times both on a 0.05 s grid (collar
    edges in decimal) and free"""
    refs = []
    for k in range(n):
        u = rng.random()
        if u < 0.1:
            refs.append(None)
            continue
        ev = []
        for _ in range(0 if u < 0.15 else int(rng.integers(1, 13))):
            on = float(np.round(rng.uniform(0, 9.5) / 0.05) * 0.05) if rng.random() < 0.5 else float(rng.uniform(0, 9.5))
            ln = float(rng.choice([0.2, 0.5, 1.0, 2.0, 5.0])) if rng.random() < 0.5 else float(rng.uniform(0.2, 6))
            ev.append((int(rng.integers(0, C)), on, on + ln))
        refs.append(ev)
    return refs


def _adversarial_batch(rng, refs, clip_idx, Q):
    """PostProcess-like outputs: a share of the queries placed on a reference event of the clip, moved by exactly +-t_collar or
    +-20 % of the length (rounded to f32: either side of the edge), or by a little less / more; crossing pairs; scores on 0.5;
    lengths on 0.2; boxes outside [0, 10]"""
    B = len(clip_idx)
    S = rng.choice(np.array([0.3, 0.5, 0.5, 0.7, 0.9], np.float32), (B, Q)).astype(np.float32)
    S = np.where(rng.random((B, Q)) < 0.5, S, rng.uniform(0.2, 1.0, (B, Q))).astype(np.float32)
    L = rng.integers(0, C, (B, Q))
    on = rng.uniform(-0.5, 9.8, (B, Q))
    X = np.stack([on, on + rng.choice([0.1, 0.2, 0.2, 0.5, 1.5, 3.0], (B, Q))], -1)
    for b, k in enumerate(clip_idx):
        ev = refs[k] if k >= 0 and refs[k] is not None else []
        for i in range(min(len(ev), Q - 2)):
            if rng.random() < 0.3:
                continue
            c, r_on, r_end = ev[i]
            coll = max(0.2, 0.2 * (r_end - r_on))
            d_on = rng.choice([0.0, 0.2, -0.2, 0.1999, 0.2001, rng.uniform(-0.3, 0.3)])
            d_end = rng.choice([0.0, coll, -coll, coll - 1e-4, coll + 1e-4, rng.uniform(-0.5, 0.5)])
            L[b, i], X[b, i] = c, (r_on + d_on, r_end + d_end)
        if ev and Q > 4:                   # a crossing pair on the first event: one estimate between A and a shifted copy B
            c, r_on, r_end = ev[0]
            L[b, Q - 2], X[b, Q - 2], S[b, Q - 2] = c, (r_on + 0.15, r_end + 0.15), 0.9
            L[b, Q - 1], X[b, Q - 1], S[b, Q - 1] = c, (r_on - 0.1, r_end - 0.05), 0.9
    return S, L, X.astype(np.float32)


def _dev(S, L, X):
    return (torch.from_numpy(S).cuda(), torch.from_numpy(np.asarray(L, np.int64)).cuda(), torch.from_numpy(X).cuda())


@pytest.mark.parametrize('B,Q', [(64, 10), (32, 20)])
@pytest.mark.parametrize('del_overlap,optimal', [(True, True), (False, True), (True, False), (False, False)])
def test_counters_equal_the_restatement(B, Q, del_overlap, optimal):
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    rng = np.random.default_rng(B * 100 + Q + 7 * del_overlap + 3 * optimal)
    N = 3 * B
    refs = _reference(rng, N)
    # the crossing pairs need a second reference event next to the first: A (on, end) and B (on + 0.3, end + 0.3), same class
    for ev in refs:
        if ev:
            c, on, end = ev[0]
            ev.append((c, on + 0.3, end + 0.3))
    fusion = (1, 2, 3)
    m = EventMetrics([f'c{i}' for i in range(C)], 10.0, del_overlap=del_overlap, optimal=optimal, fusion_strategy=fusion)
    m.set_reference([None if e is None else [(f'c{c}', on, end) for c, on, end in e] for e in refs])
    h = R.HostEventMetrics(C, refs, 10.0, n_fusion=3, del_overlap=del_overlap, optimal=optimal)
    order = rng.permutation(N)
    for s in range(0, N, B):
        idx = [int(k) for k in order[s:s + B]]
        idx[0] = -1                                                       # a clip outside the reference table
        res, hostres = {}, {}
        for m_ in fusion:
            hostres[m_] = _adversarial_batch(rng, refs, idx, Q)
            res[m_] = _dev(*hostres[m_])
        tags = rng.integers(0, 2, (B, C))
        m.update(res, torch.from_numpy(tags).cuda(), idx)
        for i, m_ in enumerate(fusion):
            h.update(i, *hostres[m_], idx, at_tags=tags if i == 0 else None)
    torch.cuda.synchronize()
    ev, tag = m.counts()
    assert ev.sum() > 0 and ev[:, :, 0].sum() > 20                # there were hits
    assert np.array_equal(ev, h.ev), np.argwhere(ev != h.ev)[:10]
    assert np.array_equal(tag, h.tag), np.argwhere(tag != h.tag)[:10]


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


def test_graphed_predict_step_with_metrics():
    """C2 (enc_layers 3, Q 10, audio tags), f32 mode, B 64, fusion strategies 1 and 2, three batches: the counters the graph
    accumulates equal the restatement fed with the graph's own PostProcess outputs and tags; the tensors the step returns are
    bit-identical to a step built without metrics; after reset() a second pass gives the same counters; engine.evaluate_events
    (graph + an eager short last batch) scores the same as finalize() on the restatement's counters."""
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, predict_step, evaluate_events
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics, finalize
    model, crit, post = _c2_model()
    B, fusion = 64, (1, 2)
    batches = _batches(3, B, 300)
    rng = np.random.default_rng(11)
    # reference events around the events the model's own eager outputs decode to, so that hits, misses and collar edges all occur;
    # a fresh seeded model scores low, so the decode threshold is the 70th percentile of its scores
    eager = [predict_step(model, crit, post, x, tg, fusion_strategy=fusion)[2][1] for x, tg in batches]
    thr = float(np.quantile(torch.cat([r[0] for r in eager]).cpu().numpy(), 0.7))
    refs = []
    for sc, lb, bx in ((t.cpu().numpy() for t in r) for r in eager):
        for b in range(B):
            if rng.random() < 0.1:
                refs.append(None)
                continue
            dec = R.decode_strong(sc[b], lb[b], bx[b], threshold=thr, max_len=10.0)[:int(rng.integers(0, 6))]
            refs.append([(c, on + float(rng.choice([0.0, 0.1, 0.25])), end + float(rng.uniform(-0.3, 0.3))) for c, on, end, _ in dec])
    labels = [f'c{i}' for i in range(C)]
    m = EventMetrics(labels, 10.0, threshold=thr, fusion_strategy=fusion)
    m.set_reference(refs)
    plain = GraphedPredictStep(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=fusion)
    g = GraphedPredictStep(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=fusion, metrics=m)
    ev0, tag0 = m.counts()
    assert not ev0.any() and not tag0.any()                                     # building the step leaves the counters alone
    h = R.HostEventMetrics(C, refs, 10.0, n_fusion=2, threshold=thr)
    for n, (x, tg) in enumerate(batches):
        idx = list(range(n * B, (n + 1) * B))
        pl, pt, pr = plain(x, tg)
        pl, pt, pr = {k: v.clone() for k, v in pl.items()}, pt.clone(), {k: tuple(t.clone() for t in v) for k, v in pr.items()}
        gl, gt, gr = g(x, tg, idx)
        torch.cuda.synchronize()
        assert torch.equal(gt, pt)
        for k in pl:
            assert torch.equal(gl[k], pl[k]), k
        for f in fusion:
            for a, b in zip(gr[f], pr[f]):
                assert torch.equal(a, b)
            h.update(fusion.index(f), *(t.cpu().numpy() for t in gr[f]), idx, at_tags=gt.cpu().numpy() if f == fusion[0] else None)
    ev, tag = m.counts()
    assert ev[:, :, 0].sum() > 10 and ev[:, :, 2].sum() > ev[:, :, 0].sum()
    assert np.array_equal(ev, h.ev), np.argwhere(ev != h.ev)[:10]
    assert np.array_equal(tag, h.tag), np.argwhere(tag != h.tag)[:10]
    # a second pass after reset(): the same integers
    m.reset()
    for n, (x, tg) in enumerate(batches):
        g(x, tg, list(range(n * B, (n + 1) * B)))
    ev2, tag2 = m.counts()
    assert np.array_equal(ev2, ev) and np.array_equal(tag2, tag)
    # evaluate_events: two full batches through a new graph, then the third as two short batches through the eager predict_step
    x3, t3 = batches[2]
    loader = [(x, tg, list(range(n * B, (n + 1) * B))) for n, (x, tg) in enumerate(batches[:2])]
    loader += [(x3[:40], t3[:40], list(range(2 * B, 2 * B + 40))), (x3[40:], t3[40:], list(range(2 * B + 40, 3 * B)))]
    h2 = R.HostEventMetrics(C, refs, 10.0, n_fusion=2, threshold=thr)
    for x, tg, idx in loader:
        if x.shape[0] == B:
            _, t, r = g(x, tg, idx)                     # (counts into m as well: evaluate_events resets it first)
        else:
            _, t, r = predict_step(model, crit, post, x, tg, fusion_strategy=fusion)
        for f in fusion:
            h2.update(fusion.index(f), *(v.cpu().numpy() for v in r[f]), idx, at_tags=t.cpu().numpy() if f == fusion[0] else None)
    got = evaluate_events(model, crit, post, loader, m)
    ev3, tag3 = m.counts()
    assert np.array_equal(ev3, h2.ev) and np.array_equal(tag3, h2.tag)
    assert got == finalize(h2.ev, h2.tag, labels, fusion)
    assert set(got) == {1, 2, 'at'} and 0.0 < got[1]['f1'] < 1.0
    runtime.set_compute_dtype('bf16')
