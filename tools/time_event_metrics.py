"""The validation-score launch at C2 shapes (B 64, Q 10, C 10, one fusion strategy) without the segment-based counts and with them at
time_resolution 1.0 and 0.01 (10 s clips: 1 and 16 words per class row), then the C2 GraphedPredictStep replay without metrics, with
the event-based metrics and with the segment-based counts (r = 1.0), in ONE process.  Replay times: device events around 50 replays,
the steps alternated over 5 rounds (printed).  Launch times: run under a kernel trace,
    rocprofv3 --kernel-trace --stats -d DIR -o metrics -- python tools/time_event_metrics.py
and summarize it with `python tools/time_event_metrics.py --trace DIR/metrics_results.db` (rocprofv3's SQLite output): the launches
of the first part come first, 5 + 50 per variant in the order above, so the trace's event_metrics_kernel rows split by position.
Under the trace a replay takes several times its untraced time (every kernel of the graph is recorded): compare replays only with
each other."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM = 50, 5


def summarize(path):
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end from kernels where name like '%event_metrics_kernel%' "
                                         "order by start").fetchall()
    seg = [r for r in rows if 'event_metrics_kernel<true>' in r[0]]
    plain = [r for r in rows if 'event_metrics_kernel<false>' in r[0]]
    us = lambda rs: [(r[2] - r[1]) / 1e3 for r in rs[WARM:WARM + N]]
    for name, t in (('no segments', us(plain)), ('r = 1.0', us(seg)), ('r = 0.01', us(seg[WARM + N:]))):
        print(f'event_metrics_kernel {name:12s} B 64: median {np.median(t):7.2f} us  min {min(t):7.2f} us  ({len(t)} launches)')


def main():
    from sound_event_detection_transformer_amd import runtime, sedt
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, predict_step
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict, synthetic_targets
    B, C = 64, 10
    runtime.manual_seed(5)
    model, crit, post = sedt.build_model(sedt.default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.cuda().eval()
    crit.cuda()
    post = post['bbox']
    x = torch.randn(B, 1, 500, 64, generator=torch.Generator().manual_seed(1)).cuda()
    tg = synthetic_targets(B, 2, C)
    for t in tg:
        t['orig_size'] = torch.tensor(10.0)
    tg = [{k: v.cuda() for k, v in t.items()} for t in tg]
    _, tags, res = predict_step(model, crit, post, x, tg, fusion_strategy=(1,))
    thr = float(np.quantile(res[1][0].cpu().numpy(), 0.7))       # a seeded model scores low: decode its top 30 % of queries
    rng = np.random.default_rng(0)
    refs = []
    for _ in range(B):
        ev = []
        for _ in range(int(rng.integers(1, 9))):
            on = float(rng.uniform(0, 9))
            ev.append((int(rng.integers(0, C)), on, min(10.0, on + float(rng.uniform(0.2, 4)))))
        refs.append(ev)
    labels, idx = [f'c{i}' for i in range(C)], list(range(B))

    def metrics(r):
        return EventMetrics(labels, 10.0, threshold=thr, fusion_strategy=(1,), time_resolution=r).set_reference(refs)

    for name, r in (('no segments', None), ('r = 1.0', 1.0), ('r = 0.01', 0.01)):
        m = metrics(r)
        for _ in range(WARM + N):
            m.update(res, tags, idx)
        torch.cuda.synchronize()
        print('launches:', name, WARM + N, flush=True)

    steps = {'no metrics': GraphedPredictStep(model, crit, post, x, tg),
             'event metrics': GraphedPredictStep(model, crit, post, x, tg, metrics=metrics(None)),
             'event + segment r = 1.0': GraphedPredictStep(model, crit, post, x, tg, metrics=metrics(1.0))}
    times = {k: [] for k in steps}
    for _ in range(5):
        for k, g in steps.items():
            for _ in range(5):
                g(x, tg, idx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N):
                g(x, tg, idx)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / N)
    for k, t in times.items():
        print(f'replay {k:24s}: median {np.median(t):.4f} ms  min {min(t):.4f} ms  (5 rounds of {N})')


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--trace':
        summarize(sys.argv[2])
    else:
        main()
