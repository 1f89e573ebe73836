"""One validation pass with the predictions decoded on the device, at the C2 shape (B 64, Q 10, C 10, one fusion strategy, twenty
batches), in ONE process:
  * engine.evaluate_events' loop (GraphedPredictStep(metrics=...) replays + one metrics.compute()): the scores only;
  * engine.get_sedt_predictions with K = 1 threshold and with K = 50: the rows of every operating point.
Each pass replays a step built beforehand (a capture costs seconds and is paid once per run, not per epoch); wall-clock times with a
device synchronisation at the end, the variants alternated over 5 rounds.  For the prediction passes the host's share is printed as
well: the time spent in utilities.predictions.collect (waiting for a batch's copy + unpacking it) and the time of the same replays
with nothing unpacked (the device alone).  A pass whose wall time is the collect time and not the device's is bound by the host.

Launch times: run under a kernel trace,
    rocprofv3 --kernel-trace --stats -d DIR -o decode -- python tools/time_decode.py --launches
and summarize it with `python tools/time_decode.py --trace DIR/decode_results.db` (rocprofv3's SQLite output): 5 + 50 launches at
K = 1, then 5 + 50 at K = 50, split by position."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM = 50, 5
B, C, NB = 64, 10, 20


def summarize(path):
    import sqlite3
    rows = sqlite3.connect(path).execute("select name, start, end from kernels where name like '%decode_events_kernel%' "
                                         "order by start").fetchall()
    us = [(r[2] - r[1]) / 1e3 for r in rows]
    for name, t in (('K = 1', us[WARM:WARM + N]), ('K = 50', us[2 * WARM + N:2 * WARM + 2 * N])):
        print(f'decode_events_kernel {name:7s} B 64: median {np.median(t):7.2f} us  min {min(t):7.2f} us  ({len(t)} launches)')


def setup():
    from sound_event_detection_transformer_amd import runtime, sedt
    from sound_event_detection_transformer_amd.engine import predict_step
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict, synthetic_targets
    runtime.manual_seed(5)
    model, crit, post = sedt.build_model(sedt.default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.cuda().eval()
    crit.cuda()
    post = post['bbox']
    batches = []
    for s in range(NB):
        x = torch.randn(B, 1, 500, 64, generator=torch.Generator().manual_seed(1 + s)).cuda()
        tg = synthetic_targets(B, 100 + s, C)
        for t in tg:
            t['orig_size'] = torch.tensor(10.0)
        batches.append((x, [{k: v.cuda() for k, v in t.items()} for t in tg], list(range(s * B, (s + 1) * B))))
    _, tags, res = predict_step(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=(1,))
    scores = res[1][0].cpu().numpy()
    # a seeded model scores low: K = 1 decodes its top 30 % of queries, K = 50 sweeps from its top 70 % to its top 1 %
    grids = {1: [float(np.quantile(scores, 0.7))], 50: [float(np.quantile(scores, q)) for q in np.linspace(0.3, 0.99, 50)]}
    return model, crit, post, batches, res, grids


def launches():
    from sound_event_detection_transformer_amd import ops
    _, _, _, _, res, grids = setup()
    for K in (1, 50):
        thr = torch.tensor(grids[K], dtype=torch.float32).cuda()
        out = torch.empty((K, B, 1 + 5 * res[1][0].shape[1]), dtype=torch.int32).cuda()
        for _ in range(WARM + N):
            ops.decode_events(*res[1], thr, C, out=out)
        torch.cuda.synchronize()
        print('launches: K =', K, WARM + N, flush=True)


def main():
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, get_sedt_predictions
    from sound_event_detection_transformer_amd.utilities import predictions as P
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    model, crit, post, batches, _, grids = setup()
    labels, names = [f'c{i}' for i in range(C)], [f'clip{i}.wav' for i in range(NB * B)]
    rng = np.random.default_rng(0)
    refs = []
    for _ in range(NB * B):
        on = rng.uniform(0, 9, int(rng.integers(1, 9)))
        refs.append([(int(rng.integers(0, C)), float(o), min(10.0, float(o) + float(rng.uniform(0.2, 4)))) for o in on])
    m = EventMetrics(labels, 10.0, threshold=grids[1][0], fusion_strategy=(1,)).set_reference(refs)
    x0, t0, _ = batches[0]
    score_step = GraphedPredictStep(model, crit, post, x0, t0, metrics=m)
    dec = {K: P.EventDecoder(labels, 10.0, thresholds=grids[K]) for K in grids}
    steps = {K: GraphedPredictStep(model, crit, post, x0, t0, decoder=dec[K]) for K in grids}
    spent = [0.0]
    real_collect = P.collect

    def timed_collect(*a):
        t = time.perf_counter()
        real_collect(*a)
        spent[0] += time.perf_counter() - t
    P.collect = timed_collect

    def scores_pass():                                      # the body of engine.evaluate_events with the step kept
        m.reset()
        for x, tg, idx in batches:
            score_step(x, tg, idx)
        return m.compute()

    def rows_pass(K):
        return get_sedt_predictions(model, crit, post, batches, dec[K], names, step=steps[K])

    def device_pass(K):                                     # the same replays and copies, nothing unpacked
        for x, tg, _ in batches:
            steps[K](x, tg)

    variants = [('evaluate_events (scores only)', scores_pass)]
    for K in grids:
        variants += [(f'get_sedt_predictions K = {K}', lambda K=K: rows_pass(K)), (f'  replays + copies alone K = {K}', lambda K=K: device_pass(K))]
    times, host = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
    for r in range(6):                                      # round 0 warms up
        for k, fn in variants:
            torch.cuda.synchronize()
            spent[0] = 0.0
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t) * 1e3)
                host[k].append(spent[0] * 1e3)
    for K in grids:
        _, sets = rows_pass(K)
        print(f'K = {K}: {sum(len(t) for t in sets[1])} rows over {NB * B} clips and {K} thresholds')
    for k, _ in variants:
        extra = f'  of which collect (wait + unpack) {np.median(host[k]):8.3f} ms' if 'get_sedt' in k else ''
        print(f'{k:36s}: median {np.median(times[k]):8.3f} ms  min {min(times[k]):8.3f} ms per pass of {NB} batches{extra}')


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--trace':
        summarize(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == '--launches':
        launches()
    else:
        main()
