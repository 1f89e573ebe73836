"""What scoring PSDS on the device costs: one validation pass at the C2 shape (B 64, Q 10, C 10, one fusion strategy, twenty batches,
K = 50 thresholds) through engine.get_sedt_predictions, with ``psds=`` and without it (the step as it was before PSDS: the baseline),
in ONE process.  Each pass replays a step captured beforehand.  Printed: the wall-clock time of a pass (device synchronised at the end)
and the device time of one graph replay (HIP events around 50 replays of the same batch), the variants alternated over 5 rounds after
one warm-up round, and the PSD scores of the pass.

Launch times: run each variant alone under a kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_psds.py --only psds
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_psds.py --only plain
and read psds_update_kernel next to decode_events_kernel in the *_kernel_stats.csv it writes (every launch of either is at K = 50)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
B, C, NB, K, REPLAYS = 64, 10, 20, 50, 50


def main(only=None):
    from sound_event_detection_transformer_amd import runtime, sedt
    from sound_event_detection_transformer_amd.engine import GraphedPredictStep, get_sedt_predictions, predict_step
    from sound_event_detection_transformer_amd.utilities import predictions as P
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
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
    scores = predict_step(model, crit, post, batches[0][0], batches[0][1], fusion_strategy=(1,))[2][1][0].cpu().numpy()
    grid = [float(np.quantile(scores, q)) for q in np.linspace(0.3, 0.99, K)]      # a seeded model scores low: its top 70 % .. top 1 %
    labels, names = [f'c{i}' for i in range(C)], [f'clip{i}.wav' for i in range(NB * B)]
    rng = np.random.default_rng(0)
    refs = []
    for _ in range(NB * B):
        on = rng.uniform(0, 9, int(rng.integers(1, 9)))
        refs.append([(int(rng.integers(0, C)), float(o), min(10.0, float(o) + float(rng.uniform(0.2, 4)))) for o in on])
    x0, t0, _ = batches[0]
    variants = {}
    for name in ('plain', 'psds'):
        if only in (None, name):
            dec = P.EventDecoder(labels, 10.0, thresholds=grid)
            m = PsdsMetrics(dec).set_reference(refs) if name == 'psds' else None
            variants[name] = (dec, m, GraphedPredictStep(model, crit, post, x0, t0, decoder=dec, psds=m))
    wall, replay = {n: [] for n in variants}, {n: [] for n in variants}
    for r in range(6 if only is None else 3):               # round 0 warms up
        for n, (dec, m, step) in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            get_sedt_predictions(model, crit, post, batches, dec, names, step=step, psds=m)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) * 1e3
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPLAYS):
                step.graph.replay()
            b.record()
            torch.cuda.synchronize()
            if r:
                wall[n].append(dt)
                replay[n].append(a.elapsed_time(b) / REPLAYS)
    for n in variants:
        print(f'{n:6s}: pass of {NB} batches median {np.median(wall[n]):8.3f} ms  min {min(wall[n]):8.3f} ms;  one replay median '
              f'{np.median(replay[n]):7.4f} ms  min {min(replay[n]):7.4f} ms')
    if 'psds' in variants:
        dec, m, step = variants['psds']
        get_sedt_predictions(model, crit, post, batches, dec, names, step=step, psds=m)
        counts = m.counts_host()[0]
        print('PSD scores of the pass:', {s: round(v, 5) for s, v in m.compute()[1]['psds'].items()}, ' counts: diagonal',
              int(np.trace(counts.sum(0)[:, :C])), 'world', int(counts[:, :, C].sum()), 'total', int(counts.sum()))


if __name__ == '__main__':
    main(sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == '--only' else None)
