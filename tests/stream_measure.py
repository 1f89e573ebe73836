"""Measure "Live streams" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/stream_measure.py --streams 8 64 --runs 20

Seeded noise on S streams in the DCASE geometry (16 kHz, 10 s windows, 5 s hop, SEDT E=3 Q=10 with audio tagging, bf16), host chunks of
one hop per stream and push, so every push is ONE round.  Device events after warm-up, medians: the whole push (staging copy, append,
cut, mel + transform, replay, stitch, the copies to the host), and alone: one GraphedDetectStep replay at B = S - the comparison
point, what a window costs without streaming - and the append, cut and stitch launches with their shares of the replay."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from recording_measure import device_ms                                                                      # noqa: E402


def measure(S, runs, model, post, clocks):
    from sound_event_detection_transformer_amd import ops
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.stream import StreamDetector
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    dev = torch.device('cuda', 0)
    mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
    dec = EventDecoder([f'c{i}' for i in range(10)], 10.0, thresholds=[0.05], fusion_strategy=(1,))
    det = StreamDetector(model, post, dec, mel, transform, 10.0, 5.0, n_streams=S)
    gen = torch.Generator().manual_seed(S)
    chunk = lambda: [(0.1 * torch.randn(det.hop, generator=gen)).numpy() for _ in range(S)]
    events = 0
    for _ in range(6):                                                   # warm-up: the rings fill, the graph is captured, events leave
        events += sum(len(e.at(0)['onset']) for e in det.push(chunk()).result().values())
    chunks = chunk()
    push = device_ms(lambda: det.push(chunks), runs)
    det.push(chunks).result()
    replay = device_ms(lambda: det._rd.step(None), runs)
    flat = torch.zeros(S * det.hop, device=dev)
    jobs = np.asarray([(s, (s * 977) % det.ring_samples, s * det.hop, det.hop) for s in range(S)], np.int32)
    d_jobs = torch.from_numpy(jobs.reshape(-1)).to(dev)
    append = device_ms(lambda: ops.stream_append(flat, jobs, d_jobs, det.ring), runs)
    cuts = np.asarray([(s, (s * 977 + 31) % det.ring_samples, det.window, s) for s in range(S)], np.int32)
    d_cuts = torch.from_numpy(cuts.reshape(-1)).to(dev)
    cut = device_ms(lambda: ops.stream_cut(det.ring, cuts, d_cuts, det._rd.wave), runs)
    rec = det._last[0]['dev'][1]
    state, status = ops.stitch_stream_state(dec.K, S, dev)
    emit = torch.zeros((dec.K, S, ops.STREAM_OPEN, ops.STREAM_EMIT_WORDS), dtype=torch.int32, device=dev)
    count = torch.zeros((dec.K, S), dtype=torch.int32, device=dev)
    ints = torch.tensor([1] * S + list(range(S)) + [0] * S, dtype=torch.int32, device=dev)
    t = torch.zeros(2 * S, dtype=torch.float64, device=dev)
    t[S:] = 10.0

    def stitch():
        count.zero_()
        ops.stitch_stream(rec, ints[:S], ints[S:2 * S], t[:S], t[S:], ints[2 * S:], 10, 0.0, state, emit, count, status)
    only_zero = device_ms(lambda: count.zero_(), runs)
    stitch_ms = device_ms(stitch, runs) - only_zero
    assert not status.any().item()
    out = {'streams': S, 'events_in_warmup': events, 'push_one_round_ms': round(push, 3), 'graph_replay_ms': round(replay, 3),
           'append_launch_ms': round(append, 4), 'cut_launch_ms': round(cut, 4), 'stitch_launch_ms': round(stitch_ms, 4),
           'share_of_replay': {k: round(v / replay, 4) for k, v in (('append', append), ('cut', cut), ('stitch', stitch_ms))},
           'push_over_replay': round(push / replay, 3), 'runs': runs}
    if clocks:
        import bench
        out['clocks'] = bench.clocks_under_load(lambda: det._rd.step(None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, nargs='+', default=[8, 64])
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--no-clocks', action='store_true')
    args = ap.parse_args()
    from sound_event_detection_transformer_amd import runtime, sedt
    from oracle.sedt_oracle import seeded_state_dict
    runtime.set_compute_dtype('bf16')
    model, _, post = sedt.build_model(sedt.default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.to(torch.device('cuda', 0)).eval()
    for S in args.streams:
        print(json.dumps(measure(S, args.runs, model, post['bbox'], not args.no_clocks)), flush=True)


if __name__ == '__main__':
    main()
