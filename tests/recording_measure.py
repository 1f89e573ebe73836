"""Measure "Recordings of any length" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/recording_measure.py --minutes 10 --hop 5 --runs 20

A seeded-noise recording in the URBAN-SED geometry (44.1 kHz, 10 s windows, SEDT E=3 Q=10, bf16) already on the device.  Device events
after warm-up, medians: the whole RecordingDetector pass, one GraphedDetectStep replay of batch_windows windows, the stitch launch
alone - and the host alternative: fetching the per-window records and running the NumPy restatement (tests/recording_ref.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import recording_ref as R                                                                                    # noqa: E402


def device_ms(fn, runs):
    """median milliseconds of fn() between two device events"""
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--hop', type=float, default=5.0)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--batch-windows', type=int, default=8)
    ap.add_argument('--thresholds', type=int, default=1, help='operating points decoded and stitched per pass')
    ap.add_argument('--no-clocks', action='store_true')
    args = ap.parse_args()
    from sound_event_detection_transformer_amd import ops, sedt
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    from oracle.sedt_oracle import seeded_state_dict
    dev = torch.device('cuda', 0)
    model, _, post = sedt.build_model(sedt.default_args(dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.to(dev).eval()
    mel, transform = DeviceMelSpectrogram.urbansed(), DeviceBoxTransform(500)
    labels = [f'c{i}' for i in range(10)]
    K = args.thresholds
    wave = 0.1 * torch.randn(int(args.minutes * 60 * mel.sr), generator=torch.Generator().manual_seed(1)).to(dev)
    # thresholds: quantiles of the model's own scores over the recording (a fresh seeded model scores low)
    probe = EventDecoder(labels, 10.0, thresholds=[0.0], fusion_strategy=(1,))
    det = RecordingDetector(model, post['bbox'], probe, mel, transform, 10.0, args.hop, batch_windows=args.batch_windows, graphed=False)
    rec, _, _ = det.records([wave])
    live = ops.decode_events_views(rec[1], 10)
    scores = live[3][live[1] >= 0].cpu().numpy()
    grid = [float(np.quantile(scores, q)) for q in (np.linspace(0.3, 0.95, K) if K > 1 else [0.6])]
    dec = EventDecoder(labels, 10.0, thresholds=grid, fusion_strategy=(1,))
    det = RecordingDetector(model, post['bbox'], dec, mel, transform, 10.0, args.hop, batch_windows=args.batch_windows)
    for _ in range(3):
        preds, _ = det([wave], ['noise.wav'])
    whole = device_ms(lambda: det([wave], ['noise.wav']), args.runs)
    replay = device_ms(lambda: det.step(None), args.runs)
    rec, _, plan = det.records([wave])
    win_off, start, t, dur = plan
    W, cap = len(start), min(4096, len(start) * 10)
    d_off, d_t, d_dur = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (win_off, t, dur))
    bufs = ops.stitch_events(rec[1], d_off, d_t, d_dur, 10, 0.0, cap)
    stitch = device_ms(lambda: ops.stitch_events(rec[1], d_off, d_t, d_dur, 10, 0.0, cap, count=bufs[0], out=bufs[1], status=bufs[2]), args.runs)
    torch.cuda.synchronize()
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        h = rec[1].cpu().numpy()
        want = R.stitch(h, win_off, t, dur, 10, 0.0, check_working_set=False)
        host.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(want[0], bufs[0].cpu().numpy()) and not bufs[2].any().item()
    clocks = None
    if not args.no_clocks:
        import bench
        clocks = bench.clocks_under_load(lambda: det.step(None))
    print(json.dumps({'minutes': args.minutes, 'hop_s': args.hop, 'windows': W, 'batch_windows': args.batch_windows, 'thresholds': K,
                      'events_in_records': int(rec[1][:, :, 0].sum()), 'merged_events': int(want[0].sum()),
                      'detect_recordings_ms': round(whole, 3), 'graph_replay_ms': round(replay, 3), 'stitch_launch_ms': round(stitch, 4),
                      'host_fetch_and_numpy_stitch_ms': round(float(np.median(host)), 3), 'runs': args.runs, 'clocks': clocks}))


if __name__ == '__main__':
    main()
