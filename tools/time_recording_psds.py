"""What PSDS on a recording costs ("PSDS on recordings", quotes its output):

    python tools/time_recording_psds.py --minutes 10 --hop 5 --thresholds 1
    python tools/time_recording_psds.py --minutes 10 --hop 5 --thresholds 50

The setting of tools/time_recording_metrics.py: the same seeded-noise recording in the URBAN-SED geometry already on the device, 10 s
windows, thresholds taken from the model's own scores.  The reference is made from the detector's own events at the lowest threshold
(every third one shifted a little, every third moved away, every third kept in place under the next label) so that true positives,
false positives and cross triggers all occur.  Timed, each as 100 launches of one entry point captured in one graph, a replay between
device events divided by 100, the graphs alternated over 15 timed replays after 3 warm-up replays (back-to-back launch intervals
inside a graph, not kernel times): the stitch launch of the call, ops.recording_psds_counts on its output, and the two recmetrics
launches beside it.  And the alternative at the parent commit, by the host clock (median of 5): fetching count / out / status and running
tests/psds_ref.counts on the host."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
LAUNCHES, WARM, TIMED = 100, 3, 15


def captured(fn):
    """LAUNCHES calls of fn() in one graph"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--hop', type=float, default=5.0)
    ap.add_argument('--batch-windows', type=int, default=8)
    ap.add_argument('--thresholds', type=int, default=1)
    ap.add_argument('--no-clocks', action='store_true')
    args = ap.parse_args()
    import psds_ref
    import recording_metrics_ref as M
    import recording_psds_ref as P
    from sound_event_detection_transformer_amd import ops, sedt
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector
    from sound_event_detection_transformer_amd.utilities.recording_metrics import RecordingMetrics
    from sound_event_detection_transformer_amd.utilities.recording_psds import RecordingPsds
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    dev = torch.device('cuda', 0)
    model, _, post = sedt.build_model(sedt.default_args(dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.to(dev).eval()
    mel, transform = DeviceMelSpectrogram.urbansed(), DeviceBoxTransform(500)
    C, K = 10, args.thresholds
    labels = [f'c{i}' for i in range(C)]
    wave = 0.1 * torch.randn(int(args.minutes * 60 * mel.sr), generator=torch.Generator().manual_seed(1)).to(dev)
    probe = EventDecoder(labels, 10.0, thresholds=[0.0], fusion_strategy=(1,))
    det = RecordingDetector(model, post['bbox'], probe, mel, transform, 10.0, args.hop, batch_windows=args.batch_windows, graphed=False)
    rec, _, _ = det.records([wave])
    live = ops.decode_events_views(rec[1], 10)
    scores = live[3][live[1] >= 0].cpu().numpy()
    grid = [float(np.quantile(scores, q)) for q in (np.linspace(0.3, 0.95, K) if K > 1 else [0.6])]
    dec = EventDecoder(labels, 10.0, thresholds=grid, fusion_strategy=(1,))
    det = RecordingDetector(model, post['bbox'], dec, mel, transform, 10.0, args.hop, batch_windows=args.batch_windows)
    preds, _ = det([wave], ['noise.wav'])
    rows = preds[1].to_rows(0)
    nxt = lambda lab: labels[(labels.index(lab) + 1) % C]
    reference = {'noise.wav': [((lab, on + 0.1, off + 0.1), (lab, on + 1.0, off + 1.5), (nxt(lab), on, off))[i % 3]
                               for i, (lab, on, off, _, _) in enumerate(rows)]}
    metrics = RecordingMetrics(dec, time_resolution=1.0).set_reference(reference)
    psds = RecordingPsds(dec).set_reference(reference)

    rec, _, plan = det.records([wave])
    win_off, start, t, dur = plan
    cap = min(4096, len(start) * 10)
    d_off, d_t, d_dur = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (win_off, t, dur))
    count, out, st = ops.stitch_events(rec[1], d_off, d_t, d_dur, C, 0.0, cap)
    idx = torch.from_numpy(metrics.recording_index(['noise.wav'])).to(dev)
    words = torch.tensor([M.n_words(float(dur[0]), [(0, a, b) for _, a, b in reference['noise.wav']], 1.0)], dtype=torch.int32, device=dev)
    workspace = torch.empty(K * C * ((cap + 63) // 64), dtype=torch.int64, device=dev)
    s_ev, s_seg, s_psds = torch.zeros_like(st), torch.zeros_like(st), torch.zeros_like(st)
    graphs = {
        'stitch_events': captured(lambda: ops.stitch_events(rec[1], d_off, d_t, d_dur, C, 0.0, cap, count=count, out=out, status=st)),
        'recording_psds_counts': captured(lambda: ops.recording_psds_counts(count, out, st, cap, idx, psds.table, d_dur, psds.counts, 0,
                                                                            pass_words=workspace, status=s_psds)),
        'recording_event_counts': captured(lambda: ops.recording_event_counts(count, out, st, cap, idx, metrics.table, metrics.ev, metrics.tag,
                                                                              0, status=s_ev)),
        'recording_segment_counts': captured(lambda: ops.recording_segment_counts(count, out, st, cap, idx, metrics.table, words, metrics.seg,
                                                                                  metrics.sdi, 0, time_resolution=1.0, status=s_seg)),
    }
    times = {n: [] for n in graphs}
    for r in range(WARM + TIMED):
        for n, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if r >= WARM:
                times[n].append(1e3 * a.elapsed_time(b) / LAUNCHES)
    assert not s_ev.any().item() and not s_seg.any().item() and not s_psds.any().item()

    # one update from zeroed counters against the host oracle, which is also the alternative being timed
    psds.reset()
    psds.update({1: (count, out, st)}, cap, ['noise.wav'], durations=dur)
    got = psds.counts_host()[0]
    index = {l: i for i, l in enumerate(labels)}
    refs = P.sort_refs([(index[l], a, b) for l, a, b in reference['noise.wav']])
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        h_count, h_out = count.cpu().numpy(), out.cpu().numpy()
        st.cpu()
        h_times = ops.stitch_events_views(h_out)[0]
        tables = [[(0, c, float(h_times[k, 0, c, i, 0]), float(h_times[k, 0, c, i, 1])) for c in range(C) for i in range(h_count[k, 0, c])]
                  for k in range(K)]
        h_counts = np.asarray(psds_ref.counts(tables, [refs], [float(dur[0])], labels), np.int64).reshape(K, C, C + 1)
        host.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(got, h_counts)
    score = psds.compute()[1]['psds']
    clocks = None
    if not args.no_clocks:
        import bench
        clocks = bench.clocks_under_load(lambda: det.step(None))
    d = np.arange(C)
    us = {n + '_us': {'median': round(float(np.median(v)), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)} for n, v in times.items()}
    print(json.dumps(dict({'minutes': args.minutes, 'hop_s': args.hop, 'windows': len(start), 'thresholds': K, 'cap': cap,
                           'stitched_events': int(count.sum()), 'reference_events': len(refs), 'tp': int(got[:, d, d].sum()),
                           'cross_triggers': int(got[:, :, :C].sum() - got[:, d, d].sum()), 'false_positives': int(got[:, :, C].sum()),
                           'psds': {str(k): round(v, 6) for k, v in score.items()}, 'launches_per_graph': LAUNCHES, 'timed_replays': TIMED,
                           'host_fetch_and_psds_ref_ms': round(float(np.median(host)), 3), 'clocks': clocks}, **us)))


if __name__ == '__main__':
    main()
