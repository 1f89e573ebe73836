"""RecordingClips.cut (ONE sedt_cut_clips launch: the batch's windows and their target tables) timed at the size a C2 step runs, in ONE
process, recordings resident on the device:
  16k     B = 64 windows of 10 s at 16 kHz   (64 x 160000 f32 = 41.0 MB written) from an hour of audio in 12 recordings
  44.1k   B = 64 windows of 10 s at 44.1 kHz (64 x 441000 f32 = 112.9 MB written) from an hour of audio in 12 recordings
Per case it prints
  cut          host picks -> pinned ring -> one launch; device events around N back-to-back cuts (after WARM), median of R windows + range
  copy floor   bytes the launch has to move (every window read once and written once; tables are noise) over the HBM copy rate
               (6.29 TB/s measured for a float4 copy on this part, 8 TB/s on paper)
  host route   the same picks through a host loader: NumPy cropping of host-resident recordings and target encoding into a list of
               dicts, one pinned host->device copy of the windows, TargetTables.load of the list; host clock around the whole, the
               device drained at the end of every repetition - what a step waits for when the loader is not ahead of it
  clocks       read while the launch keeps running (bench.clocks_under_load; read, never set)
    python tools/time_recording_clips.py [--short]        (--short: five minutes of audio instead of an hour, for a rehearsal)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM, R = 10, 3, 5
HBM_COPY_TBS, HBM_PEAK_TBS = 6.29, 8.0
B, SECONDS, MAX_TARGETS = 64, 10.0, 32
LABELS = [f'c{i}' for i in range(10)]


def corpus(sr, total_seconds, n_rec=12):
    """n_rec recordings of unequal length (host float32) and ~0.6 annotated events per second"""
    gen = np.random.default_rng(sr)
    share = gen.uniform(0.5, 1.5, n_rec)
    ns = np.maximum((share / share.sum() * total_seconds * sr).astype(np.int64), int(2 * SECONDS * sr))
    waves = [(0.1 * gen.standard_normal(int(n))).astype(np.float32) for n in ns]
    names = [f'rec{i}.wav' for i in range(n_rec)]
    ref = {}
    for name, n in zip(names, ns):
        dur = n / sr
        on = gen.uniform(0.0, dur, int(0.6 * dur))
        ref[name] = [(int(gen.integers(0, 10)), float(t), float(min(t + gen.uniform(0.2, 3.0), dur))) for t in on]
    return waves, names, ref


def host_route(waves, table, rec, start, window, sr, pinned, dev_wave, tables):
    """what a loader on the host does for the same picks (the arithmetic of the definition, vectorised per clip)"""
    W = window / sr
    targets = []
    for b, (r, s) in enumerate(zip(rec.tolist(), start.tolist())):
        src = waves[r][s:s + window]
        pinned[b, :len(src)] = torch.from_numpy(src)
        pinned[b, len(src):] = 0
        j0, j1 = int(table['off'][r]), int(table['off'][r + 1])
        t0 = s / sr
        a = np.maximum(table['on'][j0:j1], t0) - t0
        z = np.minimum(table['end'][j0:j1], t0 + W) - t0
        keep = (z - a) > 0
        a, z = a[keep][:MAX_TARGETS], z[keep][:MAX_TARGETS]
        targets.append({'labels': torch.from_numpy(table['cls'][j0:j1][keep][:MAX_TARGETS].astype(np.int64)),
                        'boxes': torch.from_numpy(np.stack([((a + z) * 0.5) / W, (z - a) / W], axis=-1).astype(np.float32))})
    dev_wave.copy_(pinned, non_blocking=True)
    tables.load(targets)


def case(name, mel, total_seconds, res):
    import bench
    from sound_event_detection_transformer_amd.sedt import TargetTables
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    sr = mel.sr
    waves, names, ref = corpus(sr, total_seconds)
    clips = RecordingClips(mel, LABELS, SECONDS, max_targets=MAX_TARGETS).add(waves, names, ref)
    np.random.seed(1)
    picks = [clips.draw(B) for _ in range(N)]
    for k in range(WARM):
        clips.cut(*picks[k])
    torch.cuda.synchronize()
    worst = int(clips.cut(*picks[0])[2].status.max().item())
    windows = []
    for _ in range(R):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(N):
            clips.cut(*picks[k])
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / N)
    us, lo, hi = float(np.median(windows)), min(windows), max(windows)
    mb = 2 * B * clips.window * 4 / 1e6
    floor, floor_peak = mb / HBM_COPY_TBS, mb / HBM_PEAK_TBS
    # the host route on the same picks
    pinned = torch.zeros((B, clips.window), dtype=torch.float32).pin_memory()
    dev_wave = torch.zeros((B, clips.window), dtype=torch.float32, device='cuda')
    tables = TargetTables(B, B, B, torch.device('cuda'), max_targets=MAX_TARGETS)
    host = []
    for i in range(WARM + R):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(N):
            host_route(waves, clips.host, picks[k][0], picks[k][1], clips.window, sr, pinned, dev_wave, tables)
        torch.cuda.synchronize()
        if i >= WARM:
            host.append((time.perf_counter() - t0) * 1e6 / N)
    h_us = float(np.median(host))
    clocks = bench.clocks_under_load(lambda: clips.cut(*picks[0]))
    res[name] = dict(sr=sr, B=B, window=clips.window, recordings=len(names), events=int(clips.host['on'].size), cut_us=round(us, 1),
                     min_us=round(lo, 1), max_us=round(hi, 1), moved_mb=round(mb, 1), copy_floor_us=round(floor, 1),
                     peak_floor_us=round(floor_peak, 1), times_floor=round(us / floor, 2), host_route_us=round(h_us, 1),
                     host_min_us=round(min(host), 1), host_max_us=round(max(host), 1), host_over_cut=round(h_us / us, 1),
                     worst_status=worst, clocks=clocks)
    print(f'{name:6s}: cut {us:8.1f} us (windows {lo:.1f} .. {hi:.1f}); {mb:6.1f} MB moved -> copy floor {floor:5.1f} us at {HBM_COPY_TBS} TB/s '
          f'({floor_peak:.1f} us at {HBM_PEAK_TBS}), x{us / floor:.2f}; host route {h_us:9.1f} us ({min(host):.1f} .. {max(host):.1f}), '
          f'x{h_us / us:.1f} the cut; worst status {worst}; clocks {clocks}', flush=True)


def main():
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    total = 300 if '--short' in sys.argv else 3600
    res = {}
    case('16k', DeviceMelSpectrogram.dcase(), total, res)
    case('44.1k', DeviceMelSpectrogram.urbansed(), total, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
