"""Measure "Soundscapes synthesized on the device" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/soundscape_measure.py --batch 64 --events 5 --calls 2000 --rounds 7

A seeded bank at 16 kHz (24 sounds of 0.5 .. 4 s over 10 classes, 3 backgrounds of 30 s) and B clips of 10 s (160 000 samples) with
``--events`` events each, next to RecordingClips.cut (sedt_cut_clips) at the same B and window over 8 annotated recordings of 60 s.
Per path two numbers, medians over ``--rounds`` windows of ``--calls`` calls between two device events, the two paths alternating:
the entry point alone on records that already lie on the device, and the host method (SoundscapeClips.mix / RecordingClips.cut: the
records through the pinned ring, then the entry point).  The bytes are the algorithm's: per output sample one background read, one
write and, under an event, one source read; a scaled clip is read and written once more."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

SR = 16000


def window_us(fn, calls):
    """microseconds per call of ``calls`` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--events', type=int, default=5)
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    B, labels = args.batch, [f'c{i}' for i in range(10)]
    mel = DeviceMelSpectrogram.dcase()
    gen = np.random.default_rng(1)
    sounds = [(0.1 * gen.standard_normal(int(gen.integers(SR // 2, 4 * SR)))).astype(np.float32) for _ in range(24)]
    scapes = SoundscapeClips(mel, labels, 10.0, max_targets=32)
    scapes.add_events(sounds, [i % 10 for i in range(24)])
    scapes.add_backgrounds([(0.02 * gen.standard_normal(30 * SR)).astype(np.float32) for _ in range(3)])
    np.random.seed(2)
    plan = scapes.draw(B, n_events=(args.events, args.events))
    window = scapes.window
    recs = [(0.1 * gen.standard_normal(60 * SR)).astype(np.float32) for _ in range(8)]
    names = [f'r{i}.wav' for i in range(8)]
    ref = {n: sorted((int(gen.integers(0, 10)), float(t), float(t + gen.uniform(0.3, 4.0))) for t in gen.uniform(0.0, 59.0, 30)) for n in names}
    clips = RecordingClips(mel, labels, 10.0, max_targets=32).add(recs, names, ref)
    picks = clips.draw(B)

    # ---- the entry points alone: records on the device once
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(scapes.dev)
    d_bg, d_ev, d_off = up(plan.bg.view(np.uint8)), up(plan.ev.view(np.uint8)), up(plan.ev_off)
    wave, blob, status, part, peak, scale = scapes.buffers(B)
    lib = L.load()

    def scape_entry():
        L.check(lib.sedt_soundscape(L.p(scapes.flat), int(scapes.src_off[-1]), L.p(scapes.table['off']), L.p(scapes.table['len']),
                                    len(scapes), L.p(d_bg), L.p(d_ev), L.p(d_off), B, window, SR, scapes.max_targets, 0.0, 1, 1.0,
                                    L.p(wave), L.p(part), L.p(peak), L.p(scale), L.p(blob), L.p(status), L.stream_ptr()), 'soundscape')

    d_rec, d_start = up(picks[0]), up(picks[1])
    c_wave, c_blob, c_status = clips.buffers(B)
    t = clips.table

    def cut_entry():
        L.check(lib.sedt_cut_clips(L.p(clips.flat), int(clips.rec_off[-1]), L.p(t['rec_off']), L.p(t['rec_len']), len(clips), L.p(d_rec),
                                   L.p(d_start), B, window, SR, L.p(t['off']), L.p(t['on']), L.p(t['end']), L.p(t['cls']), L.p(t['pmax']),
                                   t['n_events'], clips.max_targets, 0.0, L.p(c_wave), L.p(c_blob), L.p(c_status), L.stream_ptr()),
                'cut_clips')

    paths = {'soundscape_entry_us': scape_entry, 'cut_clips_entry_us': cut_entry,
             'soundscape_mix_us': lambda: scapes.mix(plan), 'cut_clips_cut_us': lambda: clips.cut(*picks)}
    for fn in paths.values():                                      # warm-up: code objects, the pinned rings
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    assert not status.any().item() and not c_status.any().item()
    got = {k: [] for k in paths}
    for _ in range(args.rounds):                                   # the paths alternate inside every round
        for k, fn in paths.items():
            got[k].append(window_us(fn, args.calls))
    ev = plan.ev
    covered = int(np.minimum(ev['n'], window - ev['onset']).sum())
    scaled = int((scapes.last_scale.cpu().numpy() != 1).sum())
    nbytes = 4 * (2 * B * window + covered + 2 * scaled * window)
    res = {'batch': B, 'window': window, 'events_per_clip': args.events, 'calls_per_window': args.calls, 'rounds': args.rounds,
           'clips_scaled': scaled, 'algorithm_bytes': nbytes}
    for k, v in got.items():
        res[k] = round(float(np.median(v)), 2)
        res[k.replace('_us', '_spread_us')] = [round(float(min(v)), 2), round(float(max(v)), 2)]
    res['soundscape_entry_GBps'] = round(nbytes / res['soundscape_entry_us'] / 1e3, 1)
    res['cut_clips_entry_GBps'] = round(8 * B * window / res['cut_clips_entry_us'] / 1e3, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
