"""Measure "Pitch shift and time stretch on the device" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/stretch_measure.py --calls 20 --rounds 5

The stage alone (sedt_stretch through DeviceStretch.launch, records uploaded per call) at n_fft 2048, kaiser_best, over
  * ONE sound of 10 s at 16 kHz, f = 1.1, p = +2;
  * the effects of a C2-sized plan: 64 clips of 10 s, 1 - 9 events each, p in +-3 semitones, f in 0.8 .. 1.2, drawn over the seeded
    bank of tests/soundscape_measure.py (24 sounds of 0.5 .. 4 s, 3 backgrounds of 30 s);
and SoundscapeClips.batch (mix -> mel -> transform) on that plan next to the same seed's plan without effects.  Per path the median over
``--rounds`` windows of ``--calls`` back-to-back calls between two device events, the paths alternating inside a round; recorded, not a
gate.  The workspace the plan needs is printed with the times."""
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
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    from sound_event_detection_transformer_amd.utilities import stretch as M
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    B, labels = args.batch, [f'c{i}' for i in range(10)]
    gen = np.random.default_rng(1)
    sounds = [(0.1 * gen.standard_normal(int(gen.integers(SR // 2, 4 * SR)))).astype(np.float32) for _ in range(24)]
    scapes = SoundscapeClips(DeviceMelSpectrogram.dcase(), labels, 10.0, max_targets=32)
    scapes.add_events(sounds, [i % 10 for i in range(24)])
    scapes.add_backgrounds([(0.02 * gen.standard_normal(30 * SR)).astype(np.float32) for _ in range(3)])
    np.random.seed(2)
    plain = scapes.draw(B)
    np.random.seed(2)
    plan = scapes.draw(B, pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2))
    transform = DeviceBoxTransform(500)

    # ---- the stage alone
    st = scapes.stretcher()
    one = torch.from_numpy((0.1 * gen.standard_normal(10 * SR)).astype(np.float32)).cuda()
    jobs1, floats1 = M.stretch_jobs([10 * SR], [1.1], [2.0], st.n_fft)
    dst1, ws1 = torch.zeros(int(jobs1['m'][0]), device='cuda'), torch.empty(floats1, device='cuda')
    _, jobs, _, _, total, floats = scapes._effect_records(plan)
    buf, ws = scapes._effect_buffer(total), st.workspace(floats)
    paths = {'one_10s_sound_us': lambda: st.launch(one, jobs1, dst1, ws1),
             'c2_plan_stage_us': lambda: st.launch(buf, jobs, buf, ws),
             'batch_with_effects_us': lambda: scapes.batch(transform, plan),
             'batch_without_effects_us': lambda: scapes.batch(transform, plain)}
    for fn in paths.values():                                      # warm-up: code objects, the pinned rings, the buffers
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    assert not scapes.last_fx_status.any().item()
    got = {k: [] for k in paths}
    for _ in range(args.rounds):                                   # the paths alternate inside every round
        for k, fn in paths.items():
            got[k].append(window_us(fn, args.calls))
    res = {'batch': B, 'n_fft': st.n_fft, 'quality': st.quality, 'calls_per_window': args.calls, 'rounds': args.rounds,
           'events': int(plan.ev.shape[0]), 'events_transformed': int(len(jobs)), 'samples_in': int(jobs['n'].sum()),
           'samples_out': int(jobs['m'].sum()), 'workspace_MB_one_sound': round(4 * floats1 / 2 ** 20, 1),
           'workspace_MB_plan': round(4 * floats / 2 ** 20, 1)}
    for k, v in got.items():
        res[k] = round(float(np.median(v)), 1)
        res[k.replace('_us', '_spread_us')] = [round(float(min(v)), 1), round(float(max(v)), 1)]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
