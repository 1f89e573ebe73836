"""Measure "Levels measured after the effects" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/relevel_measure.py --calls 10 --rounds 3

Every step runs in a child process of its own under a time limit of its own (``--limit`` seconds), one after another; the first step
that fails or runs out of time ends the run.  The bank and the plans are those of tests/reverb_measure.py (and so of
tests/soundscape_measure.py and tests/stretch_measure.py): 24 sounds of 0.5 .. 4 s, 3 backgrounds of 30 s, eight responses of 1 s, 64
clips of 10 s with 1 - 9 events each, np.random.seed(2):
  stage   sedt_relevel alone (DeviceRelevel.launch, records uploaded per call) over the events of the C2-sized plan - the bank
          excerpts of the plain plan - in both modes; the events, their samples, the longest region and the doubles of workspace
  batch   SoundscapeClips.batch (mix -> mel -> transform) with and without relevel, in both level modes, on three plans of that seed:
          plain, effects (pitch_shift (-3, 3), time_stretch (0.8, 1.2)), reverb (every event wet)
Per path the median over ``--rounds`` windows of ``--calls`` back-to-back calls between two device events, the paths alternating inside
a round; recorded, not a gate."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from reverb_measure import N_FFT, SR, decaying, measure  # noqa: E402

MODES = ('rms', 'lufs')
PLANS = ('plain', 'effects', 'reverb')
STEPS = ('stage', 'batch_rms', 'batch_lufs')


def setup(B, level, relevel=False):
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    labels = [f'c{i}' for i in range(10)]
    gen = np.random.default_rng(1)
    sounds = [(0.1 * gen.standard_normal(int(gen.integers(SR // 2, 4 * SR)))).astype(np.float32) for _ in range(24)]
    scapes = SoundscapeClips(DeviceMelSpectrogram.dcase(), labels, 10.0, max_targets=32, reverb_n_fft=N_FFT, level=level, relevel=relevel)
    scapes.add_events(sounds, [i % 10 for i in range(24)])
    scapes.add_backgrounds([(0.02 * gen.standard_normal(30 * SR)).astype(np.float32) for _ in range(3)])
    scapes.add_rirs([decaying(gen, SR) for _ in range(8)], rooms=[0, 0, 1, 1, 2, 2, 3, 3])
    plans = {}
    for name, kw in (('plain', {}), ('effects', dict(pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2))), ('reverb', dict(reverb=True))):
        np.random.seed(2)
        plans[name] = scapes.draw(B, **kw)
    return scapes, plans


def step_stage(args):
    from sound_event_detection_transformer_amd.utilities.relevel import DeviceRelevel
    res = {}
    for mode in MODES:
        scapes, plans = setup(args.batch, mode)
        ev = plans['plain'].ev
        rl = DeviceRelevel(SR, mode)
        jobs, doubles = rl.jobs(scapes.src_off[ev['src']] + ev['src_start'], ev['n'], plans['plain'].target_db)
        ws, out = rl.workspace(doubles), rl.outputs(len(jobs))
        got = measure({f'c2_plan_stage_{mode}_us': lambda: rl.launch(scapes.flat, jobs, workspace=ws, out=out)}, args.calls, args.rounds)
        assert not rl.launch(scapes.flat, jobs, workspace=ws, out=out)[2].any().item()
        got.update(events=int(len(jobs)), samples=int(jobs['n'].sum()), longest_region=int(jobs['n'].max()),
                   longest_region_hops=int(jobs['n'].max()) // rl.hop, workspace_doubles=int(doubles))
        res[mode] = got
    return res


def step_batch(args, level):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    scapes, plans = setup(args.batch, level)
    transform = DeviceBoxTransform(500)
    res = {}
    for name in PLANS:
        plan = plans[name]
        got = measure({f'batch_{name}_relevel_us': lambda: scapes.batch(transform, plan, relevel=True),
                       f'batch_{name}_us': lambda: scapes.batch(transform, plan, relevel=False)}, args.calls, args.rounds)
        scapes.batch(transform, plan, relevel=True)
        assert not scapes.last_relevel[2].any().item()
        got.update(events=int(plan.ev.shape[0]), relevel_jobs=int(len(scapes.last_fx['relevel_jobs'])),
                   longest_region=int(scapes.last_fx['relevel_jobs']['n'].max()))
        res[name] = got
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--limit', type=int, default=240, help='seconds every step may take')
    ap.add_argument('--step', choices=STEPS, help='run this step alone, in this process')
    args = ap.parse_args()
    if args.step:
        assert torch.cuda.is_available(), 'a measurement needs the GPU'
        fn = {'stage': lambda: step_stage(args), 'batch_rms': lambda: step_batch(args, 'rms'), 'batch_lufs': lambda: step_batch(args, 'lufs')}
        print(json.dumps({args.step: fn[args.step]()}), flush=True)
        return 0
    for step in STEPS:                                             # a fresh child per step, each under its own time limit
        cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(args.batch),
               '--calls', str(args.calls), '--rounds', str(args.rounds)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f'relevel_measure: step {step} ended with status {rc}: nothing more is started', flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
