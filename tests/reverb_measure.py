"""Measure "Reverberation on the device" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/reverb_measure.py --calls 20 --rounds 5

Every step runs in a child process of its own under a time limit of its own (``--limit`` seconds), one after another; the first step
that fails or runs out of time ends the run.  All at n_fft 2048:
  stage   ONE sound of 10 s with a response of 1 s, at 16 kHz and at 44.1 kHz (sedt_reverb through DeviceReverb.launch, records
          uploaded per call), for every ``group`` G (output blocks per workgroup of the product launch) the entry point takes; next to
          each time the bytes of X and H the product launch asks for - per workgroup (P + G - 1) K 8 of X and P K 8 of H, less where the
          window leaves the stored blocks - and those bytes over the WHOLE call's time: a lower bound of the bandwidth the launch
          reaches, since the call also holds the forward launch and the inverse transforms; the same call with a response of ONE tap
          (no product loop to speak of) is printed beside it
  plan    the wet events of a C2-sized plan: 64 clips of 10 s, 1 - 9 events each, every event wet with one of eight responses of 1 s,
          drawn over the seeded bank of tests/soundscape_measure.py (24 sounds of 0.5 .. 4 s, 3 backgrounds of 30 s), per G; the
          workspace the plan needs
  batch   SoundscapeClips.batch (mix -> mel -> transform) on that plan next to the same seed's plan without reverb
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

SR, N_FFT = 16000, 2048
GROUPS = (1, 2, 4, 8)
STEPS = ('stage', 'plan', 'batch')


def window_us(fn, calls):
    """microseconds per call of ``calls`` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def measure(paths, calls, rounds):
    for fn in paths.values():                                      # warm-up: code objects, the pinned rings, the buffers
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in paths}
    for _ in range(rounds):                                        # the paths alternate inside every round
        for k, fn in paths.items():
            got[k].append(window_us(fn, calls))
    res = {}
    for k, v in got.items():
        res[k] = round(float(np.median(v)), 1)
        res[k.replace('_us', '_spread_us')] = [round(float(min(v)), 1), round(float(max(v)), 1)]
    return res


def mac_bytes(ns, taps, G, n_fft=N_FFT):
    """the bytes of X and of H the product launch asks for over the jobs (ns[e] dry samples, taps[e] taps), as the kernel walks them"""
    Bs, K = n_fft // 2, n_fft // 2 + 1
    bx = bh = 0
    for n, L in zip(ns, taps):
        nb, P, nout = -(-n // Bs) + 1, -(-L // Bs), -(-(n + L - 1) // Bs)
        for j0 in range(0, nout, G):
            p_lo, p_hi = max(j0 - nb + 1, 0), min(P - 1, j0 + G - 1)
            steps = p_hi - p_lo + 1
            blocks = [i for i in range(j0 - p_hi, j0 + G - p_lo) if 0 <= i < nb]          # the window's first G and one more per further step
            bx += len(blocks) * K * 8
            bh += steps * K * 8
    return bx, bh


def decaying(gen, L):
    return (gen.standard_normal(L) * np.exp(-6.0 * np.arange(L) / L)).astype(np.float32)


def step_stage(args):
    from sound_event_detection_transformer_amd.utilities import reverb as M
    gen = np.random.default_rng(1)
    res = {}
    for sr in (16000, 44100):
        rv = M.DeviceReverb(sr, N_FFT).add_rirs([decaying(gen, sr), np.ones(1, np.float32)])
        one = torch.from_numpy((0.1 * gen.standard_normal(10 * sr)).astype(np.float32)).cuda()
        jobs, floats = M.reverb_jobs([10 * sr], [0], rv.rir_lens, N_FFT, fades=[sr // 100])
        floor, _ = M.reverb_jobs([10 * sr], [1], rv.rir_lens, N_FFT, fades=[sr // 100])
        dst, ws = torch.zeros(11 * sr, device='cuda'), torch.empty(floats, device='cuda')
        paths = {f'one_10s_sound_1s_response_G{g}_us': (lambda g=g: rv.launch(one, jobs, dst, ws, group=g)) for g in GROUPS}
        paths['one_10s_sound_one_tap_us'] = lambda: rv.launch(one, floor, dst, ws)
        got = measure(paths, args.calls, args.rounds)
        assert not rv.launch(one, jobs, dst, ws).any().item()
        got['workspace_MB'] = round(4 * floats / 2 ** 20, 1)
        for g in GROUPS:
            bx, bh = mac_bytes([10 * sr], [sr], g)
            got[f'G{g}_X_MB'], got[f'G{g}_H_MB'] = round(bx / 1e6, 1), round(bh / 1e6, 1)
            got[f'G{g}_GBps_over_the_whole_call'] = round((bx + bh) / 1e3 / got[f'one_10s_sound_1s_response_G{g}_us'], 1)
        res[f'sr_{sr}'] = got
    return res


def c2_setup(B):
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    labels = [f'c{i}' for i in range(10)]
    gen = np.random.default_rng(1)
    sounds = [(0.1 * gen.standard_normal(int(gen.integers(SR // 2, 4 * SR)))).astype(np.float32) for _ in range(24)]
    scapes = SoundscapeClips(DeviceMelSpectrogram.dcase(), labels, 10.0, max_targets=32, reverb_n_fft=N_FFT)
    scapes.add_events(sounds, [i % 10 for i in range(24)])
    scapes.add_backgrounds([(0.02 * gen.standard_normal(30 * SR)).astype(np.float32) for _ in range(3)])
    scapes.add_rirs([decaying(gen, SR) for _ in range(8)], rooms=[0, 0, 1, 1, 2, 2, 3, 3])
    np.random.seed(2)
    plain = scapes.draw(B)
    np.random.seed(2)
    plan = scapes.draw(B, reverb=True)
    return scapes, plain, plan


def step_plan(args):
    scapes, plain, plan = c2_setup(args.batch)
    rec = scapes._reverb_records(plan, plan.ev, scapes.src_off[:-1], np.asarray(scapes.ns, np.int64), int(scapes.src_off[-1]))
    rv, jobs = scapes.reverberator(), rec['jobs']
    buf, ws = scapes._effect_buffer(rec['samples']), rv.workspace(rec['floats'])
    got = measure({f'c2_plan_stage_G{g}_us': (lambda g=g: rv.launch(buf, jobs, buf, ws, group=g)) for g in GROUPS}, args.calls, args.rounds)
    assert not rv.launch(buf, jobs, buf, ws).any().item()
    taps = [rv.rir_lens[int(r)] for r in jobs['rir']]
    for g in GROUPS:
        bx, bh = mac_bytes([int(n) for n in jobs['n']], taps, g)
        got[f'G{g}_X_MB'], got[f'G{g}_H_MB'] = round(bx / 1e6, 1), round(bh / 1e6, 1)
        got[f'G{g}_GBps_over_the_whole_call'] = round((bx + bh) / 1e3 / got[f'c2_plan_stage_G{g}_us'], 1)
    got.update(batch=args.batch, events=int(plan.ev.shape[0]), events_wet=int(len(jobs)), samples_in=int(jobs['n'].sum()),
               samples_out=int(rec['tails']['total'].sum()), workspace_MB_plan=round(4 * rec['floats'] / 2 ** 20, 1),
               spectra_MB=round(8 * rv.n_parts * (N_FFT // 2 + 1) / 2 ** 20, 1))
    return got


def step_batch(args):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    scapes, plain, plan = c2_setup(args.batch)
    transform = DeviceBoxTransform(500)
    got = measure({'batch_with_reverb_us': lambda: scapes.batch(transform, plan),
                   'batch_without_reverb_us': lambda: scapes.batch(transform, plain)}, args.calls, args.rounds)
    assert not scapes.last_rv_status.any().item()
    got.update(batch=args.batch, events=int(plan.ev.shape[0]))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=240, help='seconds every step may take')
    ap.add_argument('--step', choices=STEPS, help='run this step alone, in this process')
    args = ap.parse_args()
    if args.step:
        assert torch.cuda.is_available(), 'a measurement needs the GPU'
        print(json.dumps({args.step: {'stage': step_stage, 'plan': step_plan, 'batch': step_batch}[args.step](args)}), flush=True)
        return 0
    for step in STEPS:                                             # a fresh child per step, each under its own time limit
        cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(args.batch),
               '--calls', str(args.calls), '--rounds', str(args.rounds)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f'reverb_measure: step {step} ended with status {rc}: nothing more is started', flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
