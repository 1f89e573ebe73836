"""Measure "Loudness (BS.1770) on the device" on one GPU (not a test; DESIGN.md section 4 quotes its output):

    python tests/loudness_measure.py --calls 200 --rounds 7

The seeded bank of tests/soundscape_measure.py at 16 kHz (24 sounds of 0.5 .. 4 s, 3 backgrounds of 30 s): sedt_loudness next to
sedt_bank_stats over the same 27 sources, and both over ONE background of 10 minutes.  Per path the median over ``--rounds`` windows of
``--calls`` back-to-back calls between two device events, the paths alternating inside a round; recorded, not a gate.  The float64
operations are the algorithm's: two passes of 12 multiply-adds per sample."""
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


def paths(sources, loud):
    """the two entry points over ``sources`` staged back to back: {name: call}, and what the loudness call returned"""
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities.loudness import Z_ABS, work_doubles
    lens = np.asarray([len(x) for x in sources], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    flat = torch.from_numpy(np.concatenate(sources)).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens).cuda()
    n, words = len(lens), work_doubles(lens, loud.hop)
    consts = torch.from_numpy(np.concatenate([loud.coef, loud.map.reshape(-1)])).cuda()
    work, zbar = torch.zeros(words, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.float64, device='cuda')
    counts = torch.zeros((n, 4), dtype=torch.int32, device='cuda')
    sumsq, peak = torch.zeros(n, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.float32, device='cuda')
    lib = L.load()

    def loudness():
        L.check(lib.sedt_loudness(L.p(flat), flat.numel(), L.p(d_off), L.p(d_len), n, L.p(consts), L.p(consts[10:]), loud.hop, Z_ABS,
                                  L.p(work), words, L.p(zbar), L.p(counts), L.stream_ptr()), 'loudness')

    def bank_stats():
        L.check(lib.sedt_bank_stats(L.p(flat), flat.numel(), L.p(d_off), L.p(d_len), n, L.p(sumsq), L.p(peak), L.stream_ptr()), 'bank_stats')

    return {'loudness_us': loudness, 'bank_stats_us': bank_stats}, (zbar, counts), int(lens.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    from sound_event_detection_transformer_amd.utilities.loudness import DeviceLoudness
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    gen = np.random.default_rng(1)
    sounds = [(0.1 * gen.standard_normal(int(gen.integers(SR // 2, 4 * SR)))).astype(np.float32) for _ in range(24)]
    bank = sounds + [(0.02 * gen.standard_normal(30 * SR)).astype(np.float32) for _ in range(3)]
    long_bg = [(0.02 * gen.standard_normal(600 * SR)).astype(np.float32)]
    loud = DeviceLoudness(SR)
    res = {'sr': SR, 'calls_per_window': args.calls, 'rounds': args.rounds}
    for name, sources in (('bank', bank), ('ten_minutes', long_bg)):
        fns, (zbar, counts), samples = paths(sources, loud)
        for fn in fns.values():                                    # warm-up: code objects
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        got = {k: [] for k in fns}
        for _ in range(args.rounds):                               # the paths alternate inside every round
            for k, fn in fns.items():
                got[k].append(window_us(fn, args.calls))
        out = {'sources': len(sources), 'samples': samples, 'lufs': [round(float(v), 3) for v in DeviceLoudness.result(zbar, counts).lufs[-3:]]}
        for k, v in got.items():
            out[k] = round(float(np.median(v)), 2)
            out[k.replace('_us', '_spread_us')] = [round(float(min(v)), 2), round(float(max(v)), 2)]
        out['loudness_float64_GFMAps'] = round(2 * 12 * samples / out['loudness_us'] / 1e3, 1)
        res[name] = out
    print(json.dumps(res))


if __name__ == '__main__':
    main()
