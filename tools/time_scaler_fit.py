"""The dataset Scaler's fit against the transform launch that reads the same bytes, in ONE process, on one resident tensor of
B = 64 raw clips of 496 x 64 mel amplitudes (8.1 MB):
  (a) sedt_scaler_update: stage 1 (scaler_clip_stats_kernel, a workgroup per clip: dB, clip maximum, floor, band sums) and stage 2
      (scaler_accumulate_kernel, one workgroup adding the 64 clips' [2][64] numbers in order) - reads the raw clips, writes 64 KB;
  (b) sedt_box_transform on the same tensor, apply_log=True, no augmentation, no scaler (box_transform_kernel): reads the same raw
      bytes and additionally writes the 8.1 MB of features - the natural yardstick.
Launch times come from a kernel trace (no counters in the same run):
    timeout 300 rocprofv3 --kernel-trace --stats -d DIR -o fit -- python tools/time_scaler_fit.py
    python tools/time_scaler_fit.py --trace DIR            (or the path of the <host>/fit_results.db below it)
Each variant is WARM + N launches in the order above, so the trace's rows split by position."""
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM, B, T, F = 200, 10, 64, 496, 64


def summarize(path):
    import sqlite3
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, '**', '*_results.db'), recursive=True))
        assert len(found) == 1, found
        path = found[0]
    q = "select name, start, end from kernels where name like '%{}%' order by start"
    db = sqlite3.connect(path)
    us = {k: [(r[2] - r[1]) / 1e3 for r in db.execute(q.format(k)).fetchall()]
          for k in ('scaler_clip_stats_kernel', 'scaler_accumulate_kernel', 'box_transform_kernel')}
    assert all(len(v) == WARM + N for v in us.values()), {k: len(v) for k, v in us.items()}
    s1, s2, bt = (np.asarray(us[k][WARM:]) for k in ('scaler_clip_stats_kernel', 'scaler_accumulate_kernel', 'box_transform_kernel'))
    mb = B * T * F * 4 / 1e6
    print(f'(a) scaler fit, stage 1 (per clip)      : median {np.median(s1):7.2f} us  min {s1.min():7.2f} us  reads {mb:.2f} MB, writes {B * 2 * F * 8 / 1e3:.0f} KB')
    print(f'    scaler fit, stage 2 (accumulate)    : median {np.median(s2):7.2f} us  min {s2.min():7.2f} us')
    print(f'    both kernels of sedt_scaler_update  : median {np.median(s1 + s2):7.2f} us  min {(s1 + s2).min():7.2f} us  (kernel time; the gap between them is not in it)')
    print(f'(b) sedt_box_transform, same raw tensor : median {np.median(bt):7.2f} us  min {bt.min():7.2f} us  reads {mb:.2f} MB, writes {mb:.2f} MB')


def main():
    from sound_event_detection_transformer_amd.utilities.scaler import Scaler
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform, _AUG
    gen = torch.Generator().manual_seed(2000)
    raw = (torch.randn(B, T, F, generator=gen).abs() * 10 ** (torch.rand(B, 1, 1, generator=gen) * 4 - 3)).cuda()
    sc = Scaler(T, apply_log=True)
    for _ in range(WARM + N):
        sc.update(raw)
    sc.finalize()
    torch.cuda.synchronize()
    print('(a)', WARM + N, 'x sedt_scaler_update, count', sc.count_, flush=True)
    tf = DeviceBoxTransform(T, apply_log=True)
    out = torch.empty(B, 1, T, F, device='cuda')
    params = np.zeros((B,), _AUG)
    params['nframes_raw'] = T
    for _ in range(WARM + N):
        tf(raw, params=params, out=out)
    torch.cuda.synchronize()
    v = out[:, 0].double()
    print('(b)', WARM + N, 'x sedt_box_transform; fit mean vs mean of the transform output: max |diff|',
          float((torch.from_numpy(sc.mean_).cuda() - v.mean(dim=(0, 1))).abs().max()), flush=True)


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--trace':
        summarize(sys.argv[2])
    else:
        main()
