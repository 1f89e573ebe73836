"""The input side of the C5 step (B = 64 clips of 496 x 64) two ways, in ONE process:
  (a) what bench.py's C5 leg runs: two sedt_box_transform launches from two resident raw tensors (teacher: FreqMask; student, whose raw
      copy carries noise baked in on the host: TimeMask + FreqMask) - utilities.synthetic.semi_view_transforms;
  (b) the paired launch sedt_box_transform_views from ONE resident raw tensor, the student's noise drawn in the kernel
      (utilities.synthetic.semi_pair_transform, noise on a clip with probability 0.5 as in the recipe);
and, to see where (b)'s time goes, the paired launch with (c) the noise off on every clip (two views, no band sums, no normals),
(d) drawn on every clip, (e) injected on every clip (band sums and a second operand, no hash and no transcendentals).
Launch times come from a kernel trace (no counters in the same run):
    timeout 300 rocprofv3 --kernel-trace --stats -d DIR -o views -- python tools/time_noise_views.py
    python tools/time_noise_views.py --trace DIR/<host>/views_results.db
Each variant is WARM + N iterations in the order above, so the trace's rows split by position; the same np.random seed precedes every
variant, so (b)-(e) mask the same rows and bands."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM, B, T, F = 200, 10, 64, 496, 64
PAIRED = ['(b) paired, drawn, p = 0.5', '(c) paired, noise off', '(d) paired, drawn, every clip', '(e) paired, injected, every clip']


def summarize(path):
    import sqlite3
    q = "select name, start, end from kernels where name like '%{}%' order by start"
    db = sqlite3.connect(path)
    one = [(r[2] - r[1]) / 1e3 for r in db.execute(q.format('box_transform_kernel')).fetchall()]
    two = [(r[2] - r[1]) / 1e3 for r in db.execute(q.format('box_transform_views_kernel')).fetchall()]
    assert len(one) == 2 * (WARM + N) and len(two) == len(PAIRED) * (WARM + N), (len(one), len(two))
    t, s = np.asarray(one[2 * WARM:]).reshape(N, 2)[:, 0], np.asarray(one[2 * WARM:]).reshape(N, 2)[:, 1]
    print(f'(a) two single-view launches      : median {np.median(t + s):7.2f} us (teacher {np.median(t):.2f} + student {np.median(s):.2f})  '
          f'min {np.min(t + s):7.2f} us  2 launches, {2 * B * T * F * 4 / 1e6:.2f} MB of raw clips per batch')
    for k, name in enumerate(PAIRED):
        v = two[k * (WARM + N) + WARM:(k + 1) * (WARM + N)]
        print(f'{name:34s}: median {np.median(v):7.2f} us  min {min(v):7.2f} us  1 launch, {B * T * F * 4 / 1e6:.2f} MB of raw clips per batch')


def main():
    from sound_event_detection_transformer_amd.utilities.synthetic import synthetic_semi_raw, semi_view_transforms, semi_pair_transform
    raw_t, raw_s = (r.cuda() for r in synthetic_semi_raw(32, 32, T, 1900))
    tf_t, tf_s = semi_view_transforms(T, 'cuda')
    out = [torch.empty(B, 1, T, F, device='cuda') for _ in range(2)]
    np.random.seed(1)
    for _ in range(WARM + N):
        tf_t(raw_t, out=out[0])
        tf_s(raw_s, out=out[1])
    torch.cuda.synchronize()
    print('(a)', WARM + N, 'x 2 launches', flush=True)
    z = torch.randn(B, T, F, generator=torch.Generator().manual_seed(2)).cuda()
    for name, p, inject in zip(PAIRED, (0.5, 0.0, 1.0, 1.0), (False, False, False, True)):
        tf = semi_pair_transform(T, 'cuda', seed=3)
        tf.noise_p = p
        np.random.seed(1)
        for _ in range(WARM + N):
            recs, _ = tf.draw_batch([T] * B)
            tf(raw_t, params=recs, out=out, normals=z if inject else None)
        torch.cuda.synchronize()
        print(name, WARM + N, 'launches', flush=True)


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--trace':
        summarize(sys.argv[2])
    else:
        main()
