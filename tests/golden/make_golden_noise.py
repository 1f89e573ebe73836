#!/usr/bin/env python3
"""Generate tests/golden/g19_noise_views.npz by running the REFERENCE's own transform objects (utilities/BoxTransforms.py) through
``Transform.__call__`` on ``(clip, label)`` samples, in the order get_transforms composes the noisy chain of the semi-supervised
recipe (:454-490 with noise_dict_params): AugmentGaussianNoise(mean=0., snr=30) -> [ApplyLog] -> PadOrTrunc -> TimeMask ->
FreqMask(fill_mode="mean") -> FreqShift -> ToTensor(unsqueeze_axis=0) -> Normalize(scaler).  The tuple handling (the pair that
AugmentGaussianNoise returns, TimeMask skipping member 0) and the order of the np.random draws are therefore the reference's.

ApplyLog is librosa (not installed where the fixtures are made; same exclusion as G13), so the inputs are dB-like values.  In its
position stands ``FreshCopy`` below, because ApplyLog has one side effect the chain depends on: it returns a fresh array per member.
Without it a clip whose noise is NOT applied is the same array twice (``return data, data``), a clip longer than ``frames`` stays a
slice view of it through pad_trunc_seq, and view 1's in-place masks would also land in view 0 - which cannot happen in the recipe.
FreshCopy also keeps what each member looked like when it passed, so the generator can check its own statement of the noise
(clip + std * z, z the standard normals np.random.seed(s) regenerates) against what the reference computed.

librosa, PIL and torchvision.transforms are placeholder modules; nothing computed here comes from them.  The probabilities are
raised to 0.6 as in G13 so that few clips exercise every branch.  The normals are not stored (legacy RandomState streams are
frozen): only the first eight of each noisy clip, as a guard.

usage:  python tests/golden/make_golden_noise.py --reference <reference checkout>
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES, F, SNR, P = 128, 64, 30, 0.6
SEEDS = [1000, 1001, 1002, 1003, 1004, 1005]
NRAW = [120, 150, 120, 150, 120, 150]                # shorter / longer than FRAMES


class _Absent(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        return type(k, (), {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference repository')
    ref = ap.parse_args().reference
    for name in ('librosa', 'PIL', 'torchvision', 'torchvision.transforms'):
        if name not in sys.modules:
            sys.modules[name] = _Absent(name)
    sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
    sys.path.insert(0, ref)
    import utilities.BoxTransforms as rbt
    import utilities.Scaler as rscaler

    class FreshCopy(rbt.Transform):
        def transform_data(self, data):
            self.seen.append(data.copy())
            return data.copy()

    def logged(obj):
        """keep every draw of a transform object (its ``parameters`` dict holds only the last member's)"""
        obj.log, orig = [], obj.randomize_parameters

        def randomize():
            orig()
            obj.log.append(dict(obj.parameters))
        obj.randomize_parameters = randomize
        return obj

    rng = np.random.RandomState(191)
    sc = rscaler.Scaler()
    mean = rng.randn(F) * 3 - 40
    sc.load_state_dict({'mean_': mean.tolist(), 'mean_of_square_': (mean ** 2 + rng.rand(F) * 100 + 60).tolist()})
    res = {'frames': np.int64(FRAMES), 'snr': np.float64(SNR), 'p': np.float64(P), 'seeds': np.asarray(SEEDS), 'nraw': np.asarray(NRAW),
           'scaler_mean': sc.mean_.astype(np.float64), 'scaler_std': sc.std_.astype(np.float64)}
    params, guard = [], []
    for i, (seed, n) in enumerate(zip(SEEDS, NRAW)):
        clip = (rng.randn(n, F) * 12 - 40).astype(np.float32)
        if i == 2:
            clip[:, 7] = 0.0                                     # a band of zeros: std 0, no noise there
        res[f'in{i}'] = clip
        fresh = FreshCopy()
        fresh.seen = []
        tm, fm, fs = logged(rbt.TimeMask(p=P)), logged(rbt.FreqMask(fill_mode="mean", p=P)), logged(rbt.FreqShift(p=P))
        chain = [rbt.AugmentGaussianNoise(mean=0., snr=SNR, p=P), fresh, rbt.PadOrTrunc(nb_frames=FRAMES), tm, fm, fs,
                 rbt.ToTensor(unsqueeze_axis=0), rbt.Normalize(sc)]
        label = {'labels': np.zeros(1, np.int64), 'boxes': np.asarray([[0.5, 0.2]]), 'orig_size': np.asarray(10.0)}
        np.random.seed(seed)
        sample = (clip.copy(), label)
        for tr in chain:
            sample = tr(sample)
        (v0, v1), _ = sample
        res[f'out{i}_v0'], res[f'out{i}_v1'] = v0.numpy().astype(np.float32), v1.numpy().astype(np.float32)
        assert len(tm.log) == 1 and len(fm.log) == 2 and len(fs.log) == 2          # TimeMask skips member 0
        # ---- the generator's own statement of the noise, checked against what the reference handed on
        np.random.seed(seed)
        on = np.random.uniform(0, 1) < P
        g8 = np.zeros(8)
        if on:
            z = np.random.normal(0.0, 1.0, clip.shape)
            std = np.sqrt(np.mean((clip ** 2) * (10 ** (-SNR / 10)), axis=-2))
            assert std.dtype == np.float32
            assert np.array_equal(fresh.seen[1], clip + std * z), np.abs(fresh.seen[1] - (clip + std * z)).max()
            g8 = z.reshape(-1)[:8].copy()
        else:
            assert np.array_equal(fresh.seen[1], clip)
        assert np.array_equal(fresh.seen[0], clip)
        guard.append(g8)
        row = [float(on), float(tm.log[0]['apply']), tm.log[0]['t'], tm.log[0]['t0']]
        for k in (0, 1):
            row += [float(fm.log[k]['apply']), fm.log[k]['f'], fm.log[k]['f0']]
        for k in (0, 1):
            row += [float(fs.log[k]['apply']), float(fs.log[k]['shift_size'])]
        params.append(row)
    # columns: noise_on | tm1 apply, t, t0 | fm0 apply, f, f0 | fm1 apply, f, f0 | fs0 apply, shift | fs1 apply, shift
    res['params'] = np.asarray(params, np.float64)
    res['normals_head'] = np.asarray(guard, np.float64)
    on, long_ = res['params'][:, 0] > 0, np.asarray(NRAW) > FRAMES
    assert (on & long_).any() and (on & ~long_).any() and (~on & long_).any() and (~on & ~long_).any()
    np.savez_compressed(os.path.join(HERE, 'g19_noise_views.npz'), **res)
    print('G19 ok', res['params'][:, [0, 1, 4, 7, 10, 12]].tolist())


if __name__ == '__main__':
    main()
