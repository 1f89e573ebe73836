#!/usr/bin/env python3
"""Generate tests/golden/g20_scaler.npz by running the REFERENCE's own ``utilities.Scaler.Scaler`` over clips that went through its own
transform objects, in the order get_transforms(frames) composes the chain the drivers fit the scaler on (train_sedt.py:169-190):
[ApplyLog] -> PadOrTrunc -> ToTensor(unsqueeze_axis=0); then its ``Normalize(scaler)`` on two of the clips.

ApplyLog is librosa (not installed where the fixtures are made; same exclusion as G13 / G19), so the inputs are dB-like f32 values and
the device fit is compared with apply_log=False.  librosa, PIL and torchvision.transforms are placeholder modules; nothing computed
here comes from them.

Eight ragged clips around frames = 128, F = 64: shorter (padded), longer (truncated) and one of exactly 128 rows.  Two bands are special
in every clip:
  band 7   all zeros: mean, mean of squares and variance are exactly 0, std_ = 0, and Normalize gives 0 / 0 = NaN there;
  band 11  the constant -40 on the real rows: every per-clip sum is a sum of integers, exact in float64 in any order, so the stored
           statistics of this band are reproduced bit for bit by any correct fit.

Stored: the inputs, mean_ / mean_of_square_ / std_ from calculate_scaler, the text Scaler.save wrote (data, not code), the Normalize
output of clips 0 (short) and 3 (long).

usage:  python tests/golden/make_golden_scaler.py --reference <reference checkout>
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES, F = 128, 64
NRAW = [120, 150, 128, 141, 97, 133, 64, 200]          # shorter / longer than FRAMES, one exactly FRAMES
NORMALIZED = [0, 3]                                    # a padded and a truncated clip
ZERO_BAND, CONST_BAND, CONST = 7, 11, -40.0


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

    rng = np.random.RandomState(201)
    band_level, band_spread = rng.randn(F) * 6 - 40, rng.rand(F) * 10 + 4
    chain = [rbt.PadOrTrunc(nb_frames=FRAMES), rbt.ToTensor(unsqueeze_axis=0)]

    def label():
        return {'labels': np.zeros(1, np.int64), 'boxes': np.asarray([[0.5, 0.2]]), 'orig_size': np.asarray(10.0)}

    res = {'frames': np.int64(FRAMES), 'nraw': np.asarray(NRAW), 'normalized': np.asarray(NORMALIZED),
           'zero_band': np.int64(ZERO_BAND), 'const_band': np.int64(CONST_BAND)}
    dataset = []
    for i, n in enumerate(NRAW):
        clip = (rng.randn(n, F) * band_spread + band_level).astype(np.float32)
        clip[:, ZERO_BAND] = 0.0
        clip[:, CONST_BAND] = CONST
        res[f'in{i}'] = clip
        sample = (clip.copy(), label())
        for tr in chain:
            sample = tr(sample)
        assert tuple(sample[0].shape) == (1, FRAMES, F)
        dataset.append(sample)
    sc = rscaler.Scaler()
    mean, std = sc.calculate_scaler(dataset)
    assert mean.dtype == np.float64 and mean.shape == (F,) and std is sc.std_
    res['mean_'], res['mean_of_square_'], res['std_'] = sc.mean_.copy(), sc.mean_of_square_.copy(), sc.std_.copy()
    assert sc.std_[ZERO_BAND] == 0.0 and np.isfinite(sc.std_).all() and (np.delete(sc.std_, ZERO_BAND) > 0).all()
    with tempfile.TemporaryDirectory() as d:
        sc.save(os.path.join(d, 'scaler.json'))
        with open(os.path.join(d, 'scaler.json')) as f:
            res['json'] = np.asarray(f.read())
    norm = rbt.Normalize(sc)
    with np.errstate(invalid='ignore'):
        for i in NORMALIZED:
            sample = (res[f'in{i}'].copy(), label())
            for tr in chain + [norm]:
                sample = tr(sample)
            res[f'norm{i}'] = sample[0].numpy().astype(np.float32)
            assert np.isnan(res[f'norm{i}'][..., ZERO_BAND]).all() and np.isfinite(np.delete(res[f'norm{i}'], ZERO_BAND, -1)).all()
    np.savez_compressed(os.path.join(HERE, 'g20_scaler.npz'), **res)
    print('G20 ok', os.path.getsize(os.path.join(HERE, 'g20_scaler.npz')), 'bytes; mean[:3]', sc.mean_[:3], 'std[:3]', sc.std_[:3])


if __name__ == '__main__':
    main()
