#!/usr/bin/env python3
"""Generate tests/golden/g21_mel.npz: the float64 mel amplitudes tests/mel_ref.py computes for one seeded clip per configuration
(URBAN-SED 44100 / 2048 / 1764 / 882 and DCASE 16000 / 1024 / 1024 / 323, 64 bands).  The inputs are not stored: mel_ref.fixture_signal
regenerates them from the seed (a chirp, a 440 Hz tone and white noise at 0.05 rms, sr + 37 samples, rounded to f32).

librosa - what the reference calls - is not installed where the fixtures are made, so nothing here runs the reference; mel_ref is
the restatement of librosa's published algorithm, and tests/test_mel_cpu.py holds it against torch.stft (float64), transformers'
mel_filter_bank and a brute-force DFT.  The fixture pins that restatement: a later edit of mel_ref.py that moves a number shows up.

usage:  python tests/golden/make_golden_mel.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mel_ref as R  # noqa: E402

SEEDS = {'urban': 2101, 'dcase': 2102}


def main():
    res = {}
    for name, cfg in R.CONFIGS.items():
        n = cfg['sr'] + 37
        y = R.fixture_signal(SEEDS[name], cfg['sr'], n)
        mel = R.mel_spectrogram(y, **cfg)
        assert mel.dtype == np.float64 and mel.shape == (R.n_frames(n, cfg['hop']), cfg['n_mels'])
        res[f'{name}_seed'], res[f'{name}_n'], res[f'{name}_mel'] = np.int64(SEEDS[name]), np.int64(n), mel
        res[f'{name}_wave_sum'] = np.float64(y.astype(np.float64).sum())           # guards the regenerated input
        print(name, mel.shape, 'smallest band / frame maximum', (mel.min(axis=1) / mel.max(axis=1)).min())
    path = os.path.join(HERE, 'g21_mel.npz')
    np.savez_compressed(path, **res)
    print('G21 ok', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
