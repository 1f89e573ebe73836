"""Float64 NumPy restatement (TEST INFRASTRUCTURE) of what the reference's SedData.load_and_compute_mel_spec
(data_utils/SedData.py:195-217, compute_log=False) gets from librosa, written from the published algorithm - librosa is not installed
where the tests run, and the reference holds only the call:

    librosa.stft(y, n_fft, hop_length=hop, win_length=n_window, window=np.hamming(n_window), center=True, pad_mode='reflect')
    librosa.feature.melspectrogram(S=|stft|, sr, n_mels, fmin=0, fmax=sr/2, htk=False, norm=None).T

1. window: np.hamming(n_window) (symmetric), zero-padded to n_fft centred, (n_fft - n_window) // 2 zeros on the left;
2. y reflect-padded by n_fft // 2 on both sides (np.pad mode='reflect': the edge sample is not repeated);
3. 1 + n // hop frames, frame t = padded samples [t hop, t hop + n_fft);
4. S = |rfft(frame * window)|, n_fft/2 + 1 bins;
5. mel = W @ S, W the Slaney-scale triangles (linear below 1 kHz in steps of 200/3 Hz, logarithmic above with step ln(6.4)/27) between
   n_mels + 2 points equally spaced in mel, weight max(0, min(rising, falling)), no area normalisation;
6. transposed: (T, n_mels).

tests/test_mel_cpu.py checks this file against torch.stft in float64, transformers' mel_filter_bank and a brute-force DFT; the GPU
tests and tests/golden/make_golden_mel.py use it as the reference.  It shares no code with the product's utilities/mel.py."""
import numpy as np

URBAN = dict(sr=44100, n_fft=2048, n_window=1764, hop=882, n_mels=64)        # reference config.py:39-52
DCASE = dict(sr=16000, n_fft=1024, n_window=1024, hop=323, n_mels=64)
CONFIGS = {'urban': URBAN, 'dcase': DCASE}

F_SP = 200.0 / 3.0
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = MIN_LOG_HZ / F_SP            # 15
LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.atleast_1d(np.asarray(f, np.float64))
    m = f / F_SP
    hi = f >= MIN_LOG_HZ
    m[hi] = MIN_LOG_MEL + np.log(f[hi] / MIN_LOG_HZ) / LOGSTEP
    return m


def mel_to_hz(m):
    m = np.atleast_1d(np.asarray(m, np.float64))
    f = F_SP * m
    hi = m >= MIN_LOG_MEL
    f[hi] = MIN_LOG_HZ * np.exp(LOGSTEP * (m[hi] - MIN_LOG_MEL))
    return f


def mel_filterbank(sr, n_fft, n_mels):
    """(n_mels, n_fft/2 + 1) float64"""
    fft_f = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    lo, hi = hz_to_mel(0.0)[0], hz_to_mel(sr / 2.0)[0]
    mel_f = mel_to_hz(np.linspace(lo, hi, n_mels + 2))
    W = np.zeros((n_mels, 1 + n_fft // 2))
    for m in range(n_mels):
        rising = (fft_f - mel_f[m]) / (mel_f[m + 1] - mel_f[m])
        falling = (mel_f[m + 2] - fft_f) / (mel_f[m + 2] - mel_f[m + 1])
        W[m] = np.maximum(0.0, np.minimum(rising, falling))
    return W


def padded_window(n_fft, n_window):
    w = np.zeros(n_fft)
    lpad = (n_fft - n_window) // 2
    w[lpad:lpad + n_window] = np.hamming(n_window)
    return w


def n_frames(n, hop):
    return 1 + n // hop


def stft_magnitude(y, n_fft, n_window, hop):
    """(T, n_fft/2 + 1) float64"""
    y = np.asarray(y, np.float64)
    assert y.ndim == 1 and len(y) >= n_fft // 2 + 1, 'one reflection must be enough'
    yp = np.pad(y, n_fft // 2, mode='reflect')
    w = padded_window(n_fft, n_window)
    T = n_frames(len(y), hop)
    frames = np.stack([yp[t * hop:t * hop + n_fft] for t in range(T)])
    return np.abs(np.fft.rfft(frames * w, axis=1))


def mel_spectrogram(y, sr, n_fft, n_window, hop, n_mels):
    """(T, n_mels) float64 mel amplitudes of the waveform y"""
    return stft_magnitude(y, n_fft, n_window, hop) @ mel_filterbank(sr, n_fft, n_mels).T


def fixture_signal(seed, sr, n):
    """the fixture's seeded clip, f32: a linear chirp 50 Hz -> 0.45 sr at 0.25, a 440 Hz tone at 0.15 and white noise at 0.05 rms - the
    noise floor keeps every mel band within 60 dB of its frame's maximum (tests/test_mel_cpu.py asserts >= 1.6e-3 of it)"""
    t = np.arange(n, dtype=np.float64) / sr
    dur = n / sr
    f0, f1 = 50.0, 0.45 * sr
    y = 0.25 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / dur * t * t)) + 0.15 * np.sin(2 * np.pi * 440.0 * t)
    y += 0.05 * np.random.RandomState(seed).randn(n)
    return y.astype(np.float32)


def pure_tone(n, n_fft, k, amp=0.5):
    """a sinusoid at the centre of FFT bin k, f32"""
    return (amp * np.cos(2 * np.pi * k * np.arange(n, dtype=np.float64) / n_fft + 0.3)).astype(np.float32)
