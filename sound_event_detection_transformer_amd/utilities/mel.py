"""The log-mel front end on the device, from the waveform to the mel amplitudes - counterpart of the reference's
SedData.load_and_compute_mel_spec (data_utils/SedData.py:195-217) with compute_log=False, the form every driver uses:

    ham_win = np.hamming(n_window)
    spec = librosa.stft(audio, n_fft=n_fft, win_length=n_window, window=ham_win, hop_length=hop_size, center=True, pad_mode='reflect')
    mel_spec = librosa.feature.melspectrogram(S=np.abs(spec), sr=sample_rate, n_mels=n_mels, fmin=0, fmax=sample_rate / 2,
                                               htk=False, norm=None).T

becomes

    mel = DeviceMelSpectrogram.urbansed()          # or .dcase(), or the five numbers of config.py:39-52
    amp, nframes = mel(waves)                      # ONE launch for the batch (sedt_mel_spectrogram); amp stays on the device
    x = DeviceBoxTransform(frames, scaler=scaler)(amp, nframes=nframes)

File decoding (read_audio, SedData.py:361-377) stays on the host; read_audio's down-mix and resampling are utilities/resample.py
(DeviceResampler: its (wave, samples per clip) go as they are into ``mel(wave, lengths=...)``).  The dB step's other home, the
compute_log=True branch no driver takes, is not built (ApplyLog lives in sedt_box_transform).

``mel_tables`` is the host half: the window, the FFT twiddles and the filterbank as a band-wise CSR table, all computed in float64 and
rounded once to f32 - the kernel evaluates no sine and no mel formula.  It needs no GPU."""
import collections

import numpy as np
import torch

from .. import lib as L
from .transforms import PinnedRing

MelTables = collections.namedtuple('MelTables', 'window twiddle band_bin0 band_off band_w')


def frames_of(n_samples, hop):
    """frames of a clip of ``n_samples`` samples: librosa's centred STFT gives 1 + n // hop"""
    return 1 + int(n_samples) // int(hop)


def _hz_to_mel(f):
    """Slaney's scale (librosa htk=False): linear below 1 kHz in steps of 200/3 Hz, logarithmic above with step ln(6.4)/27"""
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(sample_rate, n_fft, n_mels=64):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin=0, fmax=sr/2, htk=False, norm=None) in float64: (n_mels, n_fft/2 + 1) triangles
    between n_mels + 2 points equally spaced in mel, weight max(0, min(rising ramp, falling ramp)), no area normalisation"""
    fft_f = np.linspace(0.0, sample_rate / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sample_rate / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper))


def mel_tables(sample_rate, n_fft, n_window, hop_size, n_mels=64):
    """the kernel's constant tables as NumPy arrays (MelTables):
      window    f32 [n_fft]              np.hamming(n_window) (symmetric, float64) zero-padded to n_fft, centred: (n_fft - n_window) // 2
                                         zeros on the left
      twiddle   f32 [2][n_fft/2 + 1]     cos(2 pi t / n_fft) and -sin(2 pi t / n_fft), float64 rounded to f32
      band_bin0 int32 [n_mels]           first FFT bin with a non-zero weight in band m (0 for an empty band)
      band_off  int32 [n_mels + 1]       band m owns band_w[band_off[m] : band_off[m + 1]], the weights of bins band_bin0[m], + 1, ...
      band_w    f32 [band_off[-1]]       (zeros inside a run, if any, are kept, so a run is contiguous)
    ``hop_size`` does not enter a table; it is checked with the rest of the envelope."""
    if n_fft < 2 or n_fft % 2 or not 1 <= n_window <= n_fft or hop_size < 1 or n_mels < 1:
        raise ValueError(f'mel_tables: n_fft={n_fft} n_window={n_window} hop_size={hop_size} n_mels={n_mels}')
    lpad = (n_fft - n_window) // 2
    window = np.zeros(n_fft, np.float64)
    window[lpad:lpad + n_window] = np.hamming(n_window)
    ang = 2.0 * np.pi * np.arange(n_fft // 2 + 1, dtype=np.float64) / n_fft
    twiddle = np.stack([np.cos(ang), -np.sin(ang)])
    W = mel_filterbank(sample_rate, n_fft, n_mels)
    bin0, off, ws = np.zeros(n_mels, np.int32), np.zeros(n_mels + 1, np.int32), []
    for m in range(n_mels):
        nz = np.flatnonzero(W[m].astype(np.float32))
        if len(nz):
            bin0[m] = nz[0]
            ws.append(W[m, nz[0]:nz[-1] + 1])
        off[m + 1] = off[m] + (nz[-1] + 1 - nz[0] if len(nz) else 0)
    band_w = np.concatenate(ws) if ws else np.zeros(0)
    return MelTables(window.astype(np.float32), twiddle.astype(np.float32), bin0, off, band_w.astype(np.float32))


def expand_filterbank(tables, n_fft):
    """the dense (n_mels, n_fft/2 + 1) f32 matrix a MelTables CSR stands for"""
    n_mels = len(tables.band_bin0)
    W = np.zeros((n_mels, n_fft // 2 + 1), np.float32)
    for m in range(n_mels):
        n = tables.band_off[m + 1] - tables.band_off[m]
        W[m, tables.band_bin0[m]:tables.band_bin0[m] + n] = tables.band_w[tables.band_off[m]:tables.band_off[m + 1]]
    return W


class DeviceMelSpectrogram(object):
    """sample_rate, n_fft, n_window, hop_size, n_mels: the reference's config values (config.py:39-52).  The tables go to the device
    once, here; a call is one launch and reads nothing back."""

    def __init__(self, sample_rate, n_fft, n_window, hop_size, n_mels=64, device='cuda'):
        self.sr, self.n_fft, self.n_window, self.hop, self.F = int(sample_rate), int(n_fft), int(n_window), int(hop_size), int(n_mels)
        self.dev = torch.device(device)
        lib = L.load()
        if not lib.sedt_mel_ok(self.n_fft, self.n_window, self.hop, self.F):
            # the entry point refuses before it looks at a pointer: its message is the one a caller sees for a bad geometry
            L.check(lib.sedt_mel_spectrogram(None, L.F32, 1, None, 0, None, 1, None, None, None, None, None, 0, self.n_fft, self.n_window,
                                             self.hop, self.F, None), 'mel_spectrogram')
            raise RuntimeError('mel_spectrogram: sedt_mel_ok and sedt_mel_spectrogram disagree on the envelope')
        self.tables = mel_tables(self.sr, self.n_fft, self.n_window, self.hop, self.F)
        self._dev_tables = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in self.tables)
        self._ring, self._const = None, {}

    @classmethod
    def urbansed(cls, **kw):
        return cls(44100, 2048, 1764, 882, 64, **kw)

    @classmethod
    def dcase(cls, **kw):
        return cls(16000, 1024, 1024, 323, 64, **kw)

    @property
    def min_samples(self):
        """the shortest clip a single reflection can pad: n_fft/2 + 1 samples"""
        return self.n_fft // 2 + 1

    def stage(self, waves, staging=None):
        """a batch of waveforms on the device: ``waves`` is a (B, N) float32 / int16 tensor already there, or a list of ragged 1-D
        float32 / int16 arrays / tensors, which go through a pinned buffer (``staging``: a pinned (B, >= longest) tensor of the
        clips' dtype, or a fresh one).  Returns (wave (B, stride) on the device, samples per clip)."""
        if torch.is_tensor(waves) and waves.is_cuda:
            if waves.dim() != 2:
                raise ValueError(f'a (B, N) batch of waveforms expected, got shape {tuple(waves.shape)}')
            if waves.dtype != torch.int16:
                waves = waves.float()
            return waves.contiguous(), [waves.shape[1]] * waves.shape[0]
        if torch.is_tensor(waves) or isinstance(waves, np.ndarray):
            waves = list(waves)                                   # a host (B, N) block: its clips
        clips = [c.numpy() if torch.is_tensor(c) else np.asarray(c) for c in waves]
        if not clips:
            return torch.empty((0, 1), dtype=torch.float32, device=self.dev), []
        if any(c.ndim != 1 for c in clips):
            raise ValueError('mono waveforms expected: every clip 1-D (utilities.resample.DeviceResampler down-mixes on the device)')
        pcm = len(clips) > 0 and all(c.dtype == np.int16 for c in clips)
        ns = [int(c.shape[0]) for c in clips]
        B, stride = len(clips), max(ns, default=1)
        host = staging if staging is not None else torch.zeros((B, stride), dtype=torch.int16 if pcm else torch.float32).pin_memory()
        hv = host.numpy()
        for i, c in enumerate(clips):                             # plain memcpys into the pinned buffer (samples >= ns[i] are never read)
            hv[i, :ns[i]] = c
        return host.to(self.dev, non_blocking=True), ns

    def __call__(self, waves, lengths=None, out=None, staging=None):
        """waves, staging: see stage().  lengths: samples per clip (else the clips' own lengths; every clip of a device tensor counts
        as N samples long).  out: optional (B, rows, n_mels) f32 device tensor, rows >= 1 - frames past ``rows`` are dropped, rows past
        a clip's frames are zeroed.  Returns (mel (B, rows, n_mels) f32 on the device, frames per clip): rows = the longest clip's
        frames unless ``out`` says otherwise."""
        wave, ns = self.stage(waves, staging)
        B, stride = wave.shape[0], wave.shape[1]
        if lengths is not None:
            ns = [int(n) for n in lengths]
        if len(ns) != B or (B and max(ns) > stride):
            raise ValueError('lengths: one sample count per clip, within the samples of the batch')
        if B and min(ns) < self.min_samples:
            raise ValueError(f'mel_spectrogram: a clip of {min(ns)} samples is shorter than n_fft/2 + 1 = {self.min_samples}: '
                             'the reflect padding would have to wrap twice')
        nframes = [frames_of(n, self.hop) for n in ns]
        if out is None:
            out = torch.empty((B, max(nframes, default=1), self.F), device=self.dev, dtype=torch.float32)
        if out.dim() != 3 or out.shape[0] != B or out.shape[2] != self.F or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f'out: a contiguous ({B}, rows, {self.F}) f32 tensor expected, got {tuple(out.shape)} {out.dtype}')
        if B == 0:
            return out, nframes
        if lengths is None and torch.is_tensor(waves) and waves.is_cuda:
            # equal lengths known without the host: a constant device vector, made once per (B, N) - nothing is uploaded per call, so
            # a captured call replays from device memory alone
            nd = self._const.get((B, stride))
            if nd is None:
                nd = self._const[(B, stride)] = torch.full((B,), stride, dtype=torch.int32, device=self.dev)
        else:
            if self._ring is None:
                self._ring = PinnedRing(self.dev)
            nd = self._ring.upload(np.asarray(ns, np.int32).view(np.uint8))
        win, tw, bin0, off, bw = self._dev_tables
        L.check(L.load().sedt_mel_spectrogram(L.p(wave), L.I16 if wave.dtype == torch.int16 else L.F32, stride, L.p(nd), B, L.p(out),
                                              out.shape[1], L.p(win), L.p(tw), L.p(bin0), L.p(off), L.p(bw), bw.numel(), self.n_fft,
                                              self.n_window, self.hop, self.F, L.stream_ptr()), 'mel_spectrogram')
        return out, [min(n, out.shape[1]) for n in nframes]

    def features(self, waves):
        """a list of (T_i, n_mels) float32 NumPy arrays, one per clip: what the reference np.save()s into its feature cache, so a
        cache written from here loads in the reference's DataLoadDf unchanged.  (One read-back of the batch.)"""
        mel, nframes = self(waves)
        host = mel.cpu().numpy()
        return [host[i, :n].copy() for i, n in enumerate(nframes)]
