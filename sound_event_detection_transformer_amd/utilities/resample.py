"""Sample-rate conversion and down-mix on the device, before the mel stage - the numeric half of the reference's read_audio
(data_utils/SedData.py:361-379: np.mean(audio, axis=1), then librosa.resample); file decoding stays on the host.

    rs = DeviceResampler(48000, 16000)                   # the table goes to the device once
    wave, ns = rs([stereo_pcm, mono_f32])                # ONE launch (sedt_resample); (B, stride) f32 on the device, samples per clip
    amp, nframes = mel(wave, lengths=ns)

Definition (this module's own; tests/resample_ref.py restates it in float64).  The method is band-limited interpolation with a
Kaiser-windowed sinc, the method of resampy's kaiser_best / kaiser_fast:

    L / M = target_sr / orig_sr in lowest terms,  s = min(1, L / M)
    quality (Z, rolloff, beta):  kaiser_best = (64, 0.9475937167399596, 14.769656459379492)
                                 kaiser_fast = (16, 0.85,               8.555504641634386)
    w(u) = rolloff sinc(rolloff u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta)  for |u| <= Z, 0 outside;  sinc(x) = sin(pi x) / (pi x)
    m[j] = the mean over the channels of frame j of an interleaved (frames, channels) input; int16 PCM is worth x / 32768
    y[n] = sum_j s w(s (n M / L - j)) m[j]  over 0 <= j < N (the recording is zero outside its samples: no reflection),
    n = 0 .. n_out - 1,  n_out = ceil(N L / M) in integers.  Every such n has n M / L < N: no output is a padded zero.

Polyphase form: i = (n M) div L, p = (n M) mod L, taps k = -H .. H + 1 with H = floor(Z / s), and the table
T[p][k] = s w(s (p / L - k)) - L rows of 2 H + 2 taps, computed in float64 here and rounded once to f32.  The kernel evaluates no
Bessel function and no sine; it sums y[n] = sum_k T[p][k] m[i + k] in f32, k ascending.  orig_sr == target_sr is the identity plan:
one tap of weight 1, so the launch only widens and down-mixes and a mono f32 input comes out bit for bit.

What this is not.  It restates the method, not a package, and claims parity with none:
  * the filter is evaluated exactly at every phase; resampy interpolates linearly in a table of 512 points per zero crossing;
  * librosa >= 0.10 resamples with soxr by default, another filter altogether;
  * n_out is librosa's length, but librosa's fix_length may append a padded zero where resampy's own length is one shorter; here
    every output is an interpolated sample;
  * the ends are the zero-extended recording's, as resampy's, not reflected.

``resample_plan`` and ``resample_table`` are the host half and need no GPU."""
import collections
import math

import numpy as np
import torch

from .. import lib as L_
from .transforms import PinnedRing

QUALITIES = {'kaiser_best': (64, 0.9475937167399596, 14.769656459379492),
             'kaiser_fast': (16, 0.85, 8.555504641634386)}
MAX_CHANNELS = 64
MAX_FRAMES = 1 << 40

ResamplePlan = collections.namedtuple('ResamplePlan', 'orig_sr target_sr quality L M s Z rolloff beta H taps')


def resample_plan(orig_sr, target_sr, quality='kaiser_best'):
    """the integers of a conversion (ResamplePlan); the identity (orig_sr == target_sr) has H = 0 and one tap.  Rates are positive
    integers; a plan the kernel's envelope does not hold (sedt_resample_ok: L, M <= 4096, taps <= 8192, table <= 16 MiB, a
    workgroup's input span <= 16384 floats) is refused here"""
    if isinstance(orig_sr, bool) or isinstance(target_sr, bool) or int(orig_sr) != orig_sr or int(target_sr) != target_sr or \
            orig_sr <= 0 or target_sr <= 0:
        raise ValueError(f'resample_plan: sample rates are positive integers, got {orig_sr!r} -> {target_sr!r}')
    if quality not in QUALITIES:
        raise ValueError(f'resample_plan: quality {quality!r} is none of {sorted(QUALITIES)}')
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    g = math.gcd(orig_sr, target_sr)
    L, M = target_sr // g, orig_sr // g
    Z, rolloff, beta = QUALITIES[quality]
    if L == M:
        plan = ResamplePlan(orig_sr, target_sr, quality, 1, 1, 1.0, Z, rolloff, beta, 0, 1)
    else:
        H = (Z * M) // L if L < M else Z                   # floor(Z / s), s = min(1, L / M), in integers
        plan = ResamplePlan(orig_sr, target_sr, quality, L, M, min(1.0, L / M), Z, rolloff, beta, H, 2 * H + 2)
    if not (plan.L < 2 ** 31 and plan.M < 2 ** 31 and plan.taps < 2 ** 31 and
            L_.load().sedt_resample_ok(plan.L, plan.M, plan.taps, plan.H, 1, 1)):
        raise ValueError(f'resample_plan: {orig_sr} -> {target_sr} ({quality}) is L = {plan.L}, M = {plan.M}, {plan.taps} taps: outside '
                         'the kernel\'s envelope (L, M <= 4096; taps <= 8192; table L * taps * 4 <= 16 MiB; '
                         f'ceil({L_.RESAMPLE_BLK} M / L) + taps + 1 <= 16384)')
    return plan


def resampled_length(n, plan):
    """ceil(n L / M) in integers"""
    return -(-int(n) * plan.L // plan.M)


def kaiser_sinc(u, Z, rolloff, beta):
    """w(u) in float64"""
    u = np.asarray(u, np.float64)
    inside = np.abs(u) <= Z
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (u / Z) ** 2, 0.0, None))) / np.i0(beta)
    return np.where(inside, rolloff * np.sinc(rolloff * u) * win, 0.0)


def resample_table(plan):
    """T f32 [L][taps]: T[p][k + H] = s w(s (p / L - k)), k = -H .. taps - 1 - H, float64 rounded once; {{1}} for the identity"""
    if plan.L == plan.M:
        return np.ones((1, 1), np.float32)
    p = np.arange(plan.L, dtype=np.float64)[:, None]
    k = np.arange(-plan.H, plan.taps - plan.H, dtype=np.float64)[None, :]
    u = plan.s * ((p - k * plan.L) / plan.L)               # p - k L is an exact integer: one rounding in the quotient
    return (plan.s * kaiser_sinc(u, plan.Z, plan.rolloff, plan.beta)).astype(np.float32)


def device_table(table, plan):
    """the layout the kernel reads: f32 [taps][L], column r = n mod L holding row p = (r M) mod L of ``table``"""
    rows = (np.arange(plan.L, dtype=np.int64) * plan.M) % plan.L
    return np.ascontiguousarray(table[rows].T)


class DeviceResampler(object):
    """orig_sr -> target_sr at ``quality``.  A call is one launch and reads nothing back."""

    def __init__(self, orig_sr, target_sr, quality='kaiser_best', device='cuda'):
        self.plan = resample_plan(orig_sr, target_sr, quality)
        self.dev = torch.device(device)
        self.table = resample_table(self.plan)
        self._dev_table = torch.from_numpy(device_table(self.table, self.plan)).to(self.dev)
        self._ring = PinnedRing(self.dev)

    def n_out(self, n):
        return resampled_length(n, self.plan)

    # ------------------------------------------------------------------ input forms
    def stage(self, waves, lengths=None):
        """the clips as device tensors: ``waves`` is a (B, N) float32 / int16 tensor on the device (mono clips), or a list of 1-D
        or (N, C) interleaved float32 / int16 arrays / tensors, host or device (a host (B, N) block counts as its clips).  Returns
        [(tensor, frames, channels)] and the pinned host tensors the copies read (to be kept until they have run)."""
        if torch.is_tensor(waves) and waves.is_cuda:
            if waves.dim() != 2:
                raise ValueError(f'a (B, N) batch of waveforms expected, got shape {tuple(waves.shape)}')
            if waves.dtype != torch.int16:
                waves = waves.float()
            waves = list(waves.contiguous())
        elif torch.is_tensor(waves) or isinstance(waves, np.ndarray):
            waves = list(waves)
        clips, pins = [], []
        if lengths is not None and len(lengths) != len(waves):
            raise ValueError('lengths: one frame count per clip')
        for i, w in enumerate(waves):
            if not torch.is_tensor(w):
                w = torch.from_numpy(np.ascontiguousarray(w))
            if w.dtype not in (torch.float32, torch.int16):
                raise ValueError(f'waveforms are float32 or int16, got {w.dtype}')
            if w.dim() not in (1, 2) or w.shape[0] < 1 or (w.dim() == 2 and not 1 <= w.shape[1] <= MAX_CHANNELS):
                raise ValueError(f'clip {i}: a 1-D waveform or interleaved (frames, channels <= {MAX_CHANNELS}) expected, at least one '
                                 f'frame; got shape {tuple(w.shape)}')
            if not w.is_cuda:
                pin = w.contiguous().pin_memory()
                pins.append(pin)
                w = pin.to(self.dev, non_blocking=True)
            w = w.contiguous()
            n = int(w.shape[0])
            if lengths is not None:
                if not 1 <= int(lengths[i]) <= n:
                    raise ValueError('lengths: one frame count per clip, within the frames of the clip')
                n = int(lengths[i])
            if n > MAX_FRAMES:
                raise ValueError(f'clip {i}: {n} frames, the kernel takes 2^40')
            clips.append((w, n, 1 if w.dim() == 1 else int(w.shape[1])))
        return clips, pins

    def launch(self, clips, dst, offsets, caps):
        """ONE launch: clip i of ``clips`` ((tensor, frames, channels) on the device) resampled into the flat f32 device tensor
        ``dst`` at element offsets[i], caps[i] floats wide (samples past the clip's n_out are written as 0).  No intermediate copy."""
        if clips:
            self._run(self._ring.upload(self._descriptor(clips, dst, offsets, caps).view(np.uint8).reshape(-1)), clips, caps)

    def prepare(self, clips, dst, offsets, caps):
        """launch() with the descriptor uploaded now, into device memory of its own: the returned callable issues the launch and
        nothing else, so it can be captured into a graph and replayed after the source tensors have been refilled"""
        d = torch.from_numpy(self._descriptor(clips, dst, offsets, caps)).to(self.dev)
        return lambda: self._run(d, clips, caps)

    def _descriptor(self, clips, dst, offsets, caps):
        if dst.dtype != torch.float32 or not dst.is_contiguous() or not dst.is_cuda:
            raise ValueError('launch: dst is a contiguous f32 device tensor')
        desc = np.zeros((len(clips), L_.RESAMPLE_DESC_WORDS), np.int64)
        for i, (w, n, c) in enumerate(clips):
            off, cap = int(offsets[i]), int(caps[i])
            if off < 0 or cap < 1 or off + cap > dst.numel() or n < 1 or n * c > w.numel() or not w.is_cuda or not w.is_contiguous():
                raise ValueError(f'launch: clip {i} ({n} frames x {c}) or its destination [{off}, {off + cap}) does not fit its tensor')
            desc[i] = (w.data_ptr(), dst.data_ptr() + 4 * off, n, cap, c, L_.I16 if w.dtype == torch.int16 else L_.F32)
        return desc

    def _run(self, d, clips, caps):
        p = self.plan
        L_.check(L_.load().sedt_resample(L_.p(d), len(clips), max(int(c) for c in caps), L_.p(self._dev_table), p.L, p.M, p.taps, p.H,
                                         max(c for _, _, c in clips), max(n for _, n, _ in clips), L_.stream_ptr()), 'resample')

    def __call__(self, waves, lengths=None, out=None):
        """waves: see stage().  lengths: frames per clip (else the clips' own).  out: optional contiguous (B, stride) f32 device
        tensor, stride >= the longest result.  Returns (wave (B, stride) f32 on the device, samples per clip); samples past a clip's
        n_out are 0.  The raw input is kept alive until the next call."""
        clips, pins = self.stage(waves, lengths)
        B = len(clips)
        ns = [self.n_out(n) for _, n, _ in clips]
        if out is None:
            out = torch.empty((B, max(ns, default=1)), device=self.dev, dtype=torch.float32)
        if out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or not out.is_contiguous() or (B and out.shape[1] < max(ns)):
            raise ValueError(f'out: a contiguous ({B}, >= {max(ns, default=1)}) f32 tensor expected, got {tuple(out.shape)} {out.dtype}')
        stride = out.shape[1]
        self.launch(clips, out.view(-1), [i * stride for i in range(B)], [stride] * B)
        self._keep = (clips, pins)
        return out, ns
