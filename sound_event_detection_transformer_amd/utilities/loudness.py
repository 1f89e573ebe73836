"""Programme loudness (ITU-R BS.1770-4: K-weighted, gated) measured on the device, one channel with channel weight 1 - the sources of
a bank are mono after staging.  DESIGN.md section 4 ("Loudness (BS.1770) on the device") holds the definition; tests/loudness_ref.py
restates it in float64; csrc/loudness.hip is the kernel (sedt_loudness, sedt_scale_sources).

    loud = DeviceLoudness(16000)
    res = loud.measure_waves(recordings)                 # LoudnessResult: lufs (float64, -inf where no block passes the gates), ...
    flat, off, ns, keep = stage_recordings(recordings, 'cuda')
    out = loud.normalize(flat, off[:-1], ns, -23.0)      # in place: measure, one sedt_bank_stats, one sedt_scale_sources launch

The 400 ms blocks overlap by 75 %, so a block is four hops of H = (sr + 5) // 10 samples; a source shorter than one block has no block in
the standard and is measured HERE as one block over all its samples (``short``).  ``k_weighting``, ``hop_map`` and ``lufs_of`` are the
host half and need no GPU."""
import collections
import functools
import math

import numpy as np
import torch

from .. import lib as L

Z_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)         # the absolute gate (-70 LUFS) in the z domain

LoudnessResult = collections.namedtuple('LoudnessResult', 'lufs zbar blocks n_abs n_rel short')
LoudnessResult.__doc__ = """per source: lufs float64 (-inf where no block passes the gates), zbar float64 (the gated mean square), blocks /
n_abs / n_rel int32 (the blocks, those over the absolute gate, those over both gates), short bool (shorter than one 400 ms block:
measured as one block over all its samples, which the standard does not define)"""
NormalizeResult = collections.namedtuple('NormalizeResult', 'gains limited silent before')
NormalizeResult.__doc__ = """per source: gains float32 (applied), limited bool (the peak limit set the gain), silent bool (-inf LUFS: gain 1,
left as it was), before: the LoudnessResult the gains were computed from"""


def hop_samples(sr):
    """H: the 100 ms hop in samples"""
    return (int(sr) + 5) // 10


@functools.lru_cache(maxsize=None)
def _k_weighting(sr):
    fs = float(sr)

    def stage(f0, Q, shelf_db):
        K = math.tan(math.pi * f0 / fs)
        a0 = 1.0 + K / Q + K * K
        if shelf_db is None:
            b = (1.0, -2.0, 1.0)
        else:
            Vh = 10.0 ** (shelf_db / 20.0)
            Vb = Vh ** 0.4996667741545416
            b = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0)
        return b + (2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)

    return stage(1681.974450955533, 0.7071752369554196, 3.999843853973347) + stage(38.13547087602444, 0.5003270373238773, None)


def k_weighting(sr):
    """float64 [10]: b0 b1 b2 a1 a2 of the shelf stage, then of the high-pass stage (a0 = 1 dropped) - the closed form of the
    standard's two stages at sample rate ``sr`` (its table at 48 kHz)"""
    if int(sr) < 1:
        raise ValueError(f'k_weighting: sample rate {sr}')
    return np.asarray(_k_weighting(int(sr)), np.float64)


@functools.lru_cache(maxsize=None)
def _hop_map(sr):
    c = _k_weighting(sr)
    cols = []
    for k in range(4):
        s = [0.0] * 4
        s[k] = 1.0
        for _ in range(hop_samples(sr)):                 # the cascade on a zero sample: o = s0; s0 = -a1 o + s1; s1 = -a2 o
            o1 = c[0] * 0.0 + s[0]
            s[0], s[1] = c[1] * 0.0 - c[3] * o1 + s[1], c[2] * 0.0 - c[4] * o1
            o2 = c[5] * o1 + s[2]
            s[2], s[3] = c[6] * o1 - c[8] * o2 + s[3], c[7] * o1 - c[9] * o2
        cols.append(s)
    return tuple(tuple(cols[k][j] for k in range(4)) for j in range(4))


def hop_map(sr):
    """float64 (4, 4): the state of the cascade (shelf s0 s1, high-pass s0 s1) after H zero-input samples, column k from unit state k,
    by running the cascade in float64.  The state at the start of hop h + 1 is hop_map @ (the state at the start of hop h) + (the state
    hop h leaves when it is filtered from zero state): what lets sedt_loudness filter the hops in parallel."""
    if int(sr) < 1:
        raise ValueError(f'hop_map: sample rate {sr}')
    return np.asarray(_hop_map(int(sr)), np.float64)


def lufs_of(zbar):
    """-0.691 + 10 log10(zbar) in float64, -inf for zbar == 0"""
    z = np.asarray(zbar, np.float64)
    return np.where(z > 0, -0.691 + 10.0 * np.log10(np.where(z > 0, z, 1.0)), -np.inf)


def work_doubles(lens, hop):
    """the float64 words of sedt_loudness' workspace: every source holds len // hop + 1 hop energies"""
    return int(sum(int(n) // int(hop) + 1 for n in lens))


class DeviceLoudness(object):
    """sr: the sample rate of what is measured.  See the module docstring."""

    def __init__(self, sr, device='cuda'):
        self.sr, self.hop = int(sr), hop_samples(sr)
        self.coef, self.map = k_weighting(sr), hop_map(sr)
        self.dev = torch.device(device)
        self._consts = None

    def _tables(self, off, lens):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(self.dev)
        return up(off), up(lens)

    def launch(self, flat, flat_len, d_off, d_len, lens):
        """ONE sedt_loudness launch on the current stream over sources whose int64 offset / length tables already lie on the device
        (``lens``: the same lengths on the host, which size the workspace): (zbar float64 [n], counts int32 [n, 4]) device tensors,
        nothing read back - ``result`` does that"""
        n = len(lens)
        if self._consts is None:
            self._consts = torch.from_numpy(np.concatenate([self.coef, self.map.reshape(-1)])).to(self.dev)
        words = work_doubles(lens, self.hop)
        work = torch.empty(words, dtype=torch.float64, device=self.dev)
        zbar = torch.zeros(n, dtype=torch.float64, device=self.dev)
        counts = torch.zeros((n, 4), dtype=torch.int32, device=self.dev)
        L.check(L.load().sedt_loudness(L.p(flat), int(flat_len), L.p(d_off), L.p(d_len), n, L.p(self._consts), L.p(self._consts[10:]),
                                       self.hop, Z_ABS, L.p(work), words, L.p(zbar), L.p(counts), L.stream_ptr()), 'loudness')
        return zbar, counts

    @staticmethod
    def result(zbar, counts, what='DeviceLoudness.measure'):
        """read one launch back: a LoudnessResult of host arrays; non-finite input is refused with the source's index"""
        zbar, counts = zbar.cpu().numpy(), counts.cpu().numpy()
        for i in range(zbar.shape[0]):
            if counts[i, 0] < 0:
                raise RuntimeError(f'{what}: the workspace does not hold the hop energies of source {i}')
            if not math.isfinite(zbar[i]):
                raise ValueError(f'{what}: source {i} holds non-finite samples')
        return LoudnessResult(lufs_of(zbar), zbar, counts[:, 0].copy(), counts[:, 1].copy(), counts[:, 2].copy(), counts[:, 3] != 0)

    def _check(self, flat, off, lens):
        off, lens = np.asarray(off, np.int64).reshape(-1), np.asarray(lens, np.int64).reshape(-1)
        if not (torch.is_tensor(flat) and flat.dtype == torch.float32 and flat.dim() == 1 and flat.is_contiguous()
                and flat.device.type == self.dev.type):
            raise ValueError('DeviceLoudness: flat is a contiguous 1-D float32 tensor on the device')
        if off.shape != lens.shape or off.shape[0] < 1:
            raise ValueError('DeviceLoudness: one offset and one length per source, at least one source')
        if bool((off < 0).any()) or bool((lens < 0).any()) or int((off + lens).max()) > flat.numel():
            raise ValueError('DeviceLoudness: a source does not lie inside the flat vector')
        return off, lens

    def measure(self, flat, off, lens):
        """the loudness of sources flat[off[s]:off[s] + lens[s]] (flat: a 1-D float32 device tensor; off, lens: host integers): one
        launch, read back once"""
        off, lens = self._check(flat, off, lens)
        d_off, d_len = self._tables(off, lens)
        return self.result(*self.launch(flat, flat.numel(), d_off, d_len, lens))

    def measure_waves(self, waves):
        """stage 1-D float32 / int16 waves (host or device) with stage_recordings and measure them"""
        from .recording import stage_recordings
        waves = list(waves)
        if not waves:
            raise ValueError('DeviceLoudness.measure_waves: at least one wave')
        flat, off, ns, keep = stage_recordings(waves, self.dev)
        res = self.measure(flat[:int(off[-1])], off[:-1], ns)
        del keep                                                    # (the read-back above waited for the copies)
        return res

    def normalize(self, flat, off, lens, target_lufs, peak_limit=1.0):
        """bring every source to ``target_lufs`` IN PLACE: measure, take the peaks from sedt_bank_stats, gain = float32(min(10^((target -
        L) / 20), peak_limit / peak)) from float64 arithmetic, ONE sedt_scale_sources launch.  A source at -inf LUFS keeps gain 1 and is
        reported ``silent``; ``limited`` marks the sources whose gain the peak limit set.  Returns a NormalizeResult."""
        if not float(peak_limit) > 0.0 or not math.isfinite(float(target_lufs)):
            raise ValueError(f'DeviceLoudness.normalize: target {target_lufs} LUFS, peak_limit {peak_limit}')
        off, lens = self._check(flat, off, lens)
        d_off, d_len = self._tables(off, lens)
        n = lens.shape[0]
        zbar, counts = self.launch(flat, flat.numel(), d_off, d_len, lens)
        sumsq = torch.zeros(n, dtype=torch.float64, device=self.dev)
        peak = torch.zeros(n, dtype=torch.float32, device=self.dev)
        L.check(L.load().sedt_bank_stats(L.p(flat), flat.numel(), L.p(d_off), L.p(d_len), n, L.p(sumsq), L.p(peak), L.stream_ptr()),
                'bank_stats')
        before = self.result(zbar, counts, 'DeviceLoudness.normalize')
        gains, limited, silent = normalize_gains(before.lufs, peak.cpu().numpy(), target_lufs, peak_limit)
        d_gain = torch.from_numpy(gains).to(self.dev)
        L.check(L.load().sedt_scale_sources(L.p(flat), flat.numel(), L.p(d_off), L.p(d_len), n, L.p(d_gain), L.stream_ptr()),
                'scale_sources')
        return NormalizeResult(gains, limited, silent, before)


def normalize_gains(lufs, peak, target_lufs, peak_limit=1.0):
    """(gains float32, limited bool, silent bool) per source: float32(min(10^((target - L) / 20), peak_limit / peak)) in float64; a
    source at -inf LUFS: gain 1, silent.  Rounding the limit's gain to float32 can round it up: a limited gain is stepped down by
    float32 neighbours until float32(peak * gain) - the new peak, since a rounded product is monotone - is <= peak_limit."""
    lufs, peak = np.asarray(lufs, np.float64), np.asarray(peak, np.float64)
    gains, limited = np.ones(lufs.shape, np.float32), np.zeros(lufs.shape, bool)
    silent = np.isneginf(lufs)
    for i in range(lufs.shape[0]):
        if silent[i]:
            continue
        want = np.float64(10.0) ** ((np.float64(target_lufs) - lufs[i]) / np.float64(20.0))
        cap = np.float64(peak_limit) / peak[i] if peak[i] > 0 else np.inf
        limited[i] = bool(cap < want)
        g = np.float32(min(want, cap))
        while limited[i] and g > 0 and float(np.float32(peak[i]) * g) > float(peak_limit):
            g = np.nextafter(g, np.float32(0.0))
        gains[i] = g
    return gains, limited, silent
