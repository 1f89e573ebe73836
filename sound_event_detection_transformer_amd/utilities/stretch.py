"""Time stretch and pitch shift on the device: E excerpts of a staged bank, each with its own duration factor and its own shift in
semitones, transformed in ONE call (sedt_stretch, csrc/stretch.hip) - the two effects of the soundscape generator's event
specification (URBAN-SED drew a pitch shift of +-3 semitones and a duration factor of 0.8 .. 1.2 per event, DESED's synthetic subset the
pitch shift).  DESIGN.md section 4 ("Pitch shift and time stretch on the device") holds the definition, include/sedt_hip.h the ABI;
tests/stretch_ref.py restates it in float64.

    fx = DeviceStretch(16000)                                     # the tables go to the device once
    out, ms = fx(sounds, factors=[1.1, 0.8], semitones=[-2.0, 3.0])     # (E, stride) f32 on the device, samples per sound
    out, ms = fx.time_stretch(sounds, 1.25);  out, ms = fx.pitch_shift(sounds, -3.0)

The method is the classic phase vocoder followed by band-limited resampling - the method of librosa's time_stretch / pitch_shift and
of resampy - restated, with bit parity claimed with no package (none is a dependency).  For an excerpt x of n samples, a duration factor
f (the generator's convention: the result lasts f times as long) and p semitones, all on the host in float64:

    alpha = 2^(p / 12),  g = f alpha,  m = floor(n f + 0.5) samples come out,  m1 = floor(n g + 0.5),  r = 1 / g
    STFT      N = n_fft, hop = N / 4, periodic Hann, centred with ZEROS outside [0, n) (no reflection): T = 1 + n div hop frames
    vocoder   U = the steps u >= 0 with fl64(u r) < T - ceil(T / r), corrected by one where the rounded product says otherwise;
              step u reads frames i = floor(u r), i + 1 (zero from T on), interpolates the magnitudes and advances the phase by the
              wrapped difference of the two frames' angles; the phase is float64 on the device
    inverse   inverse real FFT, window, overlap-add at u hop over the sum of squared windows; the first N / 2 samples dropped, z = the
              next m1
    resample  y[i] = sum_j s w(s (i alpha - j)) z[j], s = min(1, 1 / alpha), w = resample.kaiser_sinc at ``quality`` read from a table
              of 512 points per zero crossing (float64 rounded once to f32) with linear interpolation - resampy's own evaluation,
              which is what admits a real ratio (utilities/resample.py's polyphase kernel needs a reduced fraction)
    g == 1 skips the vocoder (z = x), p == 0 the resampler (y = z); f == 1 and p == 0 is a copy.

Envelope: n_fft 512, 1024 or 2048; 1 <= n <= 2^26; 0.5 <= f <= 2; |p| <= 12.  What this is not: a plain vocoder smears transients (no
phase locking, no transient preservation), and nothing re-measures a sound's level after the effect.

``stretch_lengths``, ``stretch_jobs``, ``hann_window``, ``twiddle_table`` and ``filter_table`` are the host half and need no GPU; they
raise ValueError with the envelope spelled out."""
import math

import numpy as np
import torch

from .. import lib as L
from .resample import QUALITIES, kaiser_sinc
from .transforms import PinnedRing

# the device record of sedt_stretch (include/sedt_hip.h: SedtStretchJob, 72 bytes; sedt_sizeof 15)
JOB = np.dtype([('src_off', '<i8'), ('n', '<i8'), ('dst_off', '<i8'), ('m', '<i8'), ('m1', '<i8'), ('r', '<f8'), ('alpha', '<f8'),
                ('T', '<i4'), ('U', '<i4'), ('ws_off', '<i8')])
N_FFTS = (512, 1024, 2048)
MAX_N = 1 << 26
FACTOR_RANGE = (0.5, 2.0)
SEMITONE_RANGE = (-12.0, 12.0)
ENVELOPE = (f'n_fft in {N_FFTS}; 1 <= n <= 2^26 samples; {FACTOR_RANGE[0]} <= duration factor <= {FACTOR_RANGE[1]}; '
            f'{SEMITONE_RANGE[0]:g} <= semitones <= {SEMITONE_RANGE[1]:g}')
STATUS_REASONS = {2: 'the record does not lie inside the bank, the destination or the workspace'}


def check_effect(factor, semitones, who='stretch'):
    """(factor, semitones) as float64 inside the envelope, else ValueError"""
    f, p = float(factor), float(semitones)
    if not (FACTOR_RANGE[0] <= f <= FACTOR_RANGE[1]) or not (SEMITONE_RANGE[0] <= p <= SEMITONE_RANGE[1]):          # (NaN fails)
        raise ValueError(f'{who}: duration factor {factor!r}, {semitones!r} semitones: outside the envelope ({ENVELOPE})')
    return f, p


def stretch_lengths(n, factor, semitones, n_fft=2048):
    """(m, m1, r, alpha, T, U) of one excerpt of n samples (module docstring); g == 1 has T = U = 0"""
    if n_fft not in N_FFTS:
        raise ValueError(f'stretch: n_fft {n_fft!r}: outside the envelope ({ENVELOPE})')
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_N:
        raise ValueError(f'stretch: an excerpt of {n!r} samples: outside the envelope ({ENVELOPE})')
    f, p = check_effect(factor, semitones)
    n = int(n)
    alpha = float(np.float64(2.0) ** (np.float64(p) / np.float64(12.0)))
    g = f * alpha
    m, m1 = int(math.floor(n * f + 0.5)), int(math.floor(n * g + 0.5))
    if g == 1.0:
        return m, n, 1.0, alpha, 0, 0
    r = 1.0 / g
    T = 1 + n // (n_fft // 4)
    U = max(int(math.ceil(T / r)), 1)
    while U > 1 and (U - 1) * r >= T:                     # U = the steps u with fl64(u r) < T: the rounded product decides
        U -= 1
    while U * r < T:
        U += 1
    return m, m1, r, alpha, T, U


def job_floats(n_fft, m1, T, U):
    """the floats of the workspace one job owns: D re / im [T][K], S re / im [U][K], frames [U][N], z [m1], rounded up to 4"""
    K = n_fft // 2 + 1
    return (2 * T * K + 2 * U * K + U * n_fft + m1 + 3) & ~3


def stretch_jobs(ns, factors, semitones, n_fft=2048, src_offs=None, dst_offs=None):
    """the JOB records of E excerpts and the floats of workspace they need.  src_offs: each excerpt's first sample in the bank (default:
    back to back); dst_offs: each result's first sample in the destination (default: back to back, each on a multiple of 4)"""
    E = len(ns)
    if len(factors) != E or len(semitones) != E:
        raise ValueError('stretch_jobs: one duration factor and one pitch shift per excerpt')
    jobs = np.zeros(E, JOB)
    src = dst = ws = 0
    for e in range(E):
        m, m1, r, alpha, T, U = stretch_lengths(ns[e], factors[e], semitones[e], n_fft)
        jobs[e] = (src if src_offs is None else int(src_offs[e]), int(ns[e]), dst if dst_offs is None else int(dst_offs[e]), m, m1, r,
                   alpha, T, U, ws)
        src, dst, ws = src + int(ns[e]), dst + ((m + 3) & ~3), ws + job_floats(n_fft, m1, T, U)
    return jobs, ws


def regions(job, n_fft):
    """the float offsets of a job's parts in the workspace: dict D_re, D_im, S_re, S_im, frames, z -> (offset, shape)"""
    K, T, U = n_fft // 2 + 1, int(job['T']), int(job['U'])
    o = int(job['ws_off'])
    out = {}
    for name, shape in (('D_re', (T, K)), ('D_im', (T, K)), ('S_re', (U, K)), ('S_im', (U, K)), ('frames', (U, n_fft)),
                        ('z', (int(job['m1']),))):
        out[name] = (o, shape)
        o += int(np.prod(shape))
    return out


def hann_window(n_fft):
    """the periodic Hann window, float64 [n_fft]"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)


def twiddle_table(n_fft):
    """f32 [2][n_fft / 2 + 1]: cos(2 pi t / n_fft) and -sin(2 pi t / n_fft), float64 rounded once (the mel stage's table)"""
    ang = 2.0 * np.pi * np.arange(n_fft // 2 + 1, dtype=np.float64) / n_fft
    return np.stack([np.cos(ang), -np.sin(ang)]).astype(np.float32)


def filter_table(quality='kaiser_best'):
    """(f32 [512 Z + 1]: kaiser_sinc at q / 512, float64 rounded once; Z, the zero crossings)"""
    if quality not in QUALITIES:
        raise ValueError(f'stretch: quality {quality!r} is none of {sorted(QUALITIES)}')
    Z, rolloff, beta = QUALITIES[quality]
    u = np.arange(Z * L.STRETCH_TABLE_RES + 1, dtype=np.float64) / L.STRETCH_TABLE_RES
    return kaiser_sinc(u, Z, rolloff, beta).astype(np.float32), Z


class DeviceStretch(object):
    """sr: the sample rate (kept for the callers; the effects are defined on samples); n_fft: 512, 1024 or 2048; quality: the
    resampling filter.  A call is five launches behind one another and reads nothing back."""

    def __init__(self, sr, n_fft=2048, quality='kaiser_best', device='cuda'):
        if n_fft not in N_FFTS:
            raise ValueError(f'DeviceStretch: n_fft {n_fft!r}: outside the envelope ({ENVELOPE})')
        self.sr, self.n_fft, self.quality = int(sr), int(n_fft), quality
        table, self.Z = filter_table(quality)
        self.dev = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self._window, self._twiddle, self._table = up(hann_window(n_fft).astype(np.float32)), up(twiddle_table(n_fft)), up(table)
        self._ring, self._ws, self._keep = None, None, None
        self.last_jobs = self.last_workspace = self.last_status = None

    def workspace(self, floats):
        """an f32 device tensor of at least ``floats`` elements, owned by this object and reused (grown when a call needs more)"""
        if self._ws is None or self._ws.numel() < floats:
            self._ws = torch.empty(max(int(floats), 4), dtype=torch.float32, device=self.dev)
        return self._ws

    def launch(self, flat, jobs, dst, workspace, status=None, jobs_dev=None):
        """the raw stage: ``jobs`` (a host JOB array) over the f32 device tensors flat -> dst through ``workspace`` (f32, the caller's).
        jobs_dev: the same records on the device (uint8), else they travel through this object's pinned ring.  Returns the int32 [E]
        status tensor (on the device; nothing is read back)."""
        jobs = np.ascontiguousarray(jobs, JOB)
        E = int(jobs.shape[0])
        for t, who in ((flat, 'flat'), (dst, 'dst'), (workspace, 'workspace')):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f'DeviceStretch.launch: {who} is a contiguous f32 device tensor')
        if status is None:
            status = torch.zeros(max(E, 1), dtype=torch.int32, device=self.dev)
        if jobs_dev is None:
            if self._ring is None:
                self._ring = PinnedRing(self.dev)
            jobs_dev = self._ring.upload(jobs.view(np.uint8).reshape(-1) if E else np.zeros(8, np.uint8))
        host = jobs if E else np.zeros(1, JOB)
        L.check(L.load().sedt_stretch(L.p(flat), flat.numel(), host.ctypes.data, L.p(jobs_dev), E, L.p(dst), dst.numel(), L.p(workspace),
                                      4 * workspace.numel(), L.p(self._window), L.p(self._twiddle), L.p(self._table), self.Z, self.n_fft,
                                      L.p(status), L.stream_ptr()), 'stretch')
        return status

    def __call__(self, waves, factors=None, semitones=None):
        """waves: a list of 1-D float32 arrays / tensors (host or device) or an (E, n) tensor; factors / semitones: one number or one
        per sound (None: 1 / 0).  Returns (out (E, stride) f32 on the device, samples per sound); samples past a sound's m are 0.
        ``last_jobs`` / ``last_workspace`` / ``last_status`` keep the call's records, its workspace (the spectra and z of every
        sound: ``regions``) and its statuses."""
        waves = [w if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, np.float32)) for w in waves]
        E = len(waves)
        if not E or any(w.dim() != 1 or w.dtype != torch.float32 for w in waves):
            raise ValueError('DeviceStretch: at least one sound, each a 1-D float32 waveform')
        spread = lambda v, d: [d] * E if v is None else ([float(v)] * E if np.ndim(v) == 0 else [float(a) for a in v])
        ns = [int(w.shape[0]) for w in waves]
        jobs, floats = stretch_jobs(ns, spread(factors, 1.0), spread(semitones, 0.0), self.n_fft)
        stride = int(jobs['m'].max())
        jobs['dst_off'] = np.arange(E, dtype=np.int64) * stride
        pins = [w.contiguous().pin_memory() for w in waves if not w.is_cuda]
        it = iter(pins)
        flat = torch.cat([w if w.is_cuda else next(it).to(self.dev, non_blocking=True) for w in waves])
        out = torch.zeros((E, stride), dtype=torch.float32, device=self.dev)
        ws = self.workspace(floats)
        self.last_status = self.launch(flat, jobs, out.view(-1), ws)
        self.last_jobs, self.last_workspace, self._keep = jobs, ws, (flat, pins)
        return out, [int(m) for m in jobs['m']]

    def time_stretch(self, waves, factor):
        """every sound lasts ``factor`` times as long, at its pitch"""
        return self(waves, factors=factor)

    def pitch_shift(self, waves, semitones):
        """every sound ``semitones`` higher, at its length"""
        return self(waves, semitones=semitones)

    def read(self, e, name):
        """part ``name`` (D_re, D_im, S_re, S_im, frames, z) of sound e of the last call, as a host array (synchronises: for tests)"""
        o, shape = regions(self.last_jobs[e], self.n_fft)[name]
        return self.last_workspace[o:o + int(np.prod(shape))].cpu().numpy().reshape(shape)

    @staticmethod
    def check(status, who='DeviceStretch'):
        """raise on a non-zero status (reads them back)"""
        bad = np.flatnonzero(status.cpu().numpy())
        if len(bad):
            raise RuntimeError(f'{who}: sound {int(bad[0])}: status 2: {STATUS_REASONS[2]}')
