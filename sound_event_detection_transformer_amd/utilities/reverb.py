"""Reverberation on the device: E excerpts of a staged bank, each convolved with a room impulse response (RIR) of a staged RIR bank, in
ONE call (sedt_reverb, csrc/reverb.hip) - the remaining event effect of the soundscape generator (Scaper's reverb control; DESED's
later synthetic sets convolved every source with a room response).  DESIGN.md section 4 ("Reverberation on the device") holds the
definition, include/sedt_hip.h the ABI; tests/reverb_ref.py restates it in float64.

    rv = DeviceReverb(16000).add_rirs(rirs)                       # the partition spectra go to the device once
    out, ms = rv.rv(sounds, rir_index=[0, 2])                     # (E, stride) f32 on the device, samples per sound: n + L - 1

The method is uniformly partitioned overlap-save convolution.  N = n_fft, Bs = N / 2 samples per block, K = N / 2 + 1 bins:
    RIR bank  response r of L taps is P = ceil(L / Bs) partitions; H[r][p] = the N-point real FFT of taps [p Bs, (p + 1) Bs) followed by
              Bs zeros.  With normalize='energy' a response is scaled to sum h^2 = 1, in float64 on the host, before it is staged
    forward   input block j = x[(j - 1) Bs, (j + 1) Bs), zero outside [0, n), times the event's fade (sedt_soundscape's ramp over the n
              dry samples); X[j] = its real FFT; nb = ceil(n / Bs) + 1 blocks
    products  output block j: Y = sum over p ascending of X[j - p] H[r][p]; the inverse real FFT; the LAST Bs samples of the frame are
              wet[j Bs, (j + 1) Bs); ceil((n + L - 1) / Bs) blocks, clipped to n + L - 1 samples

Envelope: n_fft 512, 1024 or 2048; 1 <= n <= 2^26; 0 <= fade; 1 <= L <= 176 n_fft / 2 (at 2048: 180224 taps, 4 s at 44.1 kHz fit).

``reverb_jobs``, ``regions``, ``rir_table``, ``prepare_rirs`` and ``twiddle_table`` are the host half and need no GPU; they raise
ValueError with the envelope spelled out."""
import numpy as np
import torch

from .. import lib as L
from .stretch import twiddle_table
from .transforms import PinnedRing

# the device records (include/sedt_hip.h: SedtReverbJob 40 bytes, SedtReverbTail 40, SedtReverbBed 32; sedt_sizeof 16, 17, 18)
JOB = np.dtype([('src_off', '<i8'), ('n', '<i8'), ('dst_off', '<i8'), ('rir', '<i4'), ('fade', '<i4'), ('ws_off', '<i8')])
TAIL = np.dtype([('wet_off', '<i8'), ('onset', '<i8'), ('head', '<i8'), ('total', '<i8'), ('gain', '<f4'), ('pad', '<i4')])
BED = np.dtype([('src', '<i4'), ('tail_lo', '<i4'), ('start', '<i8'), ('gain', '<f4'), ('tail_hi', '<i4'), ('dst_off', '<i8')])
SIZEOF = {16: JOB, 17: TAIL, 18: BED}
N_FFTS = (512, 1024, 2048)
MAX_N = 1 << 26
MAX_PART = L.REVERB_MAXPART
ENVELOPE = (f'n_fft in {N_FFTS}; 1 <= n <= 2^26 samples; 0 <= fade <= 2^26; a response of 1 .. {MAX_PART} n_fft / 2 taps')
STATUS_REASONS = {2: 'the record does not lie inside the bank, the destination, the workspace or the RIR table'}


def check_sizes():
    """the record dtypes against the library that is loaded (sedt_sizeof); raises on drift"""
    for which, dt in SIZEOF.items():
        got = L.load().sedt_sizeof(which)
        if got != dt.itemsize:
            raise RuntimeError(f'utilities/reverb.py: record {which} has {dt.itemsize} bytes here, {got} in the library')


def max_taps(n_fft):
    return MAX_PART * (n_fft // 2)


def blocks_in(n, n_fft):
    """input blocks of a dry sound of n samples: ceil(n / Bs) + 1"""
    return -(-int(n) // (n_fft // 2)) + 1


def blocks_out(n, taps, n_fft):
    """output blocks: ceil((n + L - 1) / Bs)"""
    return -(-(int(n) + int(taps) - 1) // (n_fft // 2))


def job_floats(n_fft, n):
    """the floats of the workspace one job owns: X re / im [nb][K], rounded up to 4"""
    return (2 * blocks_in(n, n_fft) * (n_fft // 2 + 1) + 3) & ~3


def check_shape(n, taps, fade, n_fft, who='reverb'):
    if n_fft not in N_FFTS:
        raise ValueError(f'{who}: n_fft {n_fft!r}: outside the envelope ({ENVELOPE})')
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_N:
        raise ValueError(f'{who}: a sound of {n!r} samples: outside the envelope ({ENVELOPE})')
    if not 1 <= int(taps) <= max_taps(n_fft):
        raise ValueError(f'{who}: a response of {taps!r} taps: outside the envelope ({ENVELOPE})')
    if not 0 <= int(fade) <= MAX_N:
        raise ValueError(f'{who}: a fade of {fade!r} samples: outside the envelope ({ENVELOPE})')


def reverb_jobs(ns, rirs, rir_lens, n_fft=2048, src_offs=None, dst_offs=None, fades=None):
    """the JOB records of E dry sounds and the floats of workspace they need.  rirs: each sound's response index; rir_lens: the taps of
    every response of the bank; src_offs: each sound's first sample in the bank (default: back to back); dst_offs: each result's first
    sample in the destination (default: back to back, each on a multiple of 4); fades: the ramp lengths (default 0)"""
    E = len(ns)
    if len(rirs) != E or (fades is not None and len(fades) != E):
        raise ValueError('reverb_jobs: one response index (and one fade) per sound')
    jobs = np.zeros(E, JOB)
    src = dst = ws = 0
    for e in range(E):
        r = int(rirs[e])
        if not 0 <= r < len(rir_lens):
            raise ValueError(f'reverb_jobs: sound {e} names response {r} of {len(rir_lens)}')
        fade = 0 if fades is None else int(fades[e])
        check_shape(ns[e], rir_lens[r], fade, n_fft)
        n, total = int(ns[e]), int(ns[e]) + int(rir_lens[r]) - 1
        jobs[e] = (src if src_offs is None else int(src_offs[e]), n, dst if dst_offs is None else int(dst_offs[e]), r, fade, ws)
        src, dst, ws = src + n, dst + ((total + 3) & ~3), ws + job_floats(n_fft, n)
    return jobs, ws


def regions(job, n_fft):
    """the float offsets of a job's parts in the workspace: dict X_re, X_im -> (offset, shape)"""
    K, nb = n_fft // 2 + 1, blocks_in(job['n'], n_fft)
    o = int(job['ws_off'])
    return {'X_re': (o, (nb, K)), 'X_im': (o + nb * K, (nb, K))}


def rir_table(rir_lens, n_fft):
    """(int64 [3][R]: taps | first partition | first tap in the concatenated tap array, the partitions in all)"""
    lens = np.asarray(rir_lens, np.int64).reshape(-1)
    parts = -(-lens // (n_fft // 2))
    first = np.concatenate([[0], np.cumsum(parts)]).astype(np.int64)
    taps = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.ascontiguousarray(np.stack([lens, first[:-1], taps[:-1]])), int(first[-1])


def prepare_rirs(rirs, n_fft, normalize='energy', first=0):
    """the responses as float32 arrays ready to stage: int16 widened (x / 32768), scaled in float64 to sum h^2 = 1 under
    normalize='energy'.  Empty, non-finite, all-zero and over-long responses are refused."""
    if normalize not in ('energy', None):
        raise ValueError(f"add_rirs: normalize {normalize!r} is neither 'energy' nor None")
    out = []
    for i, h in enumerate(rirs):
        h = h.detach().cpu().numpy() if torch.is_tensor(h) else np.asarray(h)
        if h.ndim != 1 or h.dtype not in (np.float32, np.int16):
            raise ValueError(f'add_rirs: response {first + i} is not a 1-D float32 / int16 array')
        if h.shape[0] == 0:
            raise ValueError(f'add_rirs: response {first + i} is empty')
        if h.shape[0] > max_taps(n_fft):
            raise ValueError(f'add_rirs: response {first + i} has {h.shape[0]} taps: more than {MAX_PART} partitions of n_fft / 2 = '
                             f'{n_fft // 2} ({max_taps(n_fft)} taps)')
        h64 = h.astype(np.float64) / 32768.0 if h.dtype == np.int16 else h.astype(np.float64)
        if not np.isfinite(h64).all():
            raise ValueError(f'add_rirs: response {first + i} holds non-finite taps')
        energy = float(np.sum(h64 * h64))
        if energy == 0.0:
            raise ValueError(f'add_rirs: response {first + i} is all zero')
        if normalize == 'energy':
            h64 = h64 / np.sqrt(np.float64(energy))
        out.append(h64.astype(np.float32))
    return out


class DeviceReverb(object):
    """sr: the sample rate of the sounds and of the staged responses; n_fft: 512, 1024 or 2048 (the block is n_fft / 2 samples).  A call
    is two launches behind one another and reads nothing back."""

    def __init__(self, sr, n_fft=2048, device='cuda', resample_quality='kaiser_best', group=0):
        if n_fft not in N_FFTS:
            raise ValueError(f'DeviceReverb: n_fft {n_fft!r}: outside the envelope ({ENVELOPE})')
        self.sr, self.n_fft, self.group = int(sr), int(n_fft), int(group)
        self.dev = torch.device(device)
        self.resample_quality, self._resamplers = resample_quality, {}
        check_sizes()
        self._twiddle = torch.from_numpy(twiddle_table(n_fft)).to(self.dev)
        self.rirs, self.rir_lens = [], []                            # the staged responses (host float32) and their taps
        self.table, self.n_parts = None, 0                           # rir_table on the host
        self._taps = self._table_dev = self.h_re = self.h_im = None
        self._ring, self._ws, self._keep = None, None, None
        self.last_jobs = self.last_workspace = self.last_status = None

    def resampler(self, rate):
        rs = self._resamplers.get(int(rate))
        if rs is None:
            from .resample import DeviceResampler
            rs = self._resamplers[int(rate)] = DeviceResampler(int(rate), self.sr, self.resample_quality, device=self.dev)
        return rs

    def __len__(self):
        return len(self.rirs)

    def add_rirs(self, rirs, sample_rates=None, normalize='energy'):
        """stage room impulse responses: 1-D float32 / int16 at ``sr`` or, with ``sample_rates`` (one int or one per response), at any
        rate - resampled on the device as the sound banks are.  normalize='energy' scales each to sum h^2 = 1 (float64, on the host);
        None keeps it as given.  Empty, non-finite, all-zero and over-long responses are refused.  The partition spectra of the WHOLE
        bank are written in one launch.  Returns self."""
        rirs = list(rirs)
        if not rirs:
            raise ValueError('add_rirs: at least one response')
        if sample_rates is not None:
            from .recording import stage_resampled
            for i, h in enumerate(rirs):
                if int(h.shape[0]) == 0:
                    raise ValueError(f'add_rirs: response {len(self.rirs) + i} is empty')
            flat, off, ns, keep = stage_resampled(rirs, sample_rates, self.resampler, self.dev)
            host = flat.cpu().numpy()                                # staging is not the loop: read back once, normalised on the host
            del keep
            rirs = [host[int(off[i]):int(off[i]) + int(ns[i])].copy() for i in range(len(ns))]
        new = prepare_rirs(rirs, self.n_fft, normalize, first=len(self.rirs))
        if len(self.rirs) + len(new) > L.REVERB_MAXJOBS:
            raise ValueError(f'add_rirs: more than {L.REVERB_MAXJOBS} responses')
        every = self.rirs + new
        lens = [int(h.shape[0]) for h in every]
        table, n_parts = rir_table(lens, self.n_fft)
        K = self.n_fft // 2 + 1
        taps = torch.from_numpy(np.concatenate(every)).to(self.dev)
        table_dev = torch.from_numpy(table).to(self.dev)
        h_re, h_im = self._alloc_spectra(n_parts, K)
        L.check(L.load().sedt_reverb_spectra(L.p(taps), taps.numel(), table.ctypes.data, L.p(table_dev), len(every), L.p(h_re), L.p(h_im),
                                             n_parts, L.p(self._twiddle), self.n_fft, L.stream_ptr()), 'reverb_spectra')
        self.rirs, self.rir_lens, self.table, self.n_parts = every, lens, table, n_parts
        self._taps, self._table_dev, self.h_re, self.h_im = taps, table_dev, h_re, h_im
        return self

    def _alloc_spectra(self, n_parts, K):
        """the two f32 (n_parts, K) device tensors the bank's spectra are written to (a test puts guards around them)"""
        return (torch.zeros((n_parts, K), dtype=torch.float32, device=self.dev),
                torch.zeros((n_parts, K), dtype=torch.float32, device=self.dev))

    def spectra(self, r):
        """H of response r as the device holds it: complex128 (P, K) on the host (synchronises: for tests)"""
        lo = int(self.table[1][r])
        P = -(-self.rir_lens[r] // (self.n_fft // 2))
        return self.h_re[lo:lo + P].cpu().numpy().astype(np.float64) + 1j * self.h_im[lo:lo + P].cpu().numpy().astype(np.float64)

    def workspace(self, floats):
        """an f32 device tensor of at least ``floats`` elements, owned by this object and reused (grown when a call needs more)"""
        if self._ws is None or self._ws.numel() < floats:
            self._ws = torch.empty(max(int(floats), 4), dtype=torch.float32, device=self.dev)
        return self._ws

    def launch(self, flat, jobs, dst, workspace, status=None, jobs_dev=None, group=None):
        """the raw stage: ``jobs`` (a host JOB array) over the f32 device tensors flat -> dst through ``workspace`` (f32, the caller's).
        jobs_dev: the same records on the device (uint8), else they travel through this object's pinned ring.  Returns the int32 [E]
        status tensor (on the device; nothing is read back)."""
        if self.table is None:
            raise RuntimeError('DeviceReverb.launch: add_rirs() first')
        jobs = np.ascontiguousarray(jobs, JOB)
        E = int(jobs.shape[0])
        for t, who in ((flat, 'flat'), (dst, 'dst'), (workspace, 'workspace')):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f'DeviceReverb.launch: {who} is a contiguous f32 device tensor')
        if status is None:
            status = torch.zeros(max(E, 1), dtype=torch.int32, device=self.dev)
        if jobs_dev is None:
            if self._ring is None:
                self._ring = PinnedRing(self.dev)
            jobs_dev = self._ring.upload(jobs.view(np.uint8).reshape(-1) if E else np.zeros(8, np.uint8))
        host = jobs if E else np.zeros(1, JOB)
        L.check(L.load().sedt_reverb(L.p(flat), flat.numel(), host.ctypes.data, L.p(jobs_dev), E, L.p(dst), dst.numel(), L.p(workspace),
                                     4 * workspace.numel(), L.p(self.h_re), L.p(self.h_im), self.n_parts, self.table.ctypes.data,
                                     L.p(self._table_dev), len(self.rirs), L.p(self._twiddle), self.n_fft,
                                     self.group if group is None else int(group), L.p(status), L.stream_ptr()), 'reverb')
        return status

    def rv(self, sounds, rir_index, fades=None):
        """sounds: a list of 1-D float32 arrays / tensors (host or device); rir_index: one response index or one per sound; fades: the
        ramp lengths (None: 0).  Returns (out (E, stride) f32 on the device, samples per sound: n + L - 1); samples past a sound's end
        are 0.  ``last_jobs`` / ``last_workspace`` / ``last_status`` keep the call's records, its workspace and its statuses."""
        waves = [w if torch.is_tensor(w) else torch.from_numpy(np.array(w, np.float32)) for w in sounds]
        E = len(waves)
        if not E or any(w.dim() != 1 or w.dtype != torch.float32 for w in waves):
            raise ValueError('DeviceReverb: at least one sound, each a 1-D float32 waveform')
        idx = [int(rir_index)] * E if np.ndim(rir_index) == 0 else [int(r) for r in rir_index]
        ns = [int(w.shape[0]) for w in waves]
        jobs, floats = reverb_jobs(ns, idx, self.rir_lens, self.n_fft, fades=fades)
        totals = [int(j['n']) + self.rir_lens[int(j['rir'])] - 1 for j in jobs]
        stride = max(totals)
        jobs['dst_off'] = np.arange(E, dtype=np.int64) * stride
        pins = [w.contiguous().pin_memory() for w in waves if not w.is_cuda]
        it = iter(pins)
        flat = torch.cat([w if w.is_cuda else next(it).to(self.dev, non_blocking=True) for w in waves])
        out = torch.zeros((E, stride), dtype=torch.float32, device=self.dev)
        ws = self.workspace(floats)
        self.last_status = self.launch(flat, jobs, out.view(-1), ws)
        self.last_jobs, self.last_workspace, self._keep = jobs, ws, (flat, pins)
        return out, totals

    __call__ = rv

    def read(self, e, name):
        """part ``name`` (X_re, X_im) of sound e of the last call, as a host array (synchronises: for tests)"""
        o, shape = regions(self.last_jobs[e], self.n_fft)[name]
        return self.last_workspace[o:o + int(np.prod(shape))].cpu().numpy().reshape(shape)

    @staticmethod
    def check(status, who='DeviceReverb'):
        """raise on a non-zero status (reads them back)"""
        bad = np.flatnonzero(status.cpu().numpy())
        if len(bad):
            raise RuntimeError(f'{who}: sound {int(bad[0])}: status 2: {STATUS_REASONS[2]}')
