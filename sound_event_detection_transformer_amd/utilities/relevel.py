"""Levels measured after the effects: the level of E regions of a staged bank - an event's excerpt, its stretched row, its wet row -
measured on the device in ONE launch (sedt_relevel, csrc/relevel.hip), and the gain that brings each region to its target written
straight into the DEVICE records of the events (SedtScapeEvent) and of their reverberation tails (SedtReverbTail) before
sedt_reverb_bed and sedt_soundscape read them.  Scaper and the DESED generator measure the PROCESSED event and then apply its SNR;
this is that step, with nothing read back.  DESIGN.md section 4 ("Levels measured after the effects") holds the definition,
include/sedt_hip.h the ABI; tests/relevel_ref.py restates it in float64.

    rl = DeviceRelevel(16000, level='lufs')
    jobs, doubles = relevel_jobs(offs, ns, rl.targets(target_db), hop=rl.hop if rl.mode else None)
    level, counts, status = rl.launch(flat, jobs)                 # device tensors; the gains go to ev= / tails= when they are given

level='rms': level = (sum of x^2) / n in float64, the target amplitude is 10^(target_db / 20).  level='lufs': level = zbar of
sedt_loudness on the region, bit for bit, and the target amplitude is 10^((target_db + 0.691) / 20), so that the region's loudness
-0.691 + 10 log10(g^2 zbar) comes out at target_db.  g = float32(target / sqrt(level)).  Status 1: the level is 0 (silence, or every
block under the absolute gate) or not finite - the records keep the gains the host wrote; status 2: the device refused the record.

``relevel_jobs`` and ``target_amplitude`` are the host half and need no GPU."""
import numpy as np
import torch

from .. import lib as L
from . import loudness as LD
from .transforms import PinnedRing

# the device record (include/sedt_hip.h: SedtRelevelJob 40 bytes; sedt_sizeof 19)
JOB = np.dtype([('off', '<i8'), ('n', '<i8'), ('target', '<f8'), ('ev', '<i4'), ('tail', '<i4'), ('ws_off', '<i8')])
SIZEOF = {19: JOB}
MODES = {'rms': 0, 'lufs': 1}
STATUS_REASONS = {1: 'the region is silent, lies under the absolute gate in every block or holds non-finite samples: the gain is left as it was',
                  2: 'the record does not lie inside the bank, the record tables or the workspace, or its target is not a finite number > 0'}


def check_sizes():
    """the record dtype against the library that is loaded (sedt_sizeof); raises on drift"""
    for which, dt in SIZEOF.items():
        got = L.load().sedt_sizeof(which)
        if got != dt.itemsize:
            raise RuntimeError(f'utilities/relevel.py: record {which} has {dt.itemsize} bytes here, {got} in the library')


def target_amplitude(target_db, level='rms'):
    """float64: the amplitude a region at ``target_db`` has - 10^(dB / 20) of its RMS, or 10^((LUFS + 0.691) / 20) of the root of its
    gated mean square zbar, since L = -0.691 + 10 log10(zbar)"""
    if level not in MODES:
        raise ValueError(f"relevel: level {level!r} is neither 'rms' nor 'lufs'")
    db = np.asarray(target_db, np.float64) + (np.float64(0.691) if level == 'lufs' else np.float64(0.0))
    return np.float64(10.0) ** (db / np.float64(20.0))


def job_doubles(n, hop):
    """the float64 words of workspace one job owns: n // hop + 1 hop energies under BS.1770 (hop given), none for the RMS (hop None)"""
    return 0 if hop is None else int(n) // int(hop) + 1


def relevel_jobs(offs, ns, targets, ev=None, tails=None, hop=None):
    """the JOB records of E regions flat[offs[e] : offs[e] + ns[e]] and the doubles of workspace they need.  targets: the amplitude each
    region shall have (``target_amplitude``); ev / tails: the index of the event / tail record that takes each gain (default -1: none);
    hop: the 100 ms hop in samples under BS.1770, None for the RMS"""
    E = len(ns)
    if len(offs) != E or len(targets) != E or (ev is not None and len(ev) != E) or (tails is not None and len(tails) != E):
        raise ValueError('relevel_jobs: one offset, one length, one target (and one record index) per region')
    offs, ns = np.asarray(offs, np.int64).reshape(-1), np.asarray(ns, np.int64).reshape(-1)
    targets = np.asarray(targets, np.float64).reshape(-1)
    bad = np.flatnonzero((ns < 1) | (offs < 0))
    if len(bad):
        e = int(bad[0])
        raise ValueError(f'relevel_jobs: region {e} (offset {int(offs[e])}, {int(ns[e])} samples): offset >= 0, at least one sample')
    bad = np.flatnonzero(~((targets > 0.0) & (targets < np.inf)))                       # (NaN fails)
    if len(bad):
        raise ValueError(f'relevel_jobs: region {int(bad[0])} has target {float(targets[bad[0]])!r}: not a finite amplitude > 0')
    jobs = np.zeros(E, JOB)
    jobs['off'], jobs['n'], jobs['target'] = offs, ns, targets
    jobs['ev'] = -1 if ev is None else np.asarray(ev, np.int64)
    jobs['tail'] = -1 if tails is None else np.asarray(tails, np.int64)
    own = np.zeros(E, np.int64) if hop is None else ns // int(hop) + 1
    jobs['ws_off'] = np.cumsum(own) - own                            # the regions behind one another, in job order
    return jobs, int(own.sum())


class DeviceRelevel(object):
    """sr: the sample rate of what is measured (it fixes the K-weighting and the hop); level: 'rms' or 'lufs'.  A call is one launch
    and reads nothing back."""

    def __init__(self, sr, level='rms', device='cuda'):
        if level not in MODES:
            raise ValueError(f"DeviceRelevel: level {level!r} is neither 'rms' nor 'lufs'")
        self.sr, self.level, self.mode = int(sr), level, MODES[level]
        self.hop = LD.hop_samples(sr)
        self.dev = torch.device(device)
        check_sizes()
        self._consts = torch.from_numpy(np.concatenate([LD.k_weighting(sr), LD.hop_map(sr).reshape(-1)])).to(self.dev)
        self._ring, self._ws = None, None

    def targets(self, target_db):
        return target_amplitude(target_db, self.level)

    def jobs(self, offs, ns, target_db, ev=None, tails=None):
        """relevel_jobs with this object's level: targets from dB / LUFS, the workspace regions of its mode"""
        return relevel_jobs(offs, ns, self.targets(target_db), ev, tails, self.hop if self.mode else None)

    def workspace(self, doubles):
        """a float64 device tensor of at least ``doubles`` elements, owned by this object and reused (grown when a call needs more)"""
        if self._ws is None or self._ws.numel() < doubles:
            self._ws = torch.empty(max(int(doubles), 1), dtype=torch.float64, device=self.dev)
        return self._ws

    def outputs(self, E):
        """fresh zeroed (level float64 [E], counts int32 [E, 4], status int32 [E]) device tensors (at least one row)"""
        E = max(int(E), 1)
        return (torch.zeros(E, dtype=torch.float64, device=self.dev), torch.zeros((E, 4), dtype=torch.int32, device=self.dev),
                torch.zeros(E, dtype=torch.int32, device=self.dev))

    def launch(self, flat, jobs, ev=None, n_ev=0, tails=None, n_tails=0, workspace=None, jobs_dev=None, out=None, flat_len=None):
        """the raw stage: ``jobs`` (a host JOB array) over the f32 device tensor ``flat``.  ev / tails: the DEVICE records (uint8 tensors
        holding n_ev SedtScapeEvent / n_tails SedtReverbTail) whose gains are rewritten, or None; workspace: float64, the caller's, else
        this object's; jobs_dev: the same records on the device (uint8), else they travel through this object's pinned ring; out:
        (level float64 [E], counts int32 [E, 4], status int32 [E]) to write into, else fresh tensors.  Returns them (on the device;
        nothing is read back)."""
        jobs = np.ascontiguousarray(jobs, JOB)
        E = int(jobs.shape[0])
        if flat.dtype != torch.float32 or not flat.is_contiguous() or not flat.is_cuda:
            raise ValueError('DeviceRelevel.launch: flat is a contiguous f32 device tensor')
        need = int(jobs['ws_off'][-1]) + job_doubles(jobs['n'][-1], self.hop if self.mode else None) if E else 0
        if workspace is None:
            workspace = self.workspace(need)
        if workspace.dtype != torch.float64 or not workspace.is_contiguous() or not workspace.is_cuda:
            raise ValueError('DeviceRelevel.launch: workspace is a contiguous float64 device tensor')
        if out is None:
            out = self.outputs(E)
        level, counts, status = out
        if jobs_dev is None:
            if self._ring is None:
                self._ring = PinnedRing(self.dev)
            jobs_dev = self._ring.upload(jobs.view(np.uint8).reshape(-1) if E else np.zeros(8, np.uint8))
        host = jobs if E else np.zeros(1, JOB)
        L.check(L.load().sedt_relevel(L.p(flat), flat.numel() if flat_len is None else int(flat_len), host.ctypes.data, L.p(jobs_dev), E,
                                      self.mode, L.p(self._consts), L.p(self._consts[10:]), self.hop, LD.Z_ABS, L.p(workspace),
                                      workspace.numel(), None if ev is None else L.p(ev), int(n_ev), None if tails is None else L.p(tails),
                                      int(n_tails), L.p(level), L.p(counts), L.p(status), L.stream_ptr()), 'relevel')
        return level, counts, status

    @staticmethod
    def check(status, who='DeviceRelevel'):
        """raise on a non-zero status (reads them back)"""
        st = status.cpu().numpy()
        bad = np.flatnonzero(st)
        if len(bad):
            raise RuntimeError(f'{who}: region {int(bad[0])}: status {int(st[bad[0]])}: {STATUS_REASONS[int(st[bad[0]])]}')
