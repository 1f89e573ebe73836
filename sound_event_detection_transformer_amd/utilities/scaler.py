"""The dataset feature Scaler, fitted on the device - counterpart of reference utilities/Scaler.py (``Scaler``), with its public
names, so the drivers' lines (train_sedt.py:169-190, train_spsedt.py:82-102, train_ss_sedt.py:68-84) port one to one:

    scaler = Scaler(frames)                         # reference: Scaler()
    if os.path.isfile(path): scaler.load(path)
    else: scaler.calculate_scaler(batches); scaler.save(path)
    transform = DeviceBoxTransform(frames, scaler=scaler, ...)      # reference: Normalize(scaler), the last link of get_transforms

The reference walks the training set clip by clip through get_transforms(frames) (ApplyLog -> PadOrTrunc -> ToTensor) and adds, per
clip, two float64 band means - of the features and of their f32 squares - in a Python loop.  Here a whole batch of RAW clips is one
call of sedt_scaler_update: pass 1 of the transform kernel (dB, clip maximum, 80 dB floor, the clip in LDS) followed by the band sums,
so the statistics are by construction those of the features sedt_box_transform later normalises.  The accumulators ([2][n_mels]
float64 sums of the per-clip means, and the clip count) stay on the device; ``finalize()`` is the only read-back.  The clips are added
in the order they are fed and nothing is added atomically: the same sequence of clips gives the same bits however it is cut into
batches.

The JSON is the reference's ({"mean_": [...], "mean_of_square_": [...]}): a file written by either side loads in the other.
``std_ = sqrt(mean_of_square_ - mean_ ** 2)`` on the host in float64, the reference's formula."""
import json

import numpy as np
import torch

from .. import lib as L
from .transforms import PinnedRing, stage_clips


def _is_batch(x):
    """a batch of clips (a list of 2-D clips, or a 3-D array / tensor), as opposed to one 2-D clip"""
    return isinstance(x, (list, tuple)) or (hasattr(x, 'ndim') and x.ndim == 3)


class Scaler(object):
    """frames: the fixed number of frames the transforms pad or truncate to (config.max_frames) - needed to fit, not to load;
    apply_log=False takes inputs that are already in dB.  ``mean_``, ``mean_of_square_``, ``std_``: float64 NumPy arrays once
    computed or loaded.  ``sum_`` ([2][n_mels]) and ``count_`` are what the device accumulated (None after a load: a JSON file does
    not say how many clips it stands for)."""

    def __init__(self, frames=None, n_mels=64, apply_log=True, device='cuda'):
        self.frames, self.F, self.apply_log, self.dev = frames, n_mels, apply_log, torch.device(device)
        self.mean_ = self.mean_of_square_ = self.std_ = None
        self.sum_, self.count_ = None, None
        self._acc = self._count = self._stats = self._ring = None

    # ------------------------------------------------------------------------------------------------ the fit
    def reset(self):
        """forget what was accumulated (the next update starts a new fit)"""
        self._acc = self._count = None
        return self

    def update(self, clips, nframes=None):
        """add one batch: what DeviceBoxTransform.__call__ takes - a list of ragged (T_raw, n_mels) arrays / tensors of mel
        amplitudes, or a (B, T_raw, n_mels) tensor already on the device, whose clips then count as T_raw rows long unless
        ``nframes`` gives the rows of each.  One launch of sedt_scaler_update; nothing is read back."""
        if self.frames is None:
            raise ValueError('Scaler(frames=...) is needed to fit: the statistics are those of the padded / truncated clips')
        if torch.is_tensor(clips) and not clips.is_cuda or isinstance(clips, np.ndarray):
            clips = list(clips)                                  # a host (B, T_raw, n_mels) block: its clips
        amp, B, stride, nraw = stage_clips(clips, self.F, self.dev)
        if B == 0:
            return self
        if amp.dim() != 3 or amp.shape[2] != self.F:
            raise ValueError(f'clips of {self.F} mel bands expected, got a batch of shape {tuple(amp.shape)}')
        if nframes is not None:
            nraw = [int(n) for n in nframes]
        if len(nraw) != B or min(nraw) < 0 or max(nraw) > stride:
            raise ValueError('nframes: one row count per clip, within the rows of the batch')
        if self._acc is None:
            self._acc = torch.zeros((2, self.F), dtype=torch.float64, device=self.dev)
            self._count = torch.zeros((1,), dtype=torch.int64, device=self.dev)
        if self._stats is None or self._stats.shape[0] < B:
            self._stats = torch.empty((B, 2, self.F), dtype=torch.float64, device=self.dev)
        if self._ring is None:
            self._ring = PinnedRing(self.dev)
        nf = self._ring.upload(np.asarray(nraw, np.int32).view(np.uint8))
        L.check(L.load().sedt_scaler_update(L.p(amp), stride, L.p(nf), B, self.frames, self.F, int(self.apply_log), L.p(self._stats),
                                            L.p(self._acc), L.p(self._count), L.stream_ptr()), 'sedt_scaler_update')
        return self

    def finalize(self):
        """the one read-back: the device sums and the count become sum_, count_, mean_, mean_of_square_ and std_"""
        if self._acc is None:
            raise RuntimeError('finalize() before any update(): there is nothing to read back')
        self.sum_ = self._acc.cpu().numpy().copy()
        self.count_ = int(self._count.cpu()[0])
        return self._from_sums()

    def _from_sums(self):
        self.mean_ = self.sum_[0] / self.count_
        self.mean_of_square_ = self.sum_[1] / self.count_
        self.std_ = self.std(self.variance(self.mean_, self.mean_of_square_))
        return self

    @classmethod
    def from_sums(cls, sums, count, **kw):
        """a Scaler from accumulated sums ([2][n_mels] float64: the per-clip band means and means of squares added up) and the
        number of clips, e.g. what another rank gathered"""
        sums = np.array(sums, np.float64)
        if sums.ndim != 2 or sums.shape[0] != 2 or int(count) < 1:
            raise ValueError('sums is [2][n_mels], count >= 1')
        sc = cls(n_mels=sums.shape[1], **kw)
        sc.sum_, sc.count_ = sums, int(count)
        return sc._from_sums()

    def merge(self, other):
        """add what ``other`` was fitted on (each rank or worker fits its shard, then the shards are merged): host arithmetic on the
        [2][n_mels] sums and the counts.  The shards' sums are added as wholes, so the result equals a single fit over all the clips
        to the rounding of a reordered float64 sum, not bit for bit."""
        if self.sum_ is None or other.sum_ is None:
            raise ValueError('merge needs the sums and counts of both sides: finalize() them first (a Scaler loaded from JSON has none)')
        if self.sum_.shape != other.sum_.shape:
            raise ValueError('merge: different numbers of mel bands')
        self.sum_ = self.sum_ + other.sum_
        self.count_ += other.count_
        self._acc = self._count = None
        return self._from_sums()

    def means(self, batches):
        """a fresh fit over ``batches``: an iterable of batches as update() takes them, or of (clips, targets) pairs"""
        self.reset()
        for item in batches:
            if isinstance(item, (tuple, list)) and len(item) == 2 and _is_batch(item[0]):
                item = item[0]
            self.update(item)
        return self.finalize()

    def calculate_scaler(self, batches):
        self.means(batches)
        return self.mean_, self.std_

    # ------------------------------------------------------------------------------------------------ the reference's host side
    def variance(self, mean, mean_of_square):
        return mean_of_square - mean ** 2

    def std(self, variance):
        return np.sqrt(variance)

    def normalize(self, batch):
        """host data only, as the reference: (batch - mean_) / std_ in float64 (a tensor comes back as an f32 tensor).  On the device
        the normalisation is the last step of the transform kernel: DeviceBoxTransform(..., scaler=self)."""
        if torch.is_tensor(batch):
            if batch.is_cuda:
                raise RuntimeError('features on the device are normalised by the transform kernel: DeviceBoxTransform(frames, scaler=scaler)')
            return torch.Tensor((batch.numpy() - self.mean_) / self.std_)
        return (batch - self.mean_) / self.std_

    def state_dict(self):
        if type(self.mean_) is not np.ndarray:
            raise RuntimeError('nothing to save: fit (calculate_scaler) or load first')
        return {"mean_": self.mean_.tolist(), "mean_of_square_": self.mean_of_square_.tolist()}

    def load_state_dict(self, state_dict):
        self.mean_ = np.array(state_dict["mean_"], np.float64)
        self.mean_of_square_ = np.array(state_dict["mean_of_square_"], np.float64)
        self.std_ = self.std(self.variance(self.mean_, self.mean_of_square_))
        self.sum_ = self.count_ = self._acc = self._count = None
        self.F = len(self.mean_)

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.state_dict(), f)

    def load(self, path):
        with open(path, "r") as f:
            self.load_state_dict(json.load(f))
