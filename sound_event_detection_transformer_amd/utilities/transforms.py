"""Input-side feature transforms on the device - counterpart of reference utilities/BoxTransforms.py (get_transforms,
:454-490) for the transforms the training drivers enable: ApplyLog, PadOrTrunc, TimeMask, FreqMask(fill "mean"), FreqShift,
ToTensor(unsqueeze_axis=0), Normalize(scaler).

The reference runs them per clip in NumPy inside the DataLoader workers; at > 10 k clips/s per GPU that cannot feed the step.
Here a whole batch is ONE kernel launch (sedt_box_transform: a workgroup per clip, the clip stays in LDS between the passes).
The RANDOM PARAMETERS are drawn on the host with np.random in exactly the order the reference's classes draw them
(TimeMask.randomize_parameters :380-383, FreqMask :410-413, FreqShift :437-443), so a seeded run augments every clip the same
way as the reference pipeline does.  DeviceViewTransform (sedt_box_transform_views) is the paired form for the mean-teacher
recipe: both views from one raw clip, the student's Gaussian noise drawn inside the kernel."""
import numpy as np
import torch

from .. import lib as L

_AUG = np.dtype([('nframes_raw', np.int32), ('tm_t', np.int32), ('tm_t0', np.int32), ('fm_f', np.int32), ('fm_f0', np.int32),
                 ('fm_on', np.int32), ('fs_shift', np.int32), ('pad', np.int32)])


def stage_clips(clips, n_mels, dev, staging=None):
    """a batch of raw clips on the device, for DeviceBoxTransform, DeviceViewTransform and utilities.scaler.Scaler alike.  clips: a
    (B, T_raw, n_mels) tensor already on the device, or a list of ragged (T_raw, n_mels) arrays / tensors, which go through a pinned
    buffer (``staging``, or a fresh one).  Returns (amp (B, stride, n_mels) f32 on the device, B, stride, rows per clip)."""
    if torch.is_tensor(clips) and clips.is_cuda:
        amp = clips.float().contiguous()
        B, stride = amp.shape[0], amp.shape[1]
        return amp, B, stride, [stride] * B
    B = len(clips)
    nraw = [int(c.shape[0]) for c in clips]
    stride = max(nraw)
    host = staging if staging is not None else torch.zeros((B, stride, n_mels), dtype=torch.float32).pin_memory()
    hv = host.numpy()
    for i, c in enumerate(clips):                       # plain memcpys into the pinned buffer (rows >= nraw[i] are never read)
        hv[i, :nraw[i]] = c.numpy() if torch.is_tensor(c) else c
    return host.to(dev, non_blocking=True), B, stride, nraw


def _rows(nraw, nframes, stride):
    """the rows per clip of a staged batch: ``nframes`` where the caller gives them, else what stage_clips found"""
    if nframes is None:
        return nraw
    nframes = [int(n) for n in nframes]
    if len(nframes) != len(nraw) or min(nframes, default=0) < 0 or max(nframes, default=0) > stride:
        raise ValueError('nframes: one row count per clip, within the rows of the batch')
    return nframes


class PinnedRing(object):
    """small per-batch records (bytes) through a ring of PINNED staging buffers: a copy from pageable memory blocks the host until
    everything queued before it has run - the host would lose its run-ahead over the GPU on every batch (measured on the C5
    step: 8.25 -> 8.65 ms)"""

    def __init__(self, dev):
        self.dev, self.pin, self.ev, self.devbuf, self.k = dev, [], [], [], 0

    def upload(self, raw):
        n = raw.size
        if not self.pin or self.pin[0].numel() < n:
            self.pin = [torch.zeros(max(n, 4096), dtype=torch.uint8).pin_memory() for _ in range(4)]
            self.devbuf = [torch.zeros(max(n, 4096), dtype=torch.uint8, device=self.dev) for _ in range(4)]
            self.ev = [None] * 4
        k = self.k
        self.k = (k + 1) % 4
        if self.ev[k] is not None:
            self.ev[k].synchronize()
        self.pin[k].numpy()[:n] = raw
        self.devbuf[k][:n].copy_(self.pin[k][:n], non_blocking=True)
        self.ev[k] = torch.cuda.Event()
        self.ev[k].record()
        return self.devbuf[k]


class DeviceBoxTransform(object):
    """frames: fixed number of frames (config.max_frames); scaler_mean / scaler_std: per-mel float64 vectors of the dataset
    Scaler (None: no normalisation); time_mask / freq_mask / freq_shift: enable the augmentations (their constructor
    defaults are the reference's: TimeMask(0.0, 0.1, p=0.2), FreqMask(0.03, 0.4, fill "mean", p=0.5), FreqShift(p=0.5,
    max_band=4, std=2)); apply_log=False takes inputs that are already in dB; scaler: a fitted or loaded utilities.scaler.Scaler,
    equal to passing its mean_ and std_ as scaler_mean / scaler_std (one form or the other)."""

    def __init__(self, frames, scaler_mean=None, scaler_std=None, time_mask=False, freq_mask=False, freq_shift=False,
                 apply_log=True, n_mels=64, device='cuda', tm=(0.0, 0.1, 0.2), fm=(0.03, 0.4, 0.5), fs=(0.5, 4, 0.0, 2.0), scaler=None):
        if scaler is not None:
            if scaler_mean is not None or scaler_std is not None:
                raise ValueError('pass the statistics either as scaler= or as scaler_mean= / scaler_std=, not both')
            if getattr(scaler, 'mean_', None) is None or getattr(scaler, 'std_', None) is None:
                raise ValueError('scaler= needs a fitted or loaded Scaler (mean_ and std_ are not set)')
            scaler_mean, scaler_std = scaler.mean_, scaler.std_
        self.frames, self.F, self.dev = frames, n_mels, torch.device(device)
        self.time_mask, self.freq_mask, self.freq_shift, self.apply_log = time_mask, freq_mask, freq_shift, apply_log
        self.tm, self.fm, self.fs = tm, fm, fs
        self.mean = self.std = None
        if scaler_mean is not None:
            self.mean = torch.as_tensor(np.asarray(scaler_mean, np.float64)).to(self.dev)
            self.std = torch.as_tensor(np.asarray(scaler_std, np.float64)).to(self.dev)

    def _upload(self, raw):
        """the per-clip parameter records through this transform's ring of pinned staging buffers (PinnedRing)"""
        ring = self.__dict__.get('_ring')
        if ring is None:
            ring = self._ring = PinnedRing(self.dev)
        return ring.upload(raw)

    def draw(self, nframes_raw):
        """one record of augmentation parameters for a clip, consuming np.random like the reference's transform objects"""
        r = np.zeros((), _AUG)
        r['nframes_raw'] = nframes_raw
        nf, nm = self.frames, self.F
        if self.time_mask:
            lo, hi, p = self.tm
            apply = np.random.uniform(0, 1) < p
            t = np.random.uniform(lo, hi)
            t0 = np.random.uniform(0, 1 - t)
            if apply:
                r['tm_t'], r['tm_t0'] = int(t * nf), int(t0 * nf)
        if self.freq_mask:
            lo, hi, p = self.fm
            apply = np.random.uniform(0, 1) < p
            f = np.random.uniform(lo, hi)
            f0 = np.random.uniform(0, 1 - f)
            if apply:
                r['fm_on'], r['fm_f'], r['fm_f0'] = 1, int(f * nm), int(f0 * nm)
        if self.freq_shift:
            p, max_band, mean, std = self.fs
            apply = np.random.uniform(0, 1) < p
            s = int(np.random.normal(mean, std))
            while abs(s) > max_band:
                s = int(np.random.normal(mean, std))
            if apply:
                r['fs_shift'] = s
        return r

    def draw_batch(self, nraws):
        """the records of a batch: the same np.random calls in the same order as draw() clip by clip, without a structured-array
        scalar per clip (64 clips: 1.4 ms -> 0.2 ms of host time per batch)"""
        rows = []
        u, nrm = np.random.uniform, np.random.normal
        nf, nm = self.frames, self.F
        for n in nraws:
            tm_t = tm_t0 = fm_f = fm_f0 = fm_on = fs = 0
            if self.time_mask:
                lo, hi, p = self.tm
                apply = u(0, 1) < p
                t = u(lo, hi)
                t0 = u(0, 1 - t)
                if apply:
                    tm_t, tm_t0 = int(t * nf), int(t0 * nf)
            if self.freq_mask:
                lo, hi, p = self.fm
                apply = u(0, 1) < p
                f = u(lo, hi)
                f0 = u(0, 1 - f)
                if apply:
                    fm_on, fm_f, fm_f0 = 1, int(f * nm), int(f0 * nm)
            if self.freq_shift:
                p, max_band, mean, std = self.fs
                apply = u(0, 1) < p
                s_ = int(nrm(mean, std))
                while abs(s_) > max_band:
                    s_ = int(nrm(mean, std))
                if apply:
                    fs = s_
            rows.append((n, tm_t, tm_t0, fm_f, fm_f0, fm_on, fs, 0))
        return np.asarray(rows, np.int32).view(_AUG).reshape(-1)

    def __call__(self, clips, params=None, out=None, staging=None, nframes=None):
        """clips: list of (T_raw, n_mels) float arrays / tensors (mel amplitudes), or a (B, T_raw, n_mels) tensor already on
        the device.  params: optional structured array of _AUG records (else drawn).  nframes: the rows each clip of a device
        tensor really has (else T_raw) - what DeviceMelSpectrogram returns beside its batch.  Returns (B, 1, frames, n_mels) f32."""
        amp, B, stride, nraw = stage_clips(clips, self.F, self.dev, staging)
        nraw = _rows(nraw, nframes, stride)
        if params is None:
            params = self.draw_batch(nraw)
        params = np.ascontiguousarray(params)
        aug = self._upload(params.view(np.uint8).reshape(-1))
        if out is None:
            out = torch.empty((B, 1, self.frames, self.F), device=self.dev, dtype=torch.float32)
        L.check(L.load().sedt_box_transform(L.p(amp), stride, L.p(aug), L.p(self.mean), L.p(self.std), B, self.frames, self.F,
                                            int(self.apply_log), 1, 0.0, L.p(out), L.stream_ptr()), 'box_transform')
        return out


# ------------------------------------------------------------------------------------------------ the two mean-teacher views
_VAUG = np.dtype([('view', _AUG, (2,)), ('noise_on', np.int32), ('pad', np.int32)])      # SedtViewAug (include/sedt_hip.h)


class DeviceViewTransform(DeviceBoxTransform):
    """The noisy chain of the semi-supervised recipe (reference train_ss_sedt.py:87-97: get_transforms(noise_dict_params={"mean": 0.,
    "snr": noise_snr}, freq_mask, freq_shift, time_mask)) for a whole batch in ONE launch (sedt_box_transform_views): a raw clip goes
    in once and BOTH views come out - view 0 for the labelled pass and the teacher, view 1 (AugmentGaussianNoise with probability
    ``noise_p``, BoxTransforms.py:121-180, then TimeMask, which skips view 0) for the student; FreqMask / FreqShift hit each view with
    a draw of its own, as Transform._apply_transform (:19-35) does.

    ``draw_batch`` consumes np.random in the reference's order, clip by clip: noise ``uniform(0, 1) < p``; (mode 'host' only, and
    only when applied) the (T_raw, F) normals; TimeMask's three draws for view 1; FreqMask's three for view 0, then for view 1;
    FreqShift's for view 0, then for view 1.

    noise='host': the normals are drawn with np.random on the host and uploaded (the kernel's injected source), so a seeded run
    reproduces a seeded reference pipeline draw for draw.  They are STANDARD normals - ``np.random.normal(0, std, shape)`` is
    ``std * `` the same Gaussian stream, and the kernel does the scaling by the band std it computes itself - so the draw needs only
    the clips' lengths, not their data.
    noise='device' (the default): the normals never exist on the host; the kernel draws them from its counter-based stream
    (``seed``, plus ``self.offset``, which every call advances by the elements of its batch).  The LATER host draws of a seeded
    run then differ from the reference's: there the normals advance the same np.random generator the masks draw from.

    The reference's other branch (``std=`` instead of ``snr=``, :172-173, which ignores the value and adds |N(0, 0.25^2)|) is not
    part of the recipe and is not built: ``noise_snr=None`` raises."""

    def __init__(self, frames, scaler_mean=None, scaler_std=None, noise_snr=30.0, noise_p=0.5, time_mask=False, freq_mask=False,
                 freq_shift=False, noise='device', seed=0, noise_std=None, **kw):
        if noise_snr is None or noise_std is not None:
            raise ValueError("DeviceViewTransform builds the snr branch of AugmentGaussianNoise only: the recipe passes "
                             "{'mean': 0., 'snr': noise_snr}; the std= branch (reference BoxTransforms.py:172-173) is not part of it")
        if noise not in ('device', 'host'):
            raise ValueError(f"noise must be 'device' or 'host', not {noise!r}")
        super().__init__(frames, scaler_mean, scaler_std, time_mask=time_mask, freq_mask=freq_mask, freq_shift=freq_shift, **kw)
        if self.F % 2:
            raise ValueError('the normals come in pairs: n_mels must be even')
        self.noise_snr, self.noise_p, self.noise, self.seed = float(noise_snr), float(noise_p), noise, int(seed) & 0xffffffff
        self.seed_ptr = None              # optional device uint32 word added to the seed (a step that advances its own seed word)
        self.offset = 0                   # stream position of the next call's first element (drawn mode)

    def draw_batch(self, nraws):
        """(records, normals): the _VAUG records of a batch and - mode 'host' - per clip the (T_raw, F) float64 standard normals of
        its noise (None where the noise is not applied); normals is None in mode 'device'"""
        u, nrm = np.random.uniform, np.random.normal
        nf, nm = self.frames, self.F
        rows, normals = [], ([] if self.noise == 'host' else None)
        for n in nraws:
            noise_on = int(u(0, 1) < self.noise_p)
            if normals is not None:
                normals.append(nrm(0.0, 1.0, (n, nm)) if noise_on else None)
            tm_t = tm_t0 = 0
            if self.time_mask:                                   # view 1 only
                lo, hi, p = self.tm
                apply = u(0, 1) < p
                t = u(lo, hi)
                t0 = u(0, 1 - t)
                if apply:
                    tm_t, tm_t0 = int(t * nf), int(t0 * nf)
            fm = [(0, 0, 0), (0, 0, 0)]
            if self.freq_mask:
                lo, hi, p = self.fm
                for k in (0, 1):
                    apply = u(0, 1) < p
                    f = u(lo, hi)
                    f0 = u(0, 1 - f)
                    if apply:
                        fm[k] = (int(f * nm), int(f0 * nm), 1)
            fs = [0, 0]
            if self.freq_shift:
                p, max_band, mean, std = self.fs
                for k in (0, 1):
                    apply = u(0, 1) < p
                    s_ = int(nrm(mean, std))
                    while abs(s_) > max_band:
                        s_ = int(nrm(mean, std))
                    if apply:
                        fs[k] = s_
            rows.append((n, 0, 0) + fm[0] + (fs[0], 0) + (n, tm_t, tm_t0) + fm[1] + (fs[1], 0) + (noise_on, 0))
        return np.asarray(rows, np.int32).reshape(-1, 18).view(_VAUG).reshape(-1), normals

    def __call__(self, clips, params=None, out=None, staging=None, normals=None, nframes=None):
        """clips, staging, nframes: as DeviceBoxTransform.  params: optional _VAUG records (else drawn).  normals: the injected standard
        normals, a list of per-clip (T_raw, F) arrays (None entries allowed) or a (B, stride, F) f32 device tensor; None with params
        given, or in mode 'device', makes the kernel draw them.  out: optional pair of (B, 1, frames, F) f32 tensors.
        Returns (x_teacher, x_student)."""
        amp, B, stride, nraw = stage_clips(clips, self.F, self.dev, staging)
        nraw = _rows(nraw, nframes, stride)
        if params is None:
            params, normals = self.draw_batch(nraw)
        params = np.ascontiguousarray(params)
        if params.dtype != _VAUG or len(params) != B or int(params['view']['nframes_raw'].max(initial=0)) > stride:
            raise ValueError('params: one _VAUG record per clip, nframes_raw within the rows of the batch')
        z = None
        if torch.is_tensor(normals):
            z = normals.to(self.dev).float().contiguous()
            assert tuple(z.shape) == (B, stride, self.F), 'injected normals are laid out like the raw batch'
        elif normals is not None:
            zh = torch.zeros((B, stride, self.F), dtype=torch.float32).pin_memory()
            for i, n in enumerate(normals):
                if n is not None:
                    zh.numpy()[i, :len(n)] = n
            z = zh.to(self.dev, non_blocking=True)
        aug = self._upload(params.view(np.uint8).reshape(-1))
        if out is None:
            out = (torch.empty((B, 1, self.frames, self.F), device=self.dev, dtype=torch.float32),
                   torch.empty((B, 1, self.frames, self.F), device=self.dev, dtype=torch.float32))
        x0, x1 = out
        L.check(L.load().sedt_box_transform_views(L.p(amp), stride, L.p(aug), L.p(self.mean), L.p(self.std), B, self.frames, self.F,
                                                  int(self.apply_log), 1, 0.0, self.noise_snr, L.p(z), self.seed, L.p(self.seed_ptr),
                                                  self.offset, L.p(x0), L.p(x1), L.stream_ptr()), 'box_transform_views')
        if z is None:
            self.offset += B * stride * self.F
        return x0, x1


# ------------------------------------------------------------------------------------------------ SP-SEDT query patches
_JOB = np.dtype([('clip', np.int32), ('s_idx', np.int32), ('e_idx', np.int32), ('pad', np.int32)])


def random_patch_boxes(t, num_patches, mu=0.2, sigma=0.26, fixed_patch_size=False):
    """the (centre, length) patch boxes of one clip of ``t`` frames, drawn with np.random in the reference's order
    (data_utils/DataLoad.py:57-77, DataLoadDf.get_random_patch: 5 P normal lengths filtered to [0.05, 0.8), then one integer
    centre per kept length)"""
    if fixed_patch_size:
        l = np.asarray([128 / t] * num_patches)
    else:
        l = mu + sigma * np.random.randn(5 * num_patches)
        l = l[[0.05 <= i < 0.8 for i in l]][:num_patches]
    c = [np.random.randint(int(t * i / 2) + 1, int(t * (1 - i / 2))) / t for i in l]
    s, e = (c - l / 2) * t, (c + l / 2) * t
    s = [int(i) for i in s]
    e = [i + 128 for i in s] if fixed_patch_size else [int(i) for i in e]
    return [[(i + j) / (2 * t), (j - i) / t] for i, j in zip(s, e)]


class DeviceQuery(object):
    """reference utilities/BoxTransforms.py:315-360 (``Query``, the last transform of the SP-SEDT pipeline) for a whole batch in
    ONE launch: every box of every clip is cropped from the transformed clip, min-max normalised, quantised to 8 bits, resized
    to (128, F) with Pillow's bilinear arithmetic and de-normalised - bit-identical to the reference's PIL round trip
    (sedt_query_patches).  The row range of a box is computed on the host exactly as the reference does (float32 box values,
    ``int(s * t)``)."""

    def __init__(self, fixed_patch_size=False):
        self.fixed = bool(fixed_patch_size)

    def rows(self, box, t):
        c, l = np.float32(box[0]), np.float32(box[1])
        s, e = c - l / 2, c + l / 2
        s_idx, e_idx = int(s * t), int(e * t)
        if self.fixed:
            e_idx = min(t, s_idx + 128)
            s_idx = e_idx - 128
        elif s_idx >= e_idx:                                   # make sure the patch is not empty
            s_idx, e_idx = max(0, s_idx - 1), min(t, e_idx + 1)
        return s_idx, e_idx

    def __call__(self, data, boxes):
        """data (B, 1, T, F) f32 on the GPU (output of DeviceBoxTransform), boxes: per clip a (P, 2) array / tensor of (centre,
        length).  Returns patches (B, P, 1, 128, F) f32 - what the reference's collate stacks from ``label['patches']``."""
        if not data.is_cuda:
            raise RuntimeError('DeviceQuery runs on the MI355X HIP path only (no CPU fallback)')
        B, _, T, F = data.shape
        data = data.contiguous().float()
        P = len(boxes[0])
        bx = np.stack([(b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)).astype(np.float32) for b in boxes])
        assert bx.shape == (B, P, 2), 'every clip carries the same number of (centre, length) patch boxes'
        # the whole batch at once, in the float32 arithmetic of rows() (= the reference's box.numpy() scalars)
        c, l = bx[..., 0], bx[..., 1]
        half = l / np.float32(2)
        s_idx = ((c - half) * np.float32(T)).astype(np.int64)
        e_idx = ((c + half) * np.float32(T)).astype(np.int64)
        if self.fixed:
            e_idx = np.minimum(T, s_idx + 128)
            s_idx = e_idx - 128
        else:
            empty = s_idx >= e_idx                                      # make sure the patch is not empty
            s_idx = np.where(empty, np.maximum(0, s_idx - 1), s_idx)
            e_idx = np.where(empty, np.minimum(T, e_idx + 1), e_idx)
        bad = ~((0 <= s_idx) & (s_idx < e_idx) & (e_idx <= T)) | (self.fixed & (e_idx - s_idx != 128))
        if bad.any():
            b, k = np.argwhere(bad)[0]
            raise ValueError(f'patch box {bx[b, k].tolist()} gives rows [{s_idx[b, k]}, {e_idx[b, k]}) outside a clip of {T} frames')
        jobs = np.zeros((B * P,), _JOB)
        jobs['clip'] = np.repeat(np.arange(B, dtype=np.int32), P)
        jobs['s_idx'], jobs['e_idx'] = s_idx.reshape(-1), e_idx.reshape(-1)
        jd = torch.from_numpy(jobs.view(np.int32)).to(data.device, non_blocking=True)
        out = torch.empty((B, P, 1, 128, F), device=data.device, dtype=torch.float32)
        L.check(L.load().sedt_query_patches(data.data_ptr(), B, T, F, jd.data_ptr(), B * P, int(self.fixed), out.data_ptr(),
                                            L.stream_ptr()), 'query_patches')
        return out
