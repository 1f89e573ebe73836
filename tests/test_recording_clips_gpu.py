"""GPU: sedt_cut_clips (csrc/clips.hip) through utilities.recording_clips.RecordingClips against tests/recording_clips_ref.py, and the
training route it opens.  Everything is exact: waves bit-equal; offsets, labels and status equal; boxes bit-equal in float32.

Shapes: windows of 1003 samples (no multiple of any vector width: every row starts at another alignment) and 4096; starts 0, 1, 2, 3 and
one that runs past the end; a recording shorter than the window; one recording picked twice; B = 1, 5, 65; a clip without events
between two with events; exactly max_targets = 3 survivors, and 4 (status 1, the first three written); one long event that starts
before 200 short ones; two overlapping events of one class; successive cuts into the same buffers, later ones with fewer events."""
import numpy as np
import pytest
import torch

import recording_clips_ref as R
from oracle import sedt_oracle as O

pytestmark = pytest.mark.gpu

SR = 16000
LABELS = [f'c{i}' for i in range(10)]


def _corpus():
    """four recordings at 16 kHz and their annotations; times on the sample grid and off it"""
    gen = np.random.default_rng(7)
    ns = [20000, 700, 30000, 9000]
    names = ['long.wav', 'short.wav', 'dense.wav', 'quiet.wav']
    waves = [gen.standard_normal(n).astype(np.float32) for n in ns]
    s = lambda k: k / SR                                           # second k-th sample starts
    dense = [('c9', 0.01, 1.8)] + [(i % 10, 0.02 + 0.005 * i, 0.022 + 0.005 * i) for i in range(200)]
    ref = {'long.wav': [('c1', s(100), s(400)), ('c2', s(300), s(1003)), ('c2', s(350), s(500)),      # two overlapping events of c2
                        ('c3', s(1003), s(1200)), ('c4', 0.07, 0.11), ('c5', s(4096), s(5000)), ('c6', 0.5, 0.9), ('c0', 1.1, 1.3)],
           'short.wav': [('c7', 0.0, 0.01), ('c8', 0.03, 0.2)],     # the second one ends behind the recording
           'dense.wav': dense,
           'quiet.wav': []}
    return waves, names, ref, ns


# designed picks (recording, start): see the module docstring
PICKS = [(0, 0), (3, 100), (0, 1), (0, 2), (0, 3),                 # a clip without events between clips with events
         (0, 19500), (1, 0), (0, 100), (0, 100), (2, 0),           # past the end; shorter than the window; one pick twice
         (2, 12000), (2, 25000), (0, 1003), (0, 4096), (1, 3), (2, 3201), (3, 8999), (0, 300)]


def _picks(B, lo=0):
    p = [PICKS[(lo + i) % len(PICKS)] for i in range(B)]
    return np.asarray([r for r, _ in p], np.int32), np.asarray([s for _, s in p], np.int64)


@pytest.fixture(scope='module')
def corpus():
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.recording_clips import clip_event_table
    assert torch.cuda.is_available()
    waves, names, ref, ns = _corpus()
    return dict(waves=waves, names=names, ref=ref, ns=ns, mel=DeviceMelSpectrogram.dcase(), table=clip_event_table(ref, LABELS))


def _clips(corpus, window, M, **kw):
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    c = RecordingClips(corpus['mel'], LABELS, window / SR, max_targets=M, **kw)
    assert c.window == window
    return c.add(corpus['waves'], corpus['names'], corpus['ref'])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_cut(corpus, clips, rec, start, min_event_seconds=0.0):
    """one launch against the reference; returns the reference's (targets, status)"""
    from sound_event_detection_transformer_amd.utilities.recording_clips import blob_layout
    B, M, win = len(rec), clips.max_targets, clips.window
    want_wave, want_t, want_st = R.cut_clips(corpus['waves'], corpus['table'], rec, start, win, SR, M, min_event_seconds)
    wave, lengths, dt = clips.cut(rec, start)
    assert wave.shape == (B, win) and np.array_equal(_bits(wave.cpu().numpy()), _bits(want_wave))
    assert lengths == [min(win, corpus['ns'][r] - s) for r, s in zip(rec.tolist(), start.tolist())]
    assert dt.status.cpu().numpy().tolist() == want_st.tolist()
    off, lab, box, (o_lab, o_box, total) = R.blob(want_t, M)
    assert blob_layout(B, M) == (2 * B + 4, o_lab, o_box, total) and dt.blob.numel() == total
    raw = dt.blob.cpu().numpy()
    assert raw[:4 * (2 * B + 4)].view(np.int32).tolist() == off.tolist()
    assert raw[o_lab:o_lab + 8 * len(lab)].view(np.int64).tolist() == lab.tolist()
    assert np.array_equal(raw[o_box:o_box + 8 * len(lab)].view(np.int32), _bits(box.reshape(-1)))
    assert dt.names == [corpus['names'][r] for r in rec]
    return want_t, want_st


@pytest.mark.parametrize('window', [1003, 4096])
@pytest.mark.parametrize('B', [1, 5, 65])
def test_cut_clips_against_the_reference(corpus, window, B):
    clips = _clips(corpus, window, 63)
    seen_events = seen_empty = 0
    for lo in range(0, max(len(PICKS), 2 * B), B):                # successive cuts into the same buffers
        rec, start = _picks(B, lo)
        targets, status = _check_cut(corpus, clips, rec, start)
        assert not status.any()
        seen_events += sum(len(t[0]) > 0 for t in targets)
        seen_empty += sum(len(t[0]) == 0 for t in targets)
    assert seen_events >= 6 and seen_empty >= 2
    # what the designed picks are there for, at this window
    t = lambda r, s: R.clip_targets(corpus['table'], r, s, window, SR, 63)
    assert len(t(3, 100)[0]) == 0 and len(t(0, 0)[0]) > 0 and len(t(0, 1)[0]) > 0          # empty between clips with events
    assert t(0, 0)[0].tolist().count(2) == 2                                               # the overlapping pair of one class
    assert len(t(2, 25000)[0]) == 1 and t(2, 25000)[0][0] == 9                             # only the long event reaches this far
    assert len(t(2, 3201)[0]) > 10 and t(2, 3201)[0][0] == 9                               # the long one first, then the short ones
    assert 19500 + window > corpus['ns'][0] and corpus['ns'][1] < window


def test_cut_clips_random_picks_and_min_event_seconds(corpus):
    clips = _clips(corpus, 4096, 63, min_event_seconds=0.0025)
    np.random.seed(3)
    for B in (65, 64, 7):                                          # the second and third cut carry fewer clips and fewer events
        rec, start = clips.draw(B)
        targets, status = _check_cut(corpus, clips, rec, start, 0.0025)
        assert not status.any()
    plain = R.clip_targets(corpus['table'], 2, 3201, 4096, SR, 63)[0]
    kept = R.clip_targets(corpus['table'], 2, 3201, 4096, SR, 63, 0.0025)[0]
    assert 0 < len(kept) < len(plain)                              # the threshold drops events the plain cut keeps


def test_cut_clips_capacity(corpus):
    """max_targets = 3: a clip with exactly three survivors is complete, one with four raises status 1 and keeps the first three;
    a later cut into the same buffers with fewer events is complete again"""
    clips = _clips(corpus, 1003, 3)
    n = lambda r, s: len(R.clip_targets(corpus['table'], r, s, 1003, SR, 63)[0])
    assert n(0, 0) == 3 and n(0, 100) == 4 and n(0, 1003) == 2 and n(3, 0) == 0 and n(1, 0) == 2
    rec, start = np.asarray([0, 0, 3, 0, 0], np.int32), np.asarray([0, 100, 0, 1003, 100], np.int64)
    targets, status = _check_cut(corpus, clips, rec, start)
    assert status.tolist() == [0, 1, 0, 0, 1] and [len(t[0]) for t in targets] == [3, 3, 0, 2, 3]
    _, _, dt = clips.cut(rec, start)
    with pytest.raises(RuntimeError, match="clip 1 of recording 'long.wav': status 1"):
        dt.to_list()
    with pytest.raises(RuntimeError, match="clip 1 of recording 'long.wav'"):
        dt.check()
    rec, start = np.asarray([3, 0, 3, 1, 3], np.int32), np.asarray([5, 0, 0, 0, 7], np.int64)
    targets, status = _check_cut(corpus, clips, rec, start)
    assert not status.any() and [len(t[0]) for t in targets] == [0, 3, 0, 2, 0]
    lst = clips.cut(rec, start)[2].to_list()
    assert [t['labels'].tolist() for t in lst] == [t[0].tolist() for t in targets]
    assert all(np.array_equal(_bits(a['boxes'].numpy()), _bits(b[1])) for a, b in zip(lst, targets))


def test_add_refusals_and_resampled_staging(corpus):
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector      # noqa: F401 (the shared staging)
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    from sound_event_detection_transformer_amd.utilities.resample import DeviceResampler
    mel = corpus['mel']
    clips = RecordingClips(mel, LABELS, 0.25)
    with pytest.raises(ValueError, match="recording 'x.wav' has no entry in the reference"):
        clips.add([np.zeros(8000, np.float32)], ['x.wav'], {})
    with pytest.raises(ValueError, match=f'shorter than the {mel.min_samples} the front end needs'):
        clips.add([np.zeros(mel.min_samples - 1, np.float32)], ['x.wav'], {'x.wav': []})
    with pytest.raises(ValueError, match='is not one of the 10 labels'):
        clips.add([np.zeros(8000, np.float32)], ['x.wav'], {'x.wav': [('Bird', 0.0, 1.0)]})
    assert len(clips) == 0
    gen = torch.Generator().manual_seed(48)
    stereo = (0.1 * torch.randn(2 * 48000 + 123, 2, generator=gen) * 32768).clamp(-32768, 32767).to(torch.int16).numpy()
    pcm = (0.1 * torch.randn(9000, generator=gen) * 32768).clamp(-32768, 32767).to(torch.int16).numpy()
    clips.add([stereo], ['field.wav'], {'field.wav': [('c1', 0.5, 1.0)]}, sample_rates=48000)
    clips.add([pcm, corpus['waves'][3]], ['pcm.wav', 'quiet.wav'], {'pcm.wav': [], 'quiet.wav': []})      # a second add keeps the first
    want, n = DeviceResampler(48000, SR)([stereo])
    assert n == [-(-len(stereo) // 3)]
    assert torch.equal(clips.wave('field.wav'), want[0, :n[0]]) and clips.wave('field.wav').is_cuda
    assert np.array_equal(clips.wave('pcm.wav').cpu().numpy(), pcm.astype(np.float32) * np.float32(1.0 / 32768.0))
    assert np.array_equal(clips.wave('quiet.wav').cpu().numpy(), corpus['waves'][3])
    with pytest.raises(ValueError, match="recording 'pcm.wav' is staged twice"):
        clips.add([pcm], ['pcm.wav'], {'pcm.wav': []})
    wave, lengths, dt = clips.cut(np.asarray([0, 2], np.int32), np.asarray([8000, 5500], np.int64))
    assert torch.equal(wave[0], want[0, 8000:12000]) and lengths == [4000, 3500]
    assert np.array_equal(wave[1].cpu().numpy(), np.concatenate([corpus['waves'][3][5500:], np.zeros(500, np.float32)]))
    assert [t['labels'].tolist() for t in dt.to_list()] == [[1], []]
    with pytest.raises(ValueError, match='a pick outside its recording'):
        clips.cut(np.asarray([3], np.int32), np.asarray([0], np.int64))
    with pytest.raises(ValueError, match='a pick outside its recording'):
        clips.cut(np.asarray([1], np.int32), np.asarray([9000], np.int64))


# ---------------------------------------------------------------------------------------------------- end to end
def _train_setup(B, seed=5, **step_kw):
    """recordings of 25, 12 and 6 s staged, the smallest model of the stepper tests, a GraphedTrainStep built on a first cut batch"""
    from sound_event_detection_transformer_amd import sedt
    from sound_event_detection_transformer_amd.engine import GraphedTrainStep, build_optimizer
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    gen = torch.Generator().manual_seed(21)
    waves = [0.1 * torch.randn(n, generator=gen).numpy() for n in (25 * SR + 321, 12 * SR + 5, 6 * SR)]
    names = ['a.wav', 'b.wav', 'c.wav']
    ev = np.random.default_rng(4)
    ref = {n: sorted((int(ev.integers(0, 10)), float(t), float(t + ev.uniform(0.3, 4.0))) for t in ev.uniform(0.0, len(w) / SR - 0.5, k))
           for n, w, k in zip(names, waves, (14, 7, 3))}
    mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
    clips = RecordingClips(mel, LABELS, 10.0, max_targets=32).add(waves, names, ref)
    np.random.seed(17)
    x0, dt0 = clips.batch(transform, clips.draw(B))
    example, x0 = dt0.to_list(), x0.clone()
    assert sum(len(t['labels']) for t in example) > 0 and tuple(x0.shape) == (B, 1, 500, 64)
    model, crit, _ = sedt.build_model(sedt.default_args(dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), seed))
    model.cuda().train()
    crit.cuda()
    opt = build_optimizer(model)
    stepper = GraphedTrainStep(model, crit, opt, x0, example, None, slice(B), warmup=1, **step_kw)
    return clips, transform, model, opt, stepper


def _result(out, model):
    total, losses = out
    torch.cuda.synchronize()
    terms = {k: v.detach().clone() for k, v in losses.items()} if isinstance(losses, dict) else {'losses': losses.detach().clone()}
    return total.detach().clone(), terms, [p.detach().clone() for p in model.parameters()]


def test_train_step_on_device_targets_equals_the_list_route(monkeypatch):
    """GraphedTrainStep fed (x, DeviceTargets) == the same stepper restored from its snapshot and fed (x, targets.to_list()): both
    routes fill the same tables and steps are bit-reproducible.  Then engine.train_on_recordings: one cut launch per step, no host
    copy of the tables, no synchronisation inside the loop."""
    from sound_event_detection_transformer_amd import engine, lib, runtime
    runtime.set_compute_dtype('bf16')
    try:
        B = 2
        clips, transform, model, opt, stepper = _train_setup(B)
        x1, dt1 = clips.batch(transform, clips.draw(B))
        x1 = x1.clone()
        snap = engine._snapshot(model, opt)
        slot = stepper.tables._slot
        a = _result(stepper(x1, dt1), model)
        assert stepper.tables._slot == slot                                   # no pinned host slot was used: the device copy
        lst = dt1.to_list()                                                   # (no cut since: the blob still holds this batch)
        assert sum(len(t['labels']) for t in lst) > 0
        engine._restore(model, opt, snap)
        b = _result(stepper(x1, lst), model)
        assert stepper.tables._slot != slot
        assert torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
        assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
        assert any(not torch.equal(p, q) for p, q in zip(a[2], snap['p'])) and bool(torch.isfinite(a[0]).all())
        # ---- the plain loop
        calls = {'sync': 0}
        real = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a_, **k_: (calls.__setitem__('sync', calls['sync'] + 1), real(*a_, **k_))[1])
        slot = stepper.tables._slot
        before = [p.detach().clone() for p in model.parameters()]
        with lib.launch_log() as log:
            total, _ = engine.train_on_recordings(stepper, clips, transform, 3)
        monkeypatch.setattr(torch.cuda, 'synchronize', real)
        assert log['cut_clips'] == 3 and log['mel_spectrogram'] == 3 and calls['sync'] == 0
        assert stepper.tables._slot == slot                                   # no TargetTables host copy
        assert bool(torch.isfinite(total).all()) and any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
        # a clip over capacity is reported once, at the end, with step and recording
        small = type(clips)(clips.mel, LABELS, 10.0, max_targets=32)
        small.add([clips.wave('a.wav')], ['a.wav'], {'a.wav': [(i % 10, 0.1 * i, 0.1 * i + 0.05) for i in range(250)]})
        with pytest.raises(RuntimeError, match=r"train_on_recordings: step 0, clip \d of recording 'a.wav': status 1"):
            engine.train_on_recordings(stepper, small, transform, 2)
    finally:
        runtime.set_compute_dtype('f32')


def test_mixup_stepper_refuses_device_targets():
    from sound_event_detection_transformer_amd import runtime
    runtime.set_compute_dtype('bf16')
    try:
        B = 2
        clips, transform, model, opt, stepper = _train_setup(B, mix_up_ratio=0.6)
        x1, dt1 = clips.batch(transform, clips.draw(B))
        with pytest.raises(NotImplementedError, match='without mix-up only'):
            stepper(x1, dt1)
    finally:
        runtime.set_compute_dtype('f32')
