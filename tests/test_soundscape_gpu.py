"""GPU: sedt_bank_stats and sedt_soundscape (csrc/soundscape.hip) through utilities.soundscape.SoundscapeClips against
tests/soundscape_ref.py, and the training route they open.  Everything is exact: waves, peaks and scales bit-equal; offsets, labels and
status equal; boxes bit-equal in float32.

Shapes (tests/soundscape_cases.py, checked on the reference alone by tests/test_soundscape_cpu.py): windows of 1003 samples (no multiple
of a vector width and less than one chunk) and 4096 (two chunks); B = 1, 5, 65; sources of 1, 3, 700, 5000 and 20000 samples; onsets 0, 1,
2, 3, 2047, 2048; an event ending exactly at the window and one running past it; n = 1; fade 0, 160 and longer than half the event; a
700-sample background from sample 699 on, a 3-sample one, none; nested, chained, touching and disjoint events of one class with collapse
on and off; classes at the same time; a clip without events between clips with events; capacity; every kind of bad record between good
neighbours; successive calls into the same buffers, the later ones with fewer events."""
import functools

import numpy as np
import pytest
import torch

import recording_clips_ref as R
import soundscape_cases as K
import soundscape_ref as S
from oracle import sedt_oracle as O

pytestmark = pytest.mark.gpu

SR, LABELS = K.SR, K.LABELS


@pytest.fixture(scope='module')
def bank():
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    assert torch.cuda.is_available()
    sounds, classes, backgrounds = K.bank()
    return dict(sounds=sounds, classes=classes, backgrounds=backgrounds, sources=sounds + backgrounds, mel=DeviceMelSpectrogram.dcase())


def _scapes(bank, window, M, **kw):
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    s = SoundscapeClips(bank['mel'], LABELS, window / SR, max_targets=M, **kw)
    assert s.window == window
    s.add_events(bank['sounds'], [LABELS[c] for c in bank['classes']]).add_backgrounds(bank['backgrounds'])
    assert len(s) == K.N_SRC and s.backgrounds == [5, 6] and s.by_class[:5] == [[0], [1], [2], [3], [4]]
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def _ref_clip(key, W, M, min_len, collapse, limit):
    """the reference of ONE designed clip (computed once, shared): key = ('clip' | 'bad', index)"""
    chosen = (K.clips(W) if key[0] == 'clip' else K.bad_clips(W))[key[1]]
    sounds, _, backgrounds = K.bank()
    bg, ev, off = K.records([chosen])
    wave, peak, scale, targets, status = S.soundscape(sounds + backgrounds, bg, ev, off, W, SR, M, min_len, collapse, limit)
    return wave[0], peak[0], scale[0], targets[0], status[0]


def _check(scapes, keys, sources=None, plan=None, status=None):
    """one call against the reference; ``keys``: designed clips, or with ``plan`` (a drawn one) the reference is computed here"""
    from sound_event_detection_transformer_amd.utilities.recording_clips import blob_layout
    W, M = scapes.window, scapes.max_targets
    if plan is None:
        chosen = [(K.clips(W) if k[0] == 'clip' else K.bad_clips(W))[k[1]] for k in keys]
        plan = scapes.plan([g for g, _ in chosen], [e for _, e in chosen])
        ref = [_ref_clip(k, W, M, scapes.min_event_seconds, scapes.collapse, scapes.peak_limit) for k in keys]
        want = [np.stack([r[0] for r in ref]), np.asarray([r[1] for r in ref]), np.asarray([r[2] for r in ref]), [r[3] for r in ref],
                np.asarray([r[4] for r in ref])]
    else:
        want = S.soundscape(sources, plan.bg, plan.ev, plan.ev_off, W, SR, M, scapes.min_event_seconds, scapes.collapse, scapes.peak_limit)
    B = len(plan)
    wave, lengths, dt = scapes.mix(plan, status=status)
    assert wave.shape == (B, W) and lengths == [W] * B and dt.names == ['soundscape'] * B and dt.B == B
    assert np.array_equal(_bits(wave.cpu().numpy()), _bits(want[0]))
    assert np.array_equal(_bits(scapes.last_peak.cpu().numpy()), _bits(want[1].astype(np.float32)))
    assert np.array_equal(_bits(scapes.last_scale.cpu().numpy()), _bits(want[2].astype(np.float32)))
    assert dt.status.cpu().numpy().tolist() == want[4].tolist()
    off, lab, box, (o_lab, o_box, total) = R.blob(want[3], M)
    assert blob_layout(B, M) == (2 * B + 4, o_lab, o_box, total) and dt.blob.numel() == total
    raw = dt.blob.cpu().numpy()
    assert raw[:4 * (2 * B + 4)].view(np.int32).tolist() == off.tolist()
    assert raw[o_lab:o_lab + 8 * len(lab)].view(np.int64).tolist() == lab.tolist()
    assert np.array_equal(raw[o_box:o_box + 8 * len(lab)].view(np.int32), _bits(box.reshape(-1)))
    return want, dt


@pytest.mark.parametrize('collapse', [True, False])
@pytest.mark.parametrize('window', K.WINDOWS)
@pytest.mark.parametrize('B', [1, 5, 65])
def test_soundscape_against_the_reference(bank, window, B, collapse):
    scapes = _scapes(bank, window, 63, collapse=collapse)
    n = len(K.clips(window))
    for lo in range(0, max(n, 2 * B), B):                          # successive calls into the same buffers
        want, _ = _check(scapes, [('clip', (lo + i) % n) for i in range(B)])
        assert not want[4].any()
    want, _ = _check(scapes, [('clip', K.QUIET[i % len(K.QUIET)]) for i in range(B)])      # ... the last one with fewer events
    assert sum(len(t[0]) for t in want[3]) <= B


def test_capacity(bank):
    """max_targets = 3: a clip with exactly three survivors is complete, one with four raises status 1 and keeps the first three; a
    later call into the same buffers with fewer events is complete again"""
    scapes = _scapes(bank, 1003, 3)
    n = len(K.clips(1003))
    want, dt = _check(scapes, [('clip', i) for i in range(n)])
    assert want[4].tolist() == [0] * 8 + [1] and [len(t[0]) for t in want[3]] == [3, 0, 1, 1, 2, 1, 0, 2, 3]
    with pytest.raises(RuntimeError, match="clip 8 of recording 'soundscape': status 1"):
        dt.to_list()
    with pytest.raises(RuntimeError, match='clip 8'):
        dt.check()
    want, dt = _check(scapes, [('clip', i) for i in (1, 0, 6, 7, 2, 4, 1, 5, 3)])
    assert not want[4].any()
    lst = dt.to_list()
    assert [t['labels'].tolist() for t in lst] == [t[0].tolist() for t in want[3]]
    assert all(np.array_equal(_bits(a['boxes'].numpy()), _bits(b[1])) for a, b in zip(lst, want[3]))
    assert all(float(t['orig_size']) == float(np.float32(scapes.window_seconds)) for t in lst)


@pytest.mark.parametrize('window', K.WINDOWS)
def test_bad_records_raise_status_2_and_leave_their_neighbours_alone(bank, window):
    scapes = _scapes(bank, window, 63)
    keys = []
    for i in range(len(K.bad_clips(window))):
        keys += [('clip', (0, 4, 3)[i % 3]), ('bad', i)]
    log = torch.zeros(len(keys), dtype=torch.int32, device='cuda')          # the statuses go where the caller wants them
    want, dt = _check(scapes, keys + [('clip', 7)], status=None)
    assert want[4].tolist() == [0, 2] * (len(keys) // 2) + [0]
    _check(scapes, keys, status=log)
    assert log.cpu().tolist() == [0, 2] * (len(keys) // 2)
    with pytest.raises(ValueError, match='status is a contiguous int32'):
        scapes.mix(scapes.plan([None], [[]]), status=log)


def test_drawn_plans_and_min_event_seconds(bank):
    """plans drawn over the staged bank: the restated draw gives the same records from the statistics the device returned; three calls
    of falling size into the same buffers"""
    scapes = _scapes(bank, 4096, 63, min_event_seconds=0.004, peak_limit=0.05)
    dropped = scaled = 0
    for B, seed in ((33, 3), (32, 4), (7, 5)):
        np.random.seed(seed)
        plan = scapes.draw(B, n_events=(0, 9), snr_db=(0.0, 30.0), ref_db=-35.0, max_event_seconds=0.05, fade_seconds=0.002)
        np.random.seed(seed)
        bg, ev, off = S.draw(B, scapes.ns, scapes.rms, scapes.by_class, scapes.backgrounds, 4096, SR, (0, 9), (0.0, 30.0), -35.0, 0.05, 0.002)
        assert plan.bg.tobytes() == bg.tobytes() and plan.ev.tobytes() == ev.tobytes() and plan.ev_off.tolist() == off.tolist()
        want, _ = _check(scapes, None, bank['sources'], plan)
        assert not want[4].any()
        loose = S.soundscape(bank['sources'], plan.bg, plan.ev, plan.ev_off, 4096, SR, 63, 0.0, True, 0.05)
        dropped += sum(len(a[0]) - len(b[0]) for a, b in zip(loose[3], want[3]))
        scaled += int((want[2] < 1).sum())
    assert dropped > 0 and scaled > 0                               # the threshold drops events, the limit scales clips


@pytest.mark.parametrize('collapse', [True, False])
def test_full_clips_across_target_tiles(bank, collapse):
    """clips of 63, 60, 1, 63, 0, 62, 63, 63, 5 events: the targets workgroup resolves events in tiles of at most 256 (here 249 events
    in clips 0 .. 5, then the rest: a tile boundary set by the event count, not by the clip count), a clip fills 63 lanes of its wave,
    and with collapse off clips hold exactly 63 = max_targets survivors"""
    W = 4096
    scapes = _scapes(bank, W, 63, collapse=collapse)
    gen = np.random.default_rng(63)
    counts = [63, 60, 1, 63, 0, 62, 63, 63, 5]
    events = []
    for k in counts:
        clip = []
        for _ in range(k):
            src = int(gen.integers(2, 5))
            n = int(gen.integers(1, 120))
            clip.append((src, int(gen.integers(0, 4)), int(gen.integers(0, K.EVENT_LENS[src] - n)), n, int(gen.integers(0, W - 60)),
                         float(gen.uniform(0.05, 0.5)), int(gen.integers(0, 30))))
        events.append(clip)
    plan = scapes.plan([(6, 77, 0.3), None] * 4 + [(5, 1, 0.2)], events)
    want, _ = _check(scapes, None, bank['sources'], plan)
    n = [len(t[0]) for t in want[3]]
    assert not want[4].any() and (n[:3] == [63, 60, 1] and n[4] == 0 if not collapse else 0 < n[0] < 63)
    small = _scapes(bank, W, 32, collapse=False)                   # the same plan over capacity: the first 32 of 63
    want, _ = _check(small, None, bank['sources'], plan)
    assert want[4].tolist() == [1, 1, 0, 1, 0, 1, 1, 1, 0] and [len(t[0]) for t in want[3]][:3] == [32, 32, 1]


def test_cross_check_against_recording_clips(bank):
    """collapse=False: the synthesized waves staged as recordings and the plan's events as their annotations give, cut at start 0 by
    sedt_cut_clips, a byte-identical blob"""
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    W, M, B = 4096, 63, 9
    scapes = _scapes(bank, W, M, collapse=False)
    np.random.seed(12)
    plan = scapes.draw(B, n_events=(0, 9), max_event_seconds=0.1)
    wave, _, dt = scapes.mix(plan)
    names = [f'scape{b}.wav' for b in range(B)]
    rows = lambda b: sorted((int(e['onset']), int(min(e['onset'] + e['n'], W)), int(e['cls'])) for e in plan.events(b))
    ref = {names[b]: [(c, on / SR, end / SR) for on, end, c in rows(b)] for b in range(B)}
    assert sum(len(v) for v in ref.values()) > B
    clips = RecordingClips(bank['mel'], LABELS, W / SR, max_targets=M).add([wave[b] for b in range(B)], names, ref)
    wave2, _, dt2 = clips.cut(np.arange(B, dtype=np.int32), np.zeros(B, np.int64))
    assert torch.equal(wave2, wave) and torch.equal(dt2.blob, dt.blob) and torch.equal(dt2.status, dt.status)
    assert not dt.status.any().item()


def test_bank_stats_and_staging(bank):
    from sound_event_detection_transformer_amd import lib as L
    from sound_event_detection_transformer_amd.utilities.resample import DeviceResampler
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    scapes = _scapes(bank, 4096, 63)
    sumsq, peak = S.bank_stats(bank['sources'])
    assert np.array_equal(scapes.peak, peak) and scapes.peak.dtype == np.float32 and scapes.rms.dtype == np.float64
    want_rms = np.sqrt(sumsq / np.asarray(scapes.ns, np.float64))
    assert np.allclose(scapes.rms, want_rms, rtol=1e-12, atol=0.0)
    out = []
    for _ in range(2):                                             # the entry point itself, twice: identical bits
        q = torch.full((K.N_SRC,), -1.0, dtype=torch.float64, device='cuda')
        p = torch.full((K.N_SRC,), -1.0, dtype=torch.float32, device='cuda')
        L.check(L.load().sedt_bank_stats(L.p(scapes.flat), int(scapes.src_off[-1]), L.p(scapes.table['off']), L.p(scapes.table['len']),
                                         K.N_SRC, L.p(q), L.p(p), L.stream_ptr()), 'bank_stats')
        out.append((q.cpu().numpy(), p.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][1], peak) and np.allclose(out[0][0], sumsq, rtol=1e-12, atol=0.0)
    assert out[0][0][0] == 0.25 and out[0][0][1] == 0.25 ** 2 + 0.5 ** 2 + 0.125 ** 2          # sums of a few exact squares
    for s in range(K.N_SRC):
        assert np.array_equal(scapes.wave(s).cpu().numpy(), bank['sources'][s])
    # refusals that need the statistics; a refused add leaves the bank as it was
    with pytest.raises(ValueError, match='source 1 is silent'):
        scapes.add_events([np.ones(5, np.float32), np.zeros(900, np.float32)], ['c1', 'c2'])
    with pytest.raises(ValueError, match='source 0 holds non-finite samples'):
        scapes.add_backgrounds([np.asarray([0.0, np.nan, 1.0], np.float32)])
    with pytest.raises(ValueError, match='source 0 holds non-finite samples'):
        scapes.add_events([np.asarray([np.inf], np.float32)], [3])
    assert len(scapes) == K.N_SRC and scapes.flat.numel() == sum(scapes.ns)
    # a silent background, 16-bit PCM, and a stereo sound at another rate through the shared staging
    gen = torch.Generator().manual_seed(48)
    stereo = (0.1 * torch.randn(4800 + 7, 2, generator=gen) * 32768).clamp(-32768, 32767).to(torch.int16).numpy()
    pcm = (0.1 * torch.randn(900, generator=gen) * 32768).clamp(-32768, 32767).to(torch.int16).numpy()
    scapes.add_backgrounds([np.zeros(64, np.float32), pcm]).add_events([stereo], ['c9'], sample_rates=48000)
    assert scapes.backgrounds == [5, 6, 7, 8] and scapes.by_class[9] == [9] and scapes.rms[7] == 0.0 and scapes.peak[7] == 0.0
    want, n = DeviceResampler(48000, SR)([stereo])
    assert scapes.ns[9] == n[0] and torch.equal(scapes.wave(9), want[0, :n[0]])
    assert np.array_equal(scapes.wave(8).cpu().numpy(), pcm.astype(np.float32) * np.float32(1.0 / 32768.0))
    assert np.array_equal(scapes.wave(4).cpu().numpy(), bank['sources'][4])                        # a later add keeps the earlier ones
    sources = bank['sources'] + [np.zeros(64, np.float32), scapes.wave(8).cpu().numpy(), scapes.wave(9).cpu().numpy()]
    assert np.allclose(scapes.rms, np.sqrt(S.bank_stats(sources)[0] / np.asarray(scapes.ns)), rtol=1e-12, atol=0.0)
    np.random.seed(8)
    plan = scapes.draw(5, n_events=(2, 6), max_event_seconds=0.05)
    assert all(g['gain'] == 1.0 for g in plan.bg if g['src'] == 7)
    _check(scapes, None, sources, plan)
    fresh = SoundscapeClips(bank['mel'], LABELS, 4096 / SR)
    with pytest.raises(RuntimeError, match='add_events'):
        fresh.mix(plan)


# ---------------------------------------------------------------------------------------------------- end to end
def _train_setup(B, seed=5):
    """a bank of four sounds and one background staged, the smallest model of the stepper tests, a GraphedTrainStep built on a first
    synthesized batch"""
    from sound_event_detection_transformer_amd import sedt
    from sound_event_detection_transformer_amd.engine import GraphedTrainStep, build_optimizer
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    gen = torch.Generator().manual_seed(23)
    sounds = [0.1 * torch.randn(n, generator=gen).numpy() for n in (SR // 2, SR + 77, 2 * SR, 3 * SR + 1)]
    background = 0.01 * torch.randn(12 * SR + 5, generator=gen).numpy()
    mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
    scapes = SoundscapeClips(mel, LABELS, 10.0, max_targets=32).add_events(sounds, ['c1', 'c4', 'c4', 'c7']).add_backgrounds([background])
    np.random.seed(17)
    x0, dt0 = scapes.batch(transform, scapes.draw(B))
    example, x0 = dt0.to_list(), x0.clone()
    assert sum(len(t['labels']) for t in example) > 0 and tuple(x0.shape) == (B, 1, 500, 64)
    model, crit, _ = sedt.build_model(sedt.default_args(dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), seed))
    model.cuda().train()
    crit.cuda()
    opt = build_optimizer(model)
    stepper = GraphedTrainStep(model, crit, opt, x0, example, None, slice(B), warmup=1)
    return scapes, transform, model, opt, stepper


def _result(out, model):
    total, losses = out
    torch.cuda.synchronize()
    terms = {k: v.detach().clone() for k, v in losses.items()} if isinstance(losses, dict) else {'losses': losses.detach().clone()}
    return total.detach().clone(), terms, [p.detach().clone() for p in model.parameters()]


def test_train_on_recordings_takes_soundscapes(monkeypatch):
    """engine.train_on_recordings with a SoundscapeClips where it expects a RecordingClips: three steps, one sedt_soundscape call each,
    nothing read back inside the loop, finite losses - and bit-equal to the same stepper restored and fed (x, targets.to_list()) of the
    same seeded plans by hand"""
    from sound_event_detection_transformer_amd import engine, lib, runtime
    runtime.set_compute_dtype('bf16')
    try:
        B = 2
        scapes, transform, model, opt, stepper = _train_setup(B)
        snap = engine._snapshot(model, opt)
        calls = {'sync': 0}
        real = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a_, **k_: (calls.__setitem__('sync', calls['sync'] + 1), real(*a_, **k_))[1])
        slot = stepper.tables._slot
        np.random.seed(29)
        with lib.launch_log() as log:
            out = engine.train_on_recordings(stepper, scapes, transform, 3)
        monkeypatch.setattr(torch.cuda, 'synchronize', real)
        assert log['soundscape'] == 3 and log['mel_spectrogram'] == 3 and log['cut_clips'] == 0 and calls['sync'] == 0
        assert stepper.tables._slot == slot                                   # no TargetTables host copy
        a = _result(out, model)
        assert bool(torch.isfinite(a[0]).all()) and all(bool(torch.isfinite(v).all()) for v in a[1].values())
        assert any(not torch.equal(p, q) for p, q in zip(a[2], snap['p']))
        # ---- the same three steps by hand, through the list route
        engine._restore(model, opt, snap)
        np.random.seed(29)
        events = 0
        for _ in range(3):
            x, dt = scapes.batch(transform, scapes.draw(B))
            lst = dt.to_list()
            events += sum(len(t['labels']) for t in lst)
            out = stepper(x.clone(), lst)
        b = _result(out, model)
        assert events > 0 and stepper.tables._slot != slot
        assert torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
        assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
        # a clip over capacity is reported once, at the end, with its step
        small = type(scapes)(scapes.mel, LABELS, 10.0, max_targets=32, collapse=False)
        small.add_events([scapes.wave(0)], ['c1'])
        full = small.plan([None] * B, [[(0, i % 10, 0, 100, 200 * i, 1.0, 0) for i in range(40)]] * B)
        monkeypatch.setattr(small, 'draw', lambda n: full)
        with pytest.raises(RuntimeError, match=r"train_on_recordings: step 0, clip 0 of recording 'soundscape': status 1"):
            engine.train_on_recordings(stepper, small, transform, 2)
    finally:
        runtime.set_compute_dtype('f32')
