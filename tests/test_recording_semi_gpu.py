"""GPU: mix-up and mean-teacher training on recordings - the steppers fed targets that were built on the device
(utilities.recording_clips.DeviceTargets with a strong | weak | unlabelled split; TargetTables.load / load_mixed, sedt_mixup_plan)
against the SAME stepper, restored from its snapshot with np.random rewound, fed the list form of the same targets (the host plan).
Both routes fill the same tables and job records and steps are bit-reproducible, so loss terms and parameters are compared bit for bit.
Then engine.semi_train_on_recordings: one cut and one plan launch per step, no pinned TargetTables slot, no synchronisation in the loop,
a clip over capacity reported once at the end.  The kernel itself: tests/test_mixup_plan_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import sedt_oracle as O

pytestmark = pytest.mark.gpu

SR = 16000
LABELS = [f'c{i}' for i in range(10)]


def corpus():
    """two strong, two weak (one as long as the window, one a sample longer) and two unlabelled recordings; the strong ones share no class,
    so that windows of the two can be mixed"""
    gen = torch.Generator().manual_seed(33)
    samples = {'a.wav': 14 * SR + 321, 'b.wav': 12 * SR, 'w0.wav': 10 * SR, 'w1.wav': 10 * SR + 1, 'u0.wav': 15 * SR, 'u1.wav': 10 * SR}
    waves = {n: 0.1 * torch.randn(k, generator=gen).numpy() for n, k in samples.items()}
    ev = np.random.default_rng(8)
    strong = {n: sorted((c0 + i, float(t), float(t + ev.uniform(0.3, 2.0))) for i, t in enumerate(ev.uniform(0.0, samples[n] / SR - 0.5, 5)))
              for n, c0 in (('a.wav', 0), ('b.wav', 5))}
    weak = {'w0.wav': ['c3', 'c7', 'c3'], 'w1.wav': [2]}
    return waves, strong, weak


def _stage(max_targets=32, strong=None):
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.recording_clips import RecordingClips
    waves, ref, weak = corpus()
    ref = ref if strong is None else strong
    clips = RecordingClips(DeviceMelSpectrogram.dcase(), LABELS, 10.0, max_targets=max_targets)
    clips.add([waves['a.wav'], waves['b.wav']], ['a.wav', 'b.wav'], ref)
    clips.add([waves['w0.wav'], waves['w1.wav']], ['w0.wav', 'w1.wav'], weak, kind='weak')
    clips.add([waves['u0.wav'], waves['u1.wav']], ['u0.wav', 'u1.wav'], None, kind='unlabelled')
    return clips


def _model(seed=5):
    from sound_event_detection_transformer_amd import sedt
    from sound_event_detection_transformer_amd.engine import build_optimizer
    model, crit, _ = sedt.build_model(sedt.default_args(dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), seed))
    model.cuda().train()
    crit.cuda()
    return model, crit, build_optimizer(model)


def _result(out, model, ema=None):
    torch.cuda.synchronize()
    flat = []
    for o in out:
        flat += [o[k] for k in sorted(o)] if isinstance(o, dict) else [o]
    return ([t.detach().clone() for t in flat], [p.detach().clone() for p in model.parameters()],
            [] if ema is None else [ema.shadow[k].detach().clone() for k in sorted(ema.shadow)])


def _same(a, b):
    return all(len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))


def _modes(jobs):
    return jobs.cpu().numpy().view(np.int32).reshape(-1, 4)[:, 2].tolist()


def test_mixing_train_step_on_device_targets_equals_the_list_route():
    from sound_event_detection_transformer_amd import engine, lib, runtime
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    runtime.set_compute_dtype('bf16')
    try:
        clips, transform = _stage(), DeviceBoxTransform(500)
        ns, B = 2, 4
        np.random.seed(17)
        x0, dt0 = clips.batch(transform, clips.draw_split(ns, B - ns), split=(ns, B))
        assert (dt0.ns, dt0.n_lab) == (ns, B) and dt0.names[2][0] == 'w' and tuple(x0.shape) == (B, 1, 500, 64)
        model, crit, opt = _model()
        stepper = engine.GraphedTrainStep(model, crit, opt, x0.clone(), dt0.to_list(), slice(ns, B), slice(ns), warmup=1, mix_up_ratio=0.5,
                                          max_targets=32)
        merged = 0
        for k in (4, 0, 1):                                                       # (seeds picked so that the first batch's draw mixes a pair)
            np.random.seed(100 + k)
            x, dt = clips.batch(transform, clips.draw_split(ns, B - ns), split=(ns, B))
            x = x.clone()
            snap = engine._snapshot(model, opt)
            slot = stepper.tables._slot
            np.random.seed(200 + k)
            with lib.launch_log() as log:
                a = _result(stepper(x, dt), model)
            assert log['mixup_plan'] == 1 and stepper.tables._slot == slot        # planned on the device: no pinned host slot
            jobs_a = stepper._jobs.dev_buf.clone()
            lst = dt.to_list()                                                    # (no cut since: the blob still holds this batch)
            assert all(len(t['boxes']) == 0 for t in lst[ns:]) and sum(len(t['labels']) for t in lst[ns:]) > 0
            engine._restore(model, opt, snap)
            np.random.seed(200 + k)                                               # np.random rewound: the same draws
            with lib.launch_log() as log:
                b = _result(stepper(x, lst), model)
            assert log['mixup_plan'] == 0 and stepper.tables._slot != slot
            assert torch.equal(jobs_a, stepper._jobs.dev_buf)
            assert _same(a, b) and bool(torch.isfinite(a[0][0]).all())
            assert any(not torch.equal(p, q) for p, q in zip(a[1], snap['p']))
            merged += _modes(jobs_a).count(0)
        assert merged > 0                                                         # a pair really was mixed
        # the loop, with a split and a mixing stepper
        with lib.launch_log() as log:
            total, _ = engine.train_on_recordings(stepper, clips, transform, 2, split=(ns, B - ns))
        assert log['cut_clips'] == 2 and log['mixup_plan'] == 2 and bool(torch.isfinite(total).all())
        # what the device route needs is said up front
        with pytest.raises(ValueError, match=r'the stepper was built for 2 \| 4 of 4'):
            stepper(*clips.batch(transform, clips.draw_split(3, 1), split=(3, 4)))
    finally:
        runtime.set_compute_dtype('f32')


def _semi_setup(mix):
    from sound_event_detection_transformer_amd import engine
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceViewTransform
    from sound_event_detection_transformer_amd.utilities.utils import EMA
    clips, views = _stage(), DeviceViewTransform(500, noise_p=1.0)
    np.random.seed(17)
    (xt, xs), dt0 = clips.batch(views, clips.draw_split(2, 1, 2), split=(2, 3))
    assert (dt0.ns, dt0.n_lab, dt0.B) == (2, 3, 5) and not torch.equal(xt[3:], xs[3:])
    model, crit, opt = _model()
    ema = EMA(model, 0.9)
    ema.register()
    with torch.no_grad():
        for n in ema.shadow:
            ema.shadow[n].mul_(1.01)
    thr = torch.full((10,), 0.115).cuda()
    stepper = engine.GraphedSemiStep(model, ema, crit, opt, xt.clone(), xs.clone(), dt0.to_list(), mask_strong=slice(2), mask_weak=slice(2, 3),
                                     mask_label=slice(3), mask_unlabel=slice(3, 5), classwise_threshold=thr, warmup=1, max_targets=32,
                                     mix_up_ratio=mix)
    return clips, views, model, opt, ema, stepper


@pytest.mark.parametrize('mix', [0.0, 0.6])
def test_semi_step_on_device_targets_equals_the_list_route(mix, monkeypatch):
    """a 2 strong + 1 weak + 2 unlabelled batch; with mix-up int(3 * 0.6) = 1 labelled clip is mixed"""
    from sound_event_detection_transformer_amd import engine, lib, runtime
    runtime.set_compute_dtype('bf16')
    try:
        clips, views, model, opt, ema, stepper = _semi_setup(mix)
        merged = 0
        for k in (3, 0):                                                          # (with seed 3 the mixed clip's draw is a merge)
            np.random.seed(100 + k)
            (xt, xs), dt = clips.batch(views, clips.draw_split(2, 1, 2), split=(2, 3))
            xt, xs = xt.clone(), xs.clone()
            snap = engine._snapshot(model, opt, ema)
            slot = stepper.tab_l._slot
            np.random.seed(200 + k)
            with lib.launch_log() as log:
                a = _result(stepper(xt, xs, dt), model, ema)
            assert log['mixup_plan'] == (1 if mix else 0) and stepper.tab_l._slot == slot
            lst = dt.to_list()
            assert [len(t['labels']) > 0 for t in lst[2:]] == [True, False, False] and all(len(t['boxes']) == 0 for t in lst[2:])
            engine._restore(model, opt, snap, ema)
            np.random.seed(200 + k)
            b = _result(stepper(xt, xs, lst), model, ema)
            assert stepper.tab_l._slot != slot
            assert _same(a, b) and bool(torch.isfinite(a[0][0]).all())
            assert any(not torch.equal(p, q) for p, q in zip(a[1], snap['p']))
            merged += _modes(stepper._jobs_l.dev_buf).count(0) if mix else 0
        if not mix:
            return
        assert merged > 0
        # ---- the loop: three steps
        calls = {'sync': 0}
        real = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a_, **k_: (calls.__setitem__('sync', calls['sync'] + 1), real(*a_, **k_))[1])
        slot = stepper.tab_l._slot
        before = [p.detach().clone() for p in model.parameters()]
        with lib.launch_log() as log:
            total, _, _ = engine.semi_train_on_recordings(stepper, clips, views, 3, split=(2, 1, 2))
        monkeypatch.setattr(torch.cuda, 'synchronize', real)
        assert log['cut_clips'] == 3 and log['mixup_plan'] == 3 and log['box_transform_views'] == 3 and calls['sync'] == 0
        assert stepper.tab_l._slot == slot                                        # no pinned TargetTables slot
        assert bool(torch.isfinite(total).all()) and any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
        # a clip over capacity is reported once, at the end, with step and recording
        dense = {n: [(i % 10, 0.04 * i, 0.04 * i + 0.02) for i in range(300)] for n in ('a.wav', 'b.wav')}
        small = _stage(strong=dense)
        with pytest.raises(RuntimeError, match=r"semi_train_on_recordings: step 0, clip [01] of recording '[ab].wav': status 1"):
            engine.semi_train_on_recordings(stepper, small, views, 2, split=(2, 1, 2))
    finally:
        runtime.set_compute_dtype('f32')
