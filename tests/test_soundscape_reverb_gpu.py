"""GPU: the wet events of SoundscapeClips (utilities/soundscape.py: add_rirs, draw(reverb=), mix) - sedt_reverb behind the stretch stage,
the head / tail split, sedt_reverb_bed, and the unchanged mixing call on the extended source table.

A hand-made plan of three clips - one without a wet event; one with a wet and a dry event of one class and a stretched wet event; one
without a background whose wet event's tail passes the window's end - is mixed once.  The wiring is checked bit for bit: the bed rows
against tests/reverb_ref.py's bed fed the device's own wet rows, the wave against tests/soundscape_ref.py fed the device's heads and
beds.  The wave is then checked against soundscape_ref fed the REFERENCE's head rows and beds (np.convolve in float64 of the dry sound
under its fade), within the sum over the clip's wet events of gain times 8 times what the float32 restatement misses the row by - the
stage's own end-to-end criterion - plus the mixing's roundings."""
import numpy as np
import pytest
import torch

import reverb_ref as R
import soundscape_ref as S

pytestmark = pytest.mark.gpu

SR, W, NFFT = 16000, 4096, 512
LABELS = [f'c{i}' for i in range(10)]
EVENTS = [[(1, 4, 200, 2000, 1500, 0.7, 0)],
          [(1, 4, 0, 1000, 100, 0.5, 16), (2, 4, 0, 2000, 900, 0.3, 160), (0, 1, 0, 700, 2000, 0.6, 16, 3.0, 1.25)],
          [(3, 7, 1000, 700, 3000, 0.9, 8)]]
RIRS = [[-1], [0, -1, 2], [1]]
BGS = [(4, 100, 0.5), (4, 5999, 1.0), None]


@pytest.fixture(scope='module')
def bank():
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    gen = np.random.default_rng(78)
    sounds = [(0.1 * gen.standard_normal(n)).astype(np.float32) for n in (700, 3000, 2000, 5000)]
    backgrounds = [(0.01 * gen.standard_normal(6000)).astype(np.float32)]
    rirs = [(gen.standard_normal(L) * np.exp(-6.0 * np.arange(L) / L)).astype(np.float32) for L in (300, 1500, 700)]
    return dict(sounds=sounds, classes=[1, 4, 4, 7], backgrounds=backgrounds, rirs=rirs, mel=DeviceMelSpectrogram.dcase())


def _scapes(bank, rirs=True, **kw):
    from sound_event_detection_transformer_amd.utilities.soundscape import SoundscapeClips
    s = SoundscapeClips(bank['mel'], LABELS, W / SR, stretch_n_fft=512, reverb_n_fft=NFFT, resample_quality='kaiser_fast', **kw)
    s.add_events(bank['sounds'], bank['classes']).add_backgrounds(bank['backgrounds'])
    if rirs:
        s.add_rirs(bank['rirs'], rooms=['a', 'b', 'a'])
    return s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_wet_events_head_tail_and_bed(bank):
    s = _scapes(bank)
    assert s.rooms == [[0, 2], [1]] and len(s.reverberator()) == 3
    hs = s.reverberator().rirs
    assert all(abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) < 1e-6 for h in hs)          # normalize='energy'
    plan = s.plan(BGS, EVENTS, RIRS)
    assert plan.rir.tolist() == [-1, 0, -1, 2, 1] and plan.fx is not None
    wave, _, dt = s.mix(plan)
    wave, blob = wave.cpu().numpy().copy(), dt.blob.cpu().numpy().copy()
    assert not dt.status.any().item() and not s.last_fx_status.any().item() and not s.last_rv_status.any().item()
    fx = s.last_fx
    flat, jobs, rj = fx['flat'].cpu().numpy(), fx['jobs'], fx['reverb_jobs']
    bank_end = int(s.src_off[-1])
    assert flat[:bank_end].tobytes() == s.flat.cpu().numpy().tobytes()                        # the bank in front of the results
    assert len(jobs) == 1 and len(rj) == 3 and fx['wet'].tolist() == [1, 3, 4] and fx['clips'].tolist() == [1, 2]
    assert (rj['dst_off'] % 4 == 0).all() and int(rj['dst_off'][0]) >= int(jobs['dst_off'][0] + jobs['m'][0])
    stretched = flat[int(jobs['dst_off'][0]):int(jobs['dst_off'][0] + jobs['m'][0])].copy()      # the stretched wet event's dry input
    assert len(stretched) == 875 and int(rj['src_off'][1]) == int(jobs['dst_off'][0]) and rj['n'].tolist() == [1000, 875, 700]
    assert rj['fade'].tolist() == [16, 16, 8] and rj['rir'].tolist() == [0, 2, 1]
    assert int(rj['src_off'][0]) == int(s.src_off[1]) and int(rj['src_off'][2]) == int(s.src_off[3]) + 1000
    dry = [bank['sounds'][1][:1000], stretched, bank['sounds'][3][1000:1700]]
    Ls = [300, 700, 1500]
    wet_dev = [flat[int(j['dst_off']):int(j['dst_off']) + int(j['n']) + L - 1].copy() for j, L in zip(rj, Ls)]
    # ---- every wet row against the direct form, the stage's own criterion
    wet_ref, miss = [], []
    for e in range(3):
        h, fade = hs[int(rj['rir'][e])], int(rj['fade'][e])
        want = R.direct(dry[e], h, fade)
        yard = float(np.abs(R.chain(dry[e], h, fade, NFFT, np.float32)['wet'] - want).max())
        err = float(np.abs(wet_dev[e] - want).max())
        print('wet row', e, f'float32 restatement {yard:.3e} device {err:.3e}')
        assert err <= 8.0 * yard
        wet_ref.append(want.astype(np.float32))
        miss.append(8.0 * yard + 2.0 ** -24 * float(np.abs(want).max()))        # ... and the rounding of the reference row to float32
    # ---- the records: heads, tails, beds, the table
    ev, tails, beds, bg = fx['events'], fx['tails'], fx['beds'], fx['bg']
    n_src = len(s)
    assert ev['src'].tolist() == [1, n_src + 1, 2, n_src + 2, n_src + 3] and ev['src_start'].tolist() == [200, 0, 0, 0, 0]
    assert ev['n'].tolist() == [2000, 1000, 2000, 875, 700] and ev['fade'].tolist() == [0, 0, 160, 0, 0]
    assert ev['onset'].tolist() == plan.ev['onset'].tolist() and ev['gain'].tobytes() == plan.ev['gain'].tobytes()
    assert tails['head'].tolist() == [1000, 875, 700] and tails['total'].tolist() == [1299, 1574, 2199]
    assert beds['tail_lo'].tolist() == [0, 2] and beds['tail_hi'].tolist() == [2, 3] and beds['src'].tolist() == [4, -1]
    assert bg['src'].tolist() == [4, n_src + 4, n_src + 5] and bg['start'].tolist() == [100, 0, 0] and bg['gain'].tolist() == [0.5, 1.0, 1.0]
    assert fx['rows_len'].tolist() == list(s.ns) + [875, 1299, 1574, 2199, W, W] and len(fx['rows_off']) == n_src + 6

    def build(wets):
        """(the beds, soundscape_ref's answer) from three wet rows"""
        bd = [R.bed(W, bank['backgrounds'][0], 5999, 1.0, [(0.5, wets[0], 100, 1000), (0.6, wets[1], 2000, 875)]),
              R.bed(W, None, 0, 1.0, [(0.9, wets[2], 3000, 700)])]
        sources = bank['sounds'] + bank['backgrounds'] + [stretched] + list(wets) + bd
        return bd, S.soundscape(sources, bg, ev, plan.ev_off, W, SR, s.max_targets, s.min_event_seconds, s.collapse, s.peak_limit)

    # ---- the wiring, bit for bit, from the device's own wet rows
    bd, want = build(wet_dev)
    for c in range(2):
        got = flat[int(beds['dst_off'][c]):int(beds['dst_off'][c]) + W]
        assert np.array_equal(_bits(got), _bits(bd[c])), c
    assert not flat[int(beds['dst_off'][1]):int(beds['dst_off'][1]) + 3700].any()           # no background: nothing before the tail
    assert bd[1][3700:].all() and 3000 + 2199 > W                                            # the tail runs into the window's end and is cut
    assert np.array_equal(_bits(wave), _bits(want[0])) and (want[4] == 0).all()
    # ---- the wave against the reference's heads and beds
    _, ref = build(wet_ref)
    peak = float(np.abs(ref[0]).max())
    tol = [0.0, 0.5 * miss[0] + 0.6 * miss[1], 0.9 * miss[2]]
    for b in range(3):
        err = float(np.abs(wave[b] - ref[0][b]).max())
        print('clip', b, f'error {err:.3e} allowed {tol[b] + 8 * 2.0 ** -24 * peak:.3e}')
        assert err <= tol[b] + 8 * 2.0 ** -24 * peak                                          # at most 5 additions per sample round differently
    assert np.array_equal(wave[0], ref[0][0])                                               # the clip without a wet event: the same bits
    # ---- the targets are those of the same plan without ``rir``
    s2 = _scapes(bank, rirs=False)
    _, _, dt2 = s2.mix(s2.plan(BGS, EVENTS))
    assert dt2.blob.cpu().numpy().tobytes() == blob.tobytes()
    lst = dt.to_list()
    assert [t['labels'].tolist() for t in lst] == [[4], [4, 1], [7]]                          # the wet and the dry event of class 4 collapse
    # ---- a second batch into the same buffers
    wave3, _, dt3 = s.mix(plan)
    assert wave3.cpu().numpy().tobytes() == wave.tobytes() and dt3.blob.cpu().numpy().tobytes() == blob.tobytes()


def test_a_plan_of_dry_events_mixes_the_bits_of_a_plan_without(bank):
    from sound_event_detection_transformer_amd import lib as L
    s = _scapes(bank)
    plain = [[e[:7] for e in clip] for clip in EVENTS]
    wave0, _, dt0 = s.mix(s.plan(BGS, plain))
    wave0, blob0 = wave0.cpu().numpy().copy(), dt0.blob.cpu().numpy().copy()
    dry = s.plan(BGS, plain, [[-1] * len(c) for c in EVENTS])
    assert dry.rir is not None and dry.rir.tolist() == [-1] * 5 and dry.fx is None
    with L.launch_log() as log:
        wave1, _, dt1 = s.mix(dry)
    assert log['soundscape'] == 1 and log['reverb'] == 0 and log['reverb_bed'] == 0 and log['stretch'] == 0 and s.last_fx is None
    assert wave1.cpu().numpy().tobytes() == wave0.tobytes() and dt1.blob.cpu().numpy().tobytes() == blob0.tobytes()
    with L.launch_log() as log:                              # ... and with the stretch stage alone the calls of before
        s.mix(s.plan(BGS, EVENTS, [[-1] * len(c) for c in EVENTS]))
    assert log['soundscape'] == 1 and log['stretch'] == 1 and log['reverb'] == 0 and log['reverb_bed'] == 0
    with L.launch_log() as log:
        s.mix(s.plan(BGS, EVENTS, RIRS))
    assert log['soundscape'] == 1 and log['stretch'] == 1 and log['reverb'] == 1 and log['reverb_bed'] == 1
    # wet events need responses; a response the bank does not hold is refused on the host
    with pytest.raises(ValueError, match='add_rirs'):
        _scapes(bank, rirs=False).mix(s.plan(BGS, EVENTS, RIRS))
    with pytest.raises(ValueError, match='names response 7'):
        s.mix(s.plan(BGS, EVENTS, [[-1], [7, -1, 2], [1]]))
    # a wet event whose record lies outside the bank: its clip's status, as without reverb
    _, _, dt4 = s.mix(s.plan([None, None], [[(0, 1, 500, 700, 100, 0.5, 16)], [EVENTS[1][0]]], [[0], [0]]))
    assert dt4.status.cpu().tolist() == [2, 0]


def test_drawn_plans_with_reverb(bank):
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    s = _scapes(bank)
    np.random.seed(8)
    plan = s.draw(4, n_events=(1, 3), reverb=0.5, max_event_seconds=0.1)
    assert plan.rir is not None and (plan.rir >= 0).any() and (plan.rir < 0).any() and plan.fx is None
    np.random.seed(8)
    both = s.draw(4, n_events=(1, 3), reverb=True, pitch_shift=(-3.0, 3.0), time_stretch=(0.8, 1.2), max_event_seconds=0.1)
    assert (both.rir >= 0).all() and both.fx is not None
    for p in (plan, both):
        for b in range(4):
            own = {int(r) for r in p.rir[p.ev_off[b]:p.ev_off[b + 1]] if r >= 0}
            assert own <= {0, 2} or own <= {1}              # one room per clip
        wave, _, dt = s.mix(p)
        assert not dt.status.any().item() and not s.last_rv_status.any().item() and torch.isfinite(wave).all().item()
    with pytest.raises(ValueError, match='add_rirs'):
        _scapes(bank, rirs=False).draw(2, reverb=True)


def test_train_on_recordings_takes_wet_soundscapes(monkeypatch):
    """engine.train_on_recordings over two steps of batch() with reverb=0.5: the stages run inside the loop, nothing synchronises"""
    import test_soundscape_gpu as T
    from sound_event_detection_transformer_amd import engine, lib, runtime
    runtime.set_compute_dtype('bf16')
    try:
        B = 2
        scapes, transform, model, opt, stepper = T._train_setup(B)
        gen = np.random.default_rng(3)
        scapes.add_rirs([(gen.standard_normal(L) * np.exp(-6.0 * np.arange(L) / L)).astype(np.float32) for L in (800, 3000)], rooms=[0, 1])
        draw = scapes.draw
        plans = []
        monkeypatch.setattr(scapes, 'draw', lambda n: plans.append(draw(n, reverb=0.5, max_event_seconds=1.0)) or plans[-1])
        scapes.mix(scapes.draw(B))                           # the buffers and the workspace are made before the loop, as a warm-up makes them
        del plans[:]
        calls = {'sync': 0}
        real = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a_, **k_: (calls.__setitem__('sync', calls['sync'] + 1), real(*a_, **k_))[1])
        np.random.seed(31)
        with lib.launch_log() as log:
            out = engine.train_on_recordings(stepper, scapes, transform, 2)
        monkeypatch.setattr(torch.cuda, 'synchronize', real)
        wet_steps = sum(bool((p.rir >= 0).any()) for p in plans)
        assert len(plans) == 2 and wet_steps >= 1 and any((p.rir < 0).any() for p in plans)
        assert log['soundscape'] == 2 and log['reverb'] == wet_steps and log['reverb_bed'] == wet_steps and calls['sync'] == 0
        if (plans[-1].rir >= 0).any():
            assert len(scapes.last_fx['reverb_jobs']) == int((plans[-1].rir >= 0).sum())
        total, _ = out
        torch.cuda.synchronize()
        assert bool(torch.isfinite(total).all())
    finally:
        runtime.set_compute_dtype('f32')
