"""CPU: the NumPy restatement of sedt_mixup_plan (tests/mixup_plan_ref.py) against its oracle, the host plan
(utilities.mixup.plan_mixup_data on the list form, then TargetTables.load(mixed, ns=, n_lab=)) - offsets, split words, live labels,
boxes, ratios and the job records, everything exact - and the host half of mix-up and mean-teacher training on recordings: the three
kinds of recordings, draw_split, DeviceTargets with a split, the static-split prefix load on CPU tensors, every refusal of the envelope.
The kernel itself: tests/test_mixup_plan_gpu.py."""
import collections

import numpy as np
import pytest
import torch

import mixup_plan_ref as R

LABELS = ['Speech', 'Dog', 'Cat', 'Bird']
SEED, CASES = 0, 120                # chosen here, on the CPU, so that every outcome occurs at least five times (asserted below)


def _same(ref, tables, jobs):
    R.assert_same_tables({k: ref[k] for k in ('off', 'lab', 'box', 'ratio')}, tables)
    R.assert_same_jobs(ref['jobs'], jobs)


# ---------------------------------------------------------------------------------------------------- the reference against the host plan
def test_reference_equals_the_host_plan_on_random_cases():
    rng = np.random.default_rng(SEED)
    seen = collections.Counter()
    for _ in range(CASES):
        c = R.random_case(rng)
        ref = R.reference(c)
        tables, jobs = R.oracle(c, torch)
        _same(ref, tables, jobs)
        assert not ref['status'].any()
        host = R.host_outcomes(c, jobs)                              # counted on the host plan's side
        assert host == collections.Counter(ref['outcomes'])
        seen += host
    for outcome in (R.KEEP1_EMPTY, R.KEEP2, R.WEAK, R.KEEP1_EVENTS, R.KEEP1_OVERLAP, R.STRONG):
        assert seen[outcome] >= 5, (outcome, dict(seen))


@pytest.mark.parametrize('name', [n for n in R.designed_cases() if n != 'capacity + 1'])
def test_reference_equals_the_host_plan_on_the_designed_cases(name):
    c = R.designed_cases()[name]
    ref = R.reference(c)
    _same(ref, *R.oracle(c, torch))
    assert not ref['status'].any()


def test_designed_cases_are_what_they_are_named():
    d = R.designed_cases()
    out = lambda n: R.reference(d[n])['outcomes']
    assert out('B1') == [] and out('B2 both merge') == [R.STRONG, R.STRONG]
    assert out('B5 partner weak, two clips one partner, self') == [R.KEEP1_EMPTY, R.WEAK, R.KEEP1_OVERLAP]
    assert out('B5 empty partner either side, partner unlabelled') == [R.KEEP1_EMPTY, R.KEEP2, R.KEEP1_EMPTY]
    assert out('B5 both empty') == [R.WEAK, R.WEAK] and R.reference(d['B5 both empty'])['off'][-2:].tolist() == [1, 4]
    assert out('max_events reached') == [R.STRONG] * 2 and out('max_events + 1') == [R.KEEP1_EVENTS] * 2
    assert out('boxes touch') == [R.KEEP1_OVERLAP] and out('boxes miss by one ulp') == [R.STRONG]
    a, b = d['boxes touch']['clips'][1][1], d['boxes miss by one ulp']['clips'][1][1]
    assert b[0, 0] == np.nextafter(a[0, 0], np.float32(1)) and b[0, 1] == a[0, 1]
    assert out('overlap inside clip i') == [R.KEEP1_OVERLAP] and out('index[i] == i') == [R.KEEP1_OVERLAP, R.WEAK]
    # capacity: a result of exactly max_targets_out labels is complete; one more raises status 1 on its source clip and keeps the first
    full, over = R.reference(d['capacity reached']), R.reference(d['capacity + 1'])
    assert not full['status'].any() and np.diff(full['off'][:5]).tolist() == [1, 3, 3, 3]
    assert over['status'].tolist() == [1, 0, 1, 0] and np.diff(over['off'][:5]).tolist() == [1, 3, 3, 3]
    assert over['lab'].tolist() == [1, 0, 1, 2, 0, 1, 2, 0, 1, 2] and over['off'][-2:].tolist() == [1, 4]
    with pytest.raises(ValueError, match='more than max_targets=3'):      # the host route refuses such a batch outright
        R.oracle(d['capacity + 1'], torch)
    # a partner outside the batch: status 2, treated as keep-1
    c = dict(d['B2 both merge'], index=np.asarray([2, 0], np.int32))
    bad = R.reference(c)
    assert bad['status'].tolist() == [2, 0] and bad['jobs'].tolist()[0] == (0, 0, 1, 0.0) and bad['outcomes'][1] == R.STRONG


# ---------------------------------------------------------------------------------------------------- recordings of three kinds
class _Mel(object):
    sr, hop, F, min_samples = 1000, 100, 8, 200


def _clips(monkeypatch, **kw):
    from sound_event_detection_transformer_amd.utilities import recording_clips as RC

    def stage(waves, dev):                                          # the staging without pinned memory: this is a CPU test
        ns = [len(w) for w in waves]
        return torch.cat([torch.as_tensor(np.asarray(w, np.float32)) for w in waves]), None, ns, None
    monkeypatch.setattr(RC, 'stage_recordings', stage)
    return RC.RecordingClips(_Mel(), LABELS, 2.0, device='cpu', **kw)


def _wave(n):
    return np.zeros(n, np.float32)


def test_add_kinds_and_draw_split(monkeypatch):
    from sound_event_detection_transformer_amd.utilities import recording_clips as RC
    clips = _clips(monkeypatch)
    clips.add([_wave(5000), _wave(3000)], ['s0', 's1'], {'s0': [('Dog', 0.5, 1.0)], 's1': []})
    np.random.seed(3)
    a = clips.draw(4)                                               # only strong recordings: draw is what it was
    np.random.seed(3)
    b = RC.draw_picks([5000, 3000], 2000, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    clips.add([_wave(1500), _wave(6000)], ['w0', 'w1'], {'w0': ['Cat', 'Dog', 2, 'Cat'], 'w1': [3]}, kind='weak')
    clips.add([_wave(2500)], ['u0'], None, kind='unlabelled')
    assert clips.kinds == ['strong', 'strong', 'weak', 'weak', 'unlabelled'] and clips.names == ['s0', 's1', 'w0', 'w1', 'u0']
    # tags de-duplicated in input order (by class), staged from 0 to max(duration, window_seconds)
    assert clips.reference['w0'] == [(2, 0.0, 2.0), (1, 0.0, 2.0)] and clips.reference['w1'] == [(3, 0.0, 6.0)]
    assert clips.reference['u0'] == [] and clips.host['off'].tolist() == [0, 1, 1, 3, 4, 4]
    assert RC.weak_events(['Dog', 1, 'Speech'], LABELS, 3.5) == [(1, 0.0, 3.5), (0, 0.0, 3.5)]
    with pytest.raises(ValueError, match="recording 'w2': class 'Fish' is not one of the 4 labels"):
        clips.add([_wave(3000)], ['w2'], {'w2': ['Dog', 'Fish']}, kind='weak')
    with pytest.raises(ValueError, match="recording 'w2' has no entry"):
        clips.add([_wave(3000)], ['w2'], {}, kind='weak')
    with pytest.raises(ValueError, match="kind 'tagged' is not one of"):
        clips.add([_wave(3000)], ['w2'], {'w2': []}, kind='tagged')
    with pytest.raises(ValueError, match="recording 'u0' is staged twice"):
        clips.add([_wave(3000)], ['u0'], None, kind='unlabelled')
    assert len(clips) == 5
    with pytest.raises(RuntimeError, match='draw_split'):
        clips.draw(4)
    # draw_split: kind by kind, strong first, each one draw_picks over that kind's recordings
    np.random.seed(9)
    rec, start = clips.draw_split(3, 2, 4)
    np.random.seed(9)
    s = RC.draw_picks([5000, 3000], 2000, 3)
    w = RC.draw_picks([1500, 6000], 2000, 2)
    u = RC.draw_picks([2500], 2000, 4)
    assert rec.tolist() == s[0].tolist() + (w[0] + 2).tolist() + (u[0] + 4).tolist() and rec.dtype == np.int32
    assert start.tolist() == s[1].tolist() + w[1].tolist() + u[1].tolist() and start.dtype == np.int64
    assert clips.draw_split(0, 2)[0].tolist() in ([2, 2], [2, 3], [3, 2], [3, 3])
    with pytest.raises(ValueError, match='no clips asked for'):
        clips.draw_split(0)
    only = _clips(monkeypatch).add([_wave(3000)], ['s'], {'s': []})
    with pytest.raises(ValueError, match='no weak recording is staged'):
        only.draw_split(1, 1)
    # the split of a cut: the kinds of the picked recordings must be strong | weak | unlabelled in that layout
    assert clips.check_split(np.asarray([0, 1, 2, 4]), (2, 3)) == (2, 3) and clips.check_split(np.asarray([1, 0]), None) == (2, 2)
    with pytest.raises(ValueError, match="clip 1 is cut from the weak recording 'w0', the split 2 | 2 of 2 wants a strong one"):
        clips.check_split(np.asarray([0, 2]), None)
    with pytest.raises(ValueError, match="clip 2 is cut from the strong recording 's1'.*wants a weak one"):
        clips.check_split(np.asarray([0, 1, 1]), (2, 3))
    with pytest.raises(ValueError, match=r'split 3 \| 2 outside'):
        clips.check_split(np.asarray([0, 1, 1]), (3, 2))


def _device_targets(clips, M, **kw):
    from sound_event_detection_transformer_amd.utilities.recording_clips import DeviceTargets
    B = len(clips)
    return DeviceTargets(torch.from_numpy(R.source_blob(clips, M)), torch.zeros(B, dtype=torch.int32), B, M, [f'r{b}' for b in range(B)], 10.0,
                         **kw)


FIVE = R.designed_cases()['B5 of a source of 7']['clips']           # 3 strong | 1 weak | 1 unlabelled | two more


def test_device_targets_with_a_split():
    dt = _device_targets(FIVE[:5], 4)
    assert (dt.ns, dt.n_lab) == (5, 5) and [len(t['boxes']) for t in dt.to_list()] == [2, 0, 1, 2, 0]       # the positional form: all strong
    dt = _device_targets(FIVE[:5], 4, ns=3, n_lab=4)
    lst = dt.to_list()
    assert [t['labels'].tolist() for t in lst] == [[3, 1], [], [1], [4, 5], []]
    assert [tuple(t['boxes'].shape) for t in lst] == [(2, 2), (0, 2), (1, 2), (0, 2), (0, 2)]
    hidden = _device_targets(FIVE[:5], 4, ns=2, n_lab=2).to_list()
    assert [t['labels'].tolist() for t in hidden] == [[3, 1], [], [], [], []] and all(len(t['boxes']) == 0 for t in hidden[2:])
    with pytest.raises(ValueError, match=r'split 4 \| 3 outside 0..5'):
        _device_targets(FIVE[:5], 4, ns=4, n_lab=3)


@pytest.mark.parametrize('B,ns,n_lab', [(5, 3, 4), (4, 3, 4), (3, 3, 3), (3, 0, 3), (7, 7, 7)])
def test_static_split_prefix_load(B, ns, n_lab):
    """load(DeviceTargets) onto static-split tables == load(list) of the same clips: every part of the smaller layout is a prefix of the
    source's part"""
    from sound_event_detection_transformer_amd.sedt import TargetTables
    M = 4
    clips = [c if b < ns or b >= 5 else (c[0], c[1][:0]) for b, c in enumerate(FIVE)] if ns == 0 else FIVE
    dt = _device_targets(clips, M, ns=min(ns, 7), n_lab=max(n_lab, min(ns, 7)))
    want = TargetTables(B, ns, n_lab, torch.device('cpu'), max_targets=M, with_ratio=True).load(R.to_list(clips[:B], ns, n_lab, torch))
    got = TargetTables(B, ns, n_lab, torch.device('cpu'), max_targets=M, with_ratio=True)
    got.ratio_cat.fill_(0.5)
    got.load(dt)
    nl, nb = int(want.off[B]), int(want.off[B + 1 + ns])
    assert got.off[:B + ns + 2].tolist() == want.off[:B + ns + 2].tolist()
    assert got.lab_cat[:nl].tolist() == want.lab_cat[:nl].tolist() and torch.equal(got.box_cat[:nb], want.box_cat[:nb])
    assert got.ratio_cat.eq(1.0).all()


def test_static_split_load_refusals():
    from sound_event_detection_transformer_amd.sedt import TargetTables
    cpu, M = torch.device('cpu'), 4
    dt = _device_targets(FIVE, M, ns=3, n_lab=4)
    with pytest.raises(ValueError, match=r'3 strong \| 4 labelled of 7 clips.*hold 2 strong \| 4 labelled of 5'):
        TargetTables(5, 2, 4, cpu, max_targets=M).load(dt)
    with pytest.raises(ValueError, match='these tables hold 3 strong'):
        TargetTables(8, 3, 4, cpu, max_targets=M).load(dt)                          # more clips than the source has
    with pytest.raises(ValueError, match='max_targets=5'):
        TargetTables(5, 3, 4, cpu, max_targets=5).load(dt)
    with pytest.raises(NotImplementedError, match='load_mixed'):
        TargetTables(5, 3, 4, cpu, max_targets=M, dynamic_split=True, with_ratio=True).load(dt)
    with pytest.raises(ValueError, match='expected 5 clips, got 7'):                 # host lists keep their check
        TargetTables(5, 3, 4, cpu, max_targets=M).load(R.to_list(FIVE, 3, 4, torch))


def test_load_mixed_refusals():
    """everything load_mixed refuses on the host, before anything is launched (CPU tables: the launch itself would be refused last)"""
    from sound_event_detection_transformer_amd.sedt import TargetTables
    cpu, M = torch.device('cpu'), 4
    dt = _device_targets(FIVE, M, ns=3, n_lab=4)
    jobs = torch.zeros(16 * 5, dtype=torch.uint8)
    dyn = lambda B=5: TargetTables(B, 3, 4, cpu, max_targets=M, dynamic_split=True, with_ratio=True)
    with pytest.raises(ValueError, match='dynamic_split=True, with_ratio=True'):
        TargetTables(5, 3, 4, cpu, max_targets=M).load_mixed(dt, 0.5, np.arange(5), 2, 4, jobs)
    with pytest.raises(ValueError, match='dynamic_split=True, with_ratio=True'):
        TargetTables(5, 3, 4, cpu, max_targets=M, dynamic_split=True).load_mixed(dt, 0.5, np.arange(5), 2, 4, jobs)
    with pytest.raises(ValueError, match='targets built on the device'):
        dyn().load_mixed(R.to_list(FIVE[:5], 3, 4, torch), 0.5, np.arange(5), 2, 4, jobs)
    with pytest.raises(ValueError, match='expected at least 8 clips, got 7'):
        dyn(8).load_mixed(dt, 0.5, np.arange(8), 2, 4, jobs)
    for index in (np.arange(4), [0, 1, 2, 3, 5], [0, -1, 2, 3, 4]):                   # status 2 never reaches the kernel from here
        with pytest.raises(ValueError, match=r'one partner in 0\.\.4 per clip'):
            dyn().load_mixed(dt, 0.5, index, 2, 4, jobs)
    for mix_num in (4, -1):
        with pytest.raises(ValueError, match='needs as many strong clips, the batch has 3'):
            dyn().load_mixed(dt, 0.5, np.arange(5), mix_num, 4, jobs)
    for max_events in (0, 5):
        with pytest.raises(ValueError, match=r'outside 1\.\.max_targets=4'):
            dyn().load_mixed(dt, 0.5, np.arange(5), 2, max_events, jobs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dyn().load_mixed(dt, 0.5, np.arange(5), 2, 4, jobs)


def test_entry_point_refuses_outside_the_envelope():
    """1 <= B <= B_src <= 1024, 0 <= ns <= n_lab <= B, 0 <= mix_num <= ns, 1 <= max_events <= max_targets_out <= 63, refused with a
    message before a pointer is touched (every pointer here is null)"""
    from sound_event_detection_transformer_amd import _build, lib
    _build.build()
    l = lib.load()

    def call(B_src=8, M_src=32, B=8, ns=4, n_lab=6, mix_num=2, max_events=20, M_out=32):
        assert l.sedt_mixup_plan(None, B_src, M_src, B, ns, n_lab, None, None, mix_num, max_events, M_out, None, None, None, None) != 0
        return l.sedt_last_error().decode()
    for kw in (dict(B=0), dict(B=9), dict(B_src=1025, B=1025), dict(B_src=-1), dict(ns=-1), dict(ns=7), dict(n_lab=9), dict(mix_num=-1),
               dict(mix_num=5)):
        msg = call(**kw)
        assert 'outside the envelope' in msg and '1024' in msg and 'mix_num' in msg, (kw, msg)
    for kw in (dict(max_events=0), dict(max_events=33), dict(M_out=64, max_events=64), dict(M_out=0), dict(M_src=0), dict(M_src=64)):
        msg = call(**kw)
        assert 'outside the envelope' in msg and '63' in msg and 'max_events' in msg, (kw, msg)
    assert 'null pointer' in call()                                                 # inside the envelope: the pointers are looked at
    assert 'null pointer' in call(B_src=1024, B=1024, ns=1024, n_lab=1024, mix_num=1024, max_events=63, M_out=63, M_src=63)
    assert 'null pointer' in call(B=1, ns=0, n_lab=0, mix_num=0, max_events=1, M_out=1, M_src=1)
