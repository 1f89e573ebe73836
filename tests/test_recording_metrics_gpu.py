"""GPU: recordings scored against their annotations on the device (csrc/recmetrics.hip through ops.recording_event_counts /
ops.recording_segment_counts and utilities.recording_metrics.RecordingMetrics).  Stitch-layout buffers are hand-built on the device
(tests/recording_metrics_ref.stitch_buffers); every comparison is integer equality of counters against the clip-level oracles
applied to the whole recording (event_metrics_ref.clip_event_counts / clip_tag_counts, segment_metrics_ref.clip_segment_counts, through
recording_metrics_ref.recording_counts).  The last test runs a RecordingDetector with ``metrics=`` on a C2 model's own outputs."""
import numpy as np
import pytest
import torch

import recording_metrics_ref as M
from test_recording_metrics_cpu import augmenting_case, exact_collar_cases

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


def _labels(C):
    return [f'c{i}' for i in range(C)]


def _metrics(C, K, rho=None, optimal=True, t_collar=0.2, fusion=(1,)):
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording_metrics import RecordingMetrics
    dec = EventDecoder(_labels(C), 10.0, thresholds=[(k + 1) / (K + 1) for k in range(K)], fusion_strategy=fusion)
    return RecordingMetrics(dec, t_collar=t_collar, optimal=optimal, time_resolution=rho)


def _device(count, out, status):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (count, out, status))


def _score(est, reference, filenames, C, K, cap, durations=None, rho=None, optimal=True, t_collar=0.2):
    """est {(k, r, c): [(onset, offset)]} through RecordingMetrics against the oracle: returns (metrics, want, stitched)"""
    m = _metrics(C, K, rho, optimal, t_collar).set_reference(reference)
    stitched = {1: _device(*M.stitch_buffers(est, K, len(filenames), C, cap, fill=GUARD))}
    m.update(stitched, cap, filenames, durations=durations)
    want = M.recording_counts(est, reference, filenames, _labels(C), K, t_collar, 0.2, optimal, rho)
    ev, tag = m.counts()
    assert np.array_equal(ev[0], want[0]), (ev[0].tolist(), want[0].tolist())
    assert np.array_equal(tag[0], want[1]), (tag[0].tolist(), want[1].tolist())
    if rho is not None:
        seg, sdi = m.segment_counts()
        assert np.array_equal(seg[0], want[2]), (seg[0].tolist(), want[2].tolist())
        assert np.array_equal(sdi[0], want[3]), (sdi[0].tolist(), want[3].tolist())
    return m, want, stitched


def _raw(est, refs_by_class, K=1, C=1, cap=8, rec_idx=(0,), n_rec=1, optimal=True, t_collar=0.2, buffers=None):
    """one raw ops.recording_event_counts launch: refs_by_class [[(onset, offset)] per class] of ONE reference recording, written
    as given (not sorted) -> (ev [K, C, 3], tag [K, C, 3], status [K, R]) as numpy"""
    from sound_event_detection_transformer_amd import ops
    R = len(rec_idx)
    count, out, st = _device(*(buffers or M.stitch_buffers(est, K, R, C, cap, fill=GUARD)))
    off = np.concatenate([[0], np.cumsum([len(r) for r in refs_by_class])]).astype(np.int32)
    flat = [e for r in refs_by_class for e in r] or [(0.0, 0.0)]
    table = {'off': torch.from_numpy(off).cuda(), 'on': torch.tensor([e[0] for e in flat], dtype=torch.float64).cuda(),
             'end': torch.tensor([e[1] for e in flat], dtype=torch.float64).cuda(), 'n_rec': n_rec, 'n_events': int(off[-1])}
    ev = torch.zeros((1, K, C, 3), dtype=torch.int64).cuda()
    tag = torch.zeros((1, K, C, 3), dtype=torch.int64).cuda()
    status = torch.full((K, R), -7, dtype=torch.int32).cuda()
    ops.recording_event_counts(count, out, st, cap, torch.tensor(list(rec_idx), dtype=torch.int32).cuda(), table, ev, tag, 0,
                               t_collar=t_collar, optimal=optimal, status=status)
    torch.cuda.synchronize()
    return ev[0].cpu().numpy(), tag[0].cpu().numpy(), status.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- event counts
def _small_case():
    """R = 3, C = 3, K = 2, the second recording absent from the reference, one reference empty, class c1 absent from 'a.wav'"""
    reference = {'a.wav': [('c0', 1.0, 2.0), ('c2', 3.0, 5.0), ('c0', 1.1, 2.5), ('c0', 8.0, 9.0)], 'empty.wav': []}
    filenames = ['empty.wav', 'nobody.wav', 'a.wav']
    est = {(0, 0, 1): [(0.5, 1.0)], (0, 0, 2): [(0.2, 0.4), (2.0, 3.0)], (1, 0, 2): [(2.0, 3.0)],
           (0, 1, 0): [(1.0, 2.0)], (1, 1, 1): [(1.0, 2.0)],
           (0, 2, 0): [(1.05, 2.1), (2.2, 2.6), (7.9, 9.1)], (0, 2, 1): [(4.0, 4.5)], (0, 2, 2): [(3.1, 4.0)],
           (1, 2, 0): [(1.05, 2.1)], (1, 2, 2): [(3.1, 4.9)]}
    return est, reference, filenames


@pytest.mark.parametrize('optimal', [True, False])
def test_three_recordings_one_absent_one_empty(optimal):
    est, reference, filenames = _small_case()
    m, want, _ = _score(est, reference, filenames, 3, 2, 4, optimal=optimal)
    assert m.recording_index(filenames).tolist() == [1, -1, 0]
    assert want[0][0].tolist() == [[2, 3, 3], [0, 0, 2], [0, 1, 3]] and want[0][1, 2].tolist() == [1, 1, 2]
    assert want[1][0].tolist() == [[1, 0, 0], [0, 2, 0], [1, 1, 0]]          # presence {tp, fp, fn}: 'empty.wav' gives false positives


def test_a_thousand_references_in_one_recording():
    """no 64-event limit: 1000 references and 900 estimates of one class in one recording (cap 1024), next to a class with few"""
    rng = np.random.default_rng(7)
    on = np.cumsum(rng.choice([0.6, 0.75, 1.0, 1.5], 1000))
    reference = {'long.wav': [('c0', float(t), float(t + 0.25)) for t in on] + [('c1', 5.0, 6.0)]}
    keep = np.sort(rng.choice(1000, 900, replace=False))
    est = {(0, 0, 0): [(float(on[i] + rng.uniform(-0.22, 0.22)), float(on[i] + 0.25 + rng.uniform(-0.02, 0.02))) for i in keep],
           (0, 0, 1): [(5.1, 6.1)]}
    est[(0, 0, 0)] = sorted(est[(0, 0, 0)])
    est[(1, 0, 0)] = est[(0, 0, 0)][::3]
    for optimal in (True, False):
        _, want, _ = _score(est, reference, ['long.wav'], 2, 2, 1024, optimal=optimal)
        assert want[0][0, 0, 1:].tolist() == [1000, 900] and 500 < want[0][0, 0, 0] < 900 and want[0][1, 0, 2] == 300


@pytest.mark.parametrize('optimal', [True, False])
def test_seeded_dense_lists(optimal):
    """blocks of many events, overlapping references, six recordings and two thresholds in one launch; segments at 0.5 s as well"""
    from test_recording_metrics_cpu import _dense_lists
    rng = np.random.default_rng(31)
    reference, est, names = {}, {}, [f'r{r}' for r in range(6)]
    for r, name in enumerate(names):
        refs, ests = _dense_lists(rng, int(rng.integers(10, 120)), int(rng.integers(5, 40)), float(rng.choice([5.0, 20.0, 60.0])))
        reference[name] = [(c, max(on, 0.0), max(off, 0.0)) for c, on, off in refs]
        for c in range(2):
            mine = [e[1:] for e in ests if e[0] == c]
            est[(0, r, c)], est[(1, r, c)] = mine, mine[::2]
    _, want, _ = _score(est, reference, names, 2, 2, 64, durations=[150.0] * 6, rho=0.5, optimal=optimal)
    assert want[0][0, :, 0].sum() > 60 and want[3].min() > 0


def test_a_chain_of_200_blocks():
    reference = {'r': [('c0', 1.0 * i, 1.0 * i + 0.5) for i in range(200)]}
    est = {(0, 0, 0): [(1.0 * i + (0.1 if i % 3 else 0.3), 1.0 * i + 0.5) for i in range(200)]}
    _, want, _ = _score(est, reference, ['r'], 1, 1, 256)
    assert want[0][0, 0].tolist() == [133, 200, 200]
    assert len(M.blocks([e[0] for e in est[(0, 0, 0)]], [1.0 * i for i in range(200)], 0.2)[0]) >= 200


def _full_block(n_est, n_ref):
    est = [(0.01 * i, 0.01 * i + 0.005) for i in range(n_est)]
    refs = [(0.005 + 0.01 * i, 0.012 + 0.01 * i) for i in range(n_ref)]
    return est, refs


def test_block_of_64_by_64_is_accepted_and_65_is_status_2():
    est, refs = _full_block(64, 64)
    for optimal in (True, False):
        _, want, _ = _score({(0, 0, 0): est}, {'r': [('c0',) + e for e in refs]}, ['r'], 1, 1, 128, optimal=optimal)
        assert want[0][0, 0].tolist() == [64, 64, 64]
    for n_est, n_ref in ((65, 64), (64, 65)):
        est, refs = _full_block(n_est, n_ref)
        assert M.blocks([e[0] for e in est], [e[0] for e in refs], 0.2)[1] == M.OVER_CAPACITY
        ev, tag, status = _raw({(0, 0, 0): est}, [refs], cap=128)
        assert status.tolist() == [[M.OVER_CAPACITY]]
        m = _metrics(1, 1).set_reference({'dense.wav': [('c0',) + e for e in refs]})
        m.update({1: _device(*M.stitch_buffers({(0, 0, 0): est}, 1, 1, 1, 128))}, 128, ['dense.wav'])
        with pytest.raises(RuntimeError, match=r"'dense.wav' at threshold 0.5: status 2 .*one block"):
            m.compute()
    # a 65th behind a cut is the next block
    est, refs = _full_block(64, 64)
    _score({(0, 0, 0): est + [(0.9, 0.95)]}, {'r': [('c0',) + e for e in refs + [(0.91, 0.96)]]}, ['r'], 1, 1, 128)


def test_exact_collar_cuts_and_the_augmenting_path():
    for collar, ref, est, _, tp in exact_collar_cases():
        for optimal in (True, False):
            _, want, _ = _score({(0, 0, 0): [est[1:]]}, {'r': [('c0',) + ref[1:]]}, ['r'], 1, 1, 4, optimal=optimal, t_collar=collar)
            assert want[0][0, 0].tolist() == [tp, 1, 1]
    refs, ests = augmenting_case()
    for optimal, tp in ((True, 2), (False, 1)):
        _, want, _ = _score({(0, 0, 0): [e[1:] for e in ests]}, {'r': [('c0',) + r[1:] for r in refs]}, ['r'], 1, 1, 4, optimal=optimal)
        assert want[0][0, 0].tolist() == [tp, 2, 2]


@pytest.mark.parametrize('C,K', [(1, 1), (63, 1), (63, 3)])
def test_class_and_threshold_envelope(C, K):
    rng = np.random.default_rng(C + K)
    reference = {'r': [(int(c), float(on), float(on + 0.5)) for c in range(C) for on in np.cumsum(rng.choice([0.6, 1.0, 3.0], 5))],
                 's': [(C - 1, 1.0, 2.0)]}
    est = {(k, r, c): [(float(on) + 0.1 * k, float(on) + 0.45) for on in np.cumsum(rng.choice([0.6, 1.0, 3.0], 4))]
           for k in range(K) for r in range(2) for c in range(0, C, 2)}
    for k in range(K):
        est[(k, 1, C - 1)] = [(1.05 + 0.01 * k, 2.0)]                      # a hit in the last class of the second recording
    _, want, _ = _score(est, reference, ['r', 's'], C, K, 8, durations=[20.0, 20.0], rho=1.0)
    assert want[0][:, C - 1, 0].sum() > 0 and want[2].sum() > 0


# ---------------------------------------------------------------------------------------------------------------- status
def test_stitch_status_and_overflow_give_status_1():
    est, reference, filenames = _small_case()
    count, out, st = M.stitch_buffers(est, 2, 3, 3, 4, fill=GUARD)
    st[1, 2] = 2                                                           # the stitch raised a status for ('a.wav', threshold 1)
    m = _metrics(3, 2, rho=1.0).set_reference(reference)
    m.update({1: _device(count, out, st)}, 4, filenames, durations=[10.0] * 3)
    with pytest.raises(RuntimeError, match=r"'a.wav' at threshold 0.6\d*: status 1 .*not complete"):
        m.compute()
    assert [s[0].cpu().numpy().tolist() for s in m._status] == [[[0, 0, 0], [0, 0, 1]]] * 2
    ev = m.ev.cpu().numpy()[0]
    want = M.recording_counts(est, reference, filenames, _labels(3), 2)[0]
    want[1] = M.recording_counts(est, reference, ['empty.wav', 'nobody.wav', 'not-counted'], _labels(3), 2)[0][1]
    assert np.array_equal(ev, want)                                         # the other recordings and thresholds are counted


def test_count_above_cap_reads_nothing_behind_cap():
    """count > cap: status 1, nothing counted.  And a count AT cap next to a buffer whose slots behind the lists hold non-finite and
    out-of-order times: they are not read"""
    from sound_event_detection_transformer_amd import ops
    refs = [(1.0 * i, 1.0 * i + 0.5) for i in range(6)]
    est = {(0, 0, 0): [(1.0 * i + 0.05, 1.0 * i + 0.5) for i in range(5)], (0, 0, 1): [(0.5, 0.75)]}
    count, out, st = M.stitch_buffers(est, 1, 1, 2, 4, fill=GUARD)           # cap 4: the fifth estimate is not in the buffer
    assert count[0, 0].tolist() == [5, 1]
    ev, tag, status = _raw(None, [refs, []], C=2, cap=4, buffers=(count, out, st))
    assert status.tolist() == [[M.INCOMPLETE]] and not ev.any() and not tag.any()
    # cap 6, four live events in class 0, one in class 1; everything behind them poisoned
    count, out, st = M.stitch_buffers({(0, 0, 0): est[(0, 0, 0)][:4], (0, 0, 1): est[(0, 0, 1)]}, 1, 1, 2, 6)
    times = ops.stitch_events_views(out)[0]
    times[0, 0, 0, 4] = (float('nan'), float('inf'))
    times[0, 0, 0, 5] = (-5.0, 0.25)
    times[0, 0, 1, 1:] = [(0.25, float('nan')), (0.0, 0.5), (float('-inf'), 1.0), (1.05, 1.5), (2.05, 2.5)]
    ev, tag, status = _raw(None, [refs, []], C=2, cap=6, buffers=(count, out, st))
    assert status.tolist() == [[0]] and ev[0].tolist() == [[4, 6, 4], [0, 0, 1]] and tag[0].tolist() == [[1, 0, 0], [0, 1, 0]]
    m = _metrics(2, 1, rho=0.5).set_reference({'r': [('c0',) + e for e in refs]})
    m.update({1: _device(count, out, st)}, 6, ['r'], durations=[6.0])
    want = M.recording_counts({(0, 0, 0): est[(0, 0, 0)][:4], (0, 0, 1): est[(0, 0, 1)]}, {'r': [('c0',) + e for e in refs]}, ['r'],
                              _labels(2), 1, rho=0.5)
    seg, sdi = m.segment_counts()
    assert np.array_equal(seg[0], want[2]) and np.array_equal(sdi[0], want[3])


def test_descending_or_non_finite_lists_give_status_4():
    good = [(1.0, 1.5), (2.0, 2.5), (3.0, 3.5)]
    for est, refs in (([(2.0, 2.5), (1.0, 1.5)], good), (good, [(2.0, 2.5), (1.0, 1.5)]), ([(1.0, float('nan'))], good),
                      (good, [(float('inf'), 1.0)]), ([(float('nan'), 1.0)], good)):
        ev, tag, status = _raw({(0, 0, 0): est}, [refs])
        assert status.tolist() == [[M.UNORDERED]] and not ev.any() and not tag.any(), (est, refs)
    # 4 before 2: class 0 holds a block over capacity, class 1 a descending list
    est, refs = _full_block(65, 64)
    ev, tag, status = _raw({(0, 0, 0): est, (0, 0, 1): [(2.0, 2.5), (1.0, 1.5)]}, [refs, good], C=2, cap=128)
    assert status.tolist() == [[M.UNORDERED]]
    # a rec_idx outside the table is skipped
    ev, tag, status = _raw({(0, 0, 0): good, (0, 1, 0): good, (0, 2, 0): good}, [good], rec_idx=(5, -3, 0))
    assert status.tolist() == [[0, 0, 0]] and ev[0].tolist() == [[3, 3, 3]]


def test_arguments_are_checked_on_the_host():
    for kw, msg in ((dict(C=64), 'C=64'), (dict(t_collar=-1.0), 't_collar'), (dict(t_collar=float('nan')), 't_collar')):
        a = dict(C=1, t_collar=0.2)
        a.update(kw)
        with pytest.raises(RuntimeError, match='recording_event_counts.*' + msg):
            _raw({}, [[] for _ in range(a['C'])], C=a['C'], t_collar=a['t_collar'])
    ev, tag, status = _raw({}, [[]], rec_idx=())                            # R == 0 launches nothing
    assert not ev.any() and status.shape == (1, 0)


# ---------------------------------------------------------------------------------------------------------------- segments
@pytest.mark.parametrize('rho', [1.0, 0.1])
def test_segments_at_word_edges(rho):
    """recordings of exactly 64, 65 and 130 segments; events ending exactly on segment 64 and 128; a long reference event covering
    several later ones; 0.3 / 0.1-style quotients"""
    u = rho
    reference = {'w64': [('c0', 0.3 * u, 64 * u), ('c1', 10 * u, 11 * u), ('c1', 0.3, 0.7)],
                 'w65': [('c0', 63 * u, 65 * u), ('c1', 0.0, 0.3 * u)],
                 'w130': [('c0', 2 * u, 128 * u), ('c0', 5 * u, 6 * u), ('c0', 60 * u, 70 * u), ('c0', 127.5 * u, 129.25 * u),
                          ('c1', 64 * u, 64 * u), ('c1', 100 * u, 130 * u)]}
    filenames = ['w64', 'w65', 'w130']
    est = {(0, 0, 0): [(0.0, 0.3 * u), (0.3 * u, 0.6 * u), (32 * u, 64 * u)], (0, 0, 1): [(0.3, 0.6), (10.5 * u, 12 * u)],
           (0, 1, 0): [(0.0, 64 * u), (64 * u, 64.5 * u)], (0, 1, 1): [(0.3 * u, 0.7 * u)],
           (0, 2, 0): [(0.0, 1 * u), (64 * u, 128 * u), (128 * u, 130 * u)], (0, 2, 1): [(63.9 * u, 64.1 * u), (99 * u, 128 * u)],
           (1, 2, 1): [(0.0, 130 * u)]}
    m, want, _ = _score(est, reference, filenames, 2, 2, 4, durations=[64 * u, 65 * u, 130 * u], rho=rho)
    outer = dict(reference, w130=[e for e in reference['w130'] if e[1:] not in ((5 * u, 6 * u), (60 * u, 70 * u))])
    assert len(outer['w130']) == 4 and want[3].sum() > 0                    # the long reference event covers the ones inside it
    assert np.array_equal(M.recording_counts(est, outer, filenames, _labels(2), 2, rho=rho)[2], want[2])
    res = m.compute()
    assert res[1][0]['segment']['overall']['Nref'] == int(want[2][0, :, 1].sum())


def test_five_thousand_segments():
    rng = np.random.default_rng(50)
    reference = {'r': [(int(rng.integers(0, 3)), float(on), float(on + rng.choice([0.3, 2.0, 40.0]))) for on in rng.uniform(0, 490, 60)]}
    est = {}
    for c in range(3):
        on = np.cumsum(rng.choice([0.7, 3.0, 30.0], 40))
        est[(0, 0, c)] = [(float(t), float(t + 0.65)) for t in on if t < 495]
    est[(0, 0, 2)] = [(0.05, 0.1), (499.95, 500.0)]                            # the first and the last segment
    _, want, _ = _score(est, reference, ['r'], 3, 1, 64, durations=[500.0], rho=0.1)
    assert want[2][0, :, 1].sum() > 1000 and want[3][0].sum() > 0
    # the references run past the recording: the span follows the largest reference offset
    _score({(0, 0, 0): [(1.0, 2.0)]}, {'r': [('c0', 1.5, 700.0)]}, ['r'], 1, 1, 4, durations=[10.0], rho=1.0)


# ---------------------------------------------------------------------------------------------------------------- reproducibility
def test_two_runs_equal_bytes_updates_accumulate_reset_zeroes():
    est, reference, filenames = _small_case()
    m, want, stitched = _score(est, reference, filenames, 3, 2, 4, durations=[10.0] * 3, rho=1.0)
    first = [t.clone() for t in m.counters()]
    m.reset()
    assert not any(bool(t.any()) for t in m.counters())
    m.update(stitched, 4, filenames, durations=[10.0] * 3)
    assert all(torch.equal(a, b) for a, b in zip(first, m.counters()))
    m.update(stitched, 4, filenames, durations=[10.0] * 3)
    assert all(torch.equal(2 * a, b) for a, b in zip(first, m.counters()))
    assert np.array_equal(m.counts()[0][0], 2 * want[0])


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_detector_with_metrics_end_to_end():
    from test_recording_gpu import HOP, WIN, _c2_model
    from sound_event_detection_transformer_amd import engine, runtime
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector
    from sound_event_detection_transformer_amd.utilities.recording_metrics import RecordingMetrics
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    model, _, post = _c2_model()
    try:
        C, fusion = 10, (1, 2)
        labels = _labels(C)
        mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
        n = WIN + 3 * HOP + 32000                                          # 26 s: 5 windows
        wave = (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(77))).numpy()
        sizes = torch.full((4,), 10.0).cuda()
        amp, nframes = mel([wave[s:s + WIN] for s in (0, HOP, 2 * HOP, 3 * HOP)])
        scores = engine.detect_step(model, post, transform(amp, nframes=nframes), sizes, fusion)[1][1][0].cpu().numpy()
        grid = [float(np.quantile(scores, q)) for q in (0.5, 0.8)]          # a fresh seeded model scores low: thresholds from its own scores
        dec = EventDecoder(labels, 10.0, thresholds=grid, fusion_strategy=fusion)
        det = RecordingDetector(model, post, dec, mel, transform, 10.0, 5.0, batch_windows=4, merge_gap=0.25)
        preds, _ = det([wave], ['noise.wav'])
        rows = preds[1].to_rows(0)
        assert len(rows) > 3
        # the reference: the detector's own events at the lower threshold, shifted by less than the collar; one dropped, one added
        reference = {'noise.wav': [(lab, on + 0.1, off + 0.15) for lab, on, off, _, _ in rows[1:]] + [(labels[3], 30.0, 31.0)]}
        m = RecordingMetrics(dec, time_resolution=1.0).set_reference(reference)
        res = engine.evaluate_recordings(det, m, [([wave], ['noise.wav'])])
        ev, tag = m.counts()
        seg, sdi = m.segment_counts()
        for i, f in enumerate(fusion):
            est = {(k, 0, labels.index(lab)): [] for k in range(2) for lab in labels}
            for k in range(2):
                for lab, on, off, _, _ in preds[f].to_rows(k):
                    est[(k, 0, labels.index(lab))].append((on, off))
            want = M.recording_counts(est, reference, ['noise.wav'], labels, 2, rho=1.0)
            assert np.array_equal(ev[i], want[0]) and np.array_equal(tag[i], want[1]), f
            assert np.array_equal(seg[i], want[2]) and np.array_equal(sdi[i], want[3]), f
        assert ev[0, 0, :, 0].sum() >= len(rows) - 2 and res[1][0]['f1'] > 0 and len(res[2]) == 2
        from sound_event_detection_transformer_amd.utilities.operating_points import select_class_wise
        assert m.class_wise_thresholds(1)['thresholds'].tolist() == select_class_wise(ev[0], dec.threshold_values)['thresholds'].tolist()
        # metrics=None: the same predictions bit for bit
        again, _ = det([wave], ['noise.wav'], metrics=None)
        scored, _ = det([wave], ['noise.wav'], metrics=m)
        for other in (again, scored):
            for f in fusion:
                for k in range(2):
                    a, b = preds[f].at(k), other[f].at(k)
                    assert all(np.array_equal(a[c], b[c]) for c in a), (f, k)
    finally:
        runtime.set_compute_dtype('bf16')
