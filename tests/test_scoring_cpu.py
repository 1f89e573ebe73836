"""CPU: the reference tables the five scorers share (utilities/scoring.py: ClipReference, RecordingReference) on device='cpu': the
arrays against literals, every refusal with its message, the PSDS constants by hand, the generation rule, and what a scorer that counts
segments adds on a shared reference."""
import re

import numpy as np
import pytest
import torch

LABELS = ['a', 'b', 'c']
# clip 0 has no row in the reference, clip 1 an empty one; ('b', 2, 2) has no length; a class may be given by its index
EVENTS = [None, [], [('a', 1.0, 3.0), ('b', 2.0, 2.0)], [('c', 0.5, 1.5), (0, 4.0, 6.5)]]
DURATIONS = [10.0, 8.0, 6.0, 4.0]


def _clip(events=EVENTS, durations=DURATIONS, **kw):
    from sound_event_detection_transformer_amd.utilities.scoring import ClipReference
    return ClipReference(LABELS, 'cpu').set(events, durations, **kw)


def _decoder(K=2):
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    return EventDecoder(LABELS, 10.0, thresholds=[0.3, 0.7][:K], device='cpu')


def test_clip_table_arrays_and_dtypes():
    r = _clip()
    want = {'present': ([0, 1, 1, 1], torch.int32), 'off': ([0, 0, 0, 2, 4], torch.int32), 'cls': ([0, 1, 2, 0], torch.int32),
            'on': ([1.0, 2.0, 0.5, 4.0], torch.float64), 'end': ([3.0, 2.0, 1.5, 6.5], torch.float64),
            'dur': ([10.0, 8.0, 6.0, 4.0], torch.float64)}
    assert sorted(r.table) == sorted(want) == sorted(r.host)
    for k, (values, dtype) in want.items():
        assert r.table[k].dtype == dtype and r.table[k].tolist() == values, k
        assert r.host[k].tolist() == values and torch.from_numpy(r.host[k]).dtype == dtype, k
    assert (r.n_clips, r.n_events, r.max_ref) == (4, 4, 2)
    # without durations every clip has the default; an empty list still gives arrays a launch can be handed
    assert _clip(durations=None, default_duration=7.5).table['dur'].tolist() == [7.5] * 4
    e = _clip([], None)
    assert (e.n_clips, e.max_ref) == (0, 0) and e.table['off'].tolist() == [0] and all(e.table[k].numel() == 1 for k in e.table)


def test_clip_psds_constants_by_hand():
    r = _clip()
    assert r.n_gt.tolist() == [2, 0, 1] and r.n_gt.dtype == np.int64            # the zero-length event of 'b' is left out
    assert r.gt_dur.tolist() == [2.0 + 2.5, 0.0, 1.0]
    assert r.total_dur == 8.0 + 6.0 + 4.0                                        # clip 0 is not present


@pytest.mark.parametrize('events,durations,message', [
    ([[(7, 0.0, 1.0)]], None, 'set_reference: clip 0: class 7 is not one of the 3 labels'),
    ([[], [('a', 0.0, float('inf'))]], None, 'set_reference: clip 1: non-finite event time'),
    ([[], [('a', float('nan'), 1.0)]], None, 'set_reference: clip 1: non-finite event time'),
    ([[('a', 0.0, 1.0)] * 65], None, 'set_reference: clip 0 has 65 reference events (at most 64)'),
    ([[], []], [1.0], 'set_reference: 1 durations for 2 clips'),
    ([[]], [-1.0], 'set_reference: clip 0: duration -1.0 is not a finite non-negative number of seconds'),
    ([[], None], [1.0, float('nan')], 'set_reference: clip 1: duration nan is not a finite non-negative number of seconds'),
])
def test_clip_refusals_keep_their_messages(events, durations, message):
    """the refusals of EventMetrics.set_reference and PsdsMetrics.set_reference, word for word; through the scorers too"""
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
    r = _clip()
    before = {k: v.clone() for k, v in r.table.items()}
    with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
        r.set(events, durations)
    assert all(torch.equal(r.table[k], before[k]) for k in before) and r.n_clips == 4       # a refusal leaves the table alone
    with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
        PsdsMetrics(_decoder()).set_reference(events, durations)
    if durations is None:
        with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
            EventMetrics(LABELS, 10.0, device='cpu').set_reference(events)
    _clip([[('a', 0.0, 1.0)] * 64], None)                                        # 64 events in a clip are held


def test_clip_generation_rule():
    r = _clip()
    gen, tensors = r.generation, dict(r.table)
    r.set([[('b', 0.0, 1.0)], None, [('c', 1.0, 2.0), ('c', 3.0, 4.0)], [('a', 5.0, 6.0)]], [1.0, 2.0, 3.0, 4.0])
    assert r.generation == gen and all(r.table[k] is tensors[k] for k in tensors)           # same shape: written in place
    assert r.table['cls'].tolist() == [1, 2, 2, 0] and r.table['present'].tolist() == [1, 0, 1, 1] and r.total_dur == 8.0
    r.set([[('b', 0.0, 1.0), ('b', 2.0, 3.0), ('b', 4.0, 5.0)], None, [], []], [1.0] * 4)     # fits, but max_ref 2 -> 3
    assert r.generation > gen and all(r.table[k] is tensors[k] for k in tensors)
    gen = r.generation
    r.set(EVENTS + [[('a', 0.0, 1.0)]], DURATIONS + [1.0])                                   # a longer list: new tensors
    assert r.generation > gen and r.table['present'] is not tensors['present'] and r.n_clips == 5


def test_clip_index_is_checked_against_the_table():
    r = _clip()
    assert r.host_clip_index([3, -1, 0]).tolist() == [3, -1, 0] and r.host_clip_index([3]).dtype == torch.int32
    for bad in (4, -2):
        with pytest.raises(ValueError, match=f'clip index {bad} outside -1 .. 3'):
            r.host_clip_index([0, bad])


def test_a_shared_clip_reference_and_the_segment_checks():
    """EventMetrics(time_resolution=...) keeps its own checks - negative times, MAX_SEGMENTS, n_seg_words - and runs them on the shared
    reference's host arrays; a PsdsMetrics or SweepEventMetrics holding the same reference does not inherit them"""
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    from sound_event_detection_transformer_amd.utilities.operating_points import SweepEventMetrics
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
    negative = _clip([[('a', 1.0, 2.0)], [('b', -0.5, 1.0)]], None)
    psds, sweep = PsdsMetrics(_decoder()).set_reference(negative), SweepEventMetrics(_decoder()).set_reference(negative)
    assert psds.reference is sweep.reference is negative and psds.table is negative.table
    assert psds.n_gt.tolist() == [1, 1, 0] and psds.gt_dur.tolist() == [1.0, 1.5, 0.0] and psds.total_dur == 20.0
    EventMetrics(LABELS, 10.0, device='cpu').set_reference(negative)                        # no segments: accepted
    seg = EventMetrics(LABELS, 10.0, device='cpu', time_resolution=1.0)
    with pytest.raises(ValueError, match=re.escape('set_reference: clip 1: negative event time (-0.5, 1.0) in a segment-based evaluation')):
        seg.set_reference(negative)
    assert seg.table is None and seg.reference is not negative
    with pytest.raises(ValueError, match='negative event time'):
        seg.set_reference([[('a', 1.0, 2.0)], [('b', -0.5, 1.0)]])
    assert seg.table is None
    PsdsMetrics(_decoder()).set_reference([[('a', 1.0, 2.0)], [('b', -0.5, 1.0)]])           # the PSDS path alone takes the list
    long = _clip([[('a', 0.0, 1025.0)]], None)
    with pytest.raises(ValueError, match='more than 1024 segments per clip'):
        seg.set_reference(long)
    shared = _clip()
    seg.set_reference(shared)
    assert seg.reference is shared and seg.n_seg_words == 1 and (seg.n_clips, seg.max_ref) == (4, 2)
    # whoever sets the shared reference, the scorer that counts segments is asked first and follows: its words, and with them
    # its generation, which a captured step compares
    gen, psds_gen = seg.generation, psds.set_reference(shared).generation
    psds.set_reference([None, [], [('a', 1.0, 70.0), ('b', 2.0, 2.0)], [('c', 0.5, 1.5), (0, 4.0, 6.5)]], DURATIONS)   # in place
    assert psds.reference is shared and seg.n_seg_words == 2 and seg.generation > gen and psds.generation == psds_gen
    before, gen = {k: v.clone() for k, v in shared.table.items()}, seg.generation
    for refused in ([[('a', 0.0, 500.0)], [('b', -3.0, 2.0)]], [[('a', 0.0, 1025.0)]]):
        with pytest.raises(ValueError, match='negative event time|more than 1024 segments'):
            shared.set(refused)
        with pytest.raises(ValueError, match='negative event time|more than 1024 segments'):
            sweep.set_reference(shared).set_reference(refused)
    assert all(torch.equal(shared.table[k], before[k]) for k in before) and shared.n_clips == 4      # a refusal leaves the table alone
    assert seg.n_seg_words == 2 and seg.generation == gen
    # a scorer that swaps to another reference changes its generation, also to a reference older than its own last change
    older = _clip()
    mine = EventMetrics(LABELS, 10.0, device='cpu', time_resolution=1.0).set_reference(EVENTS)
    gen, table = mine.generation, mine.table
    assert mine.set_reference(older).generation != gen and mine.table is older.table is not table
    gen = sweep.generation
    assert sweep.set_reference(older).generation != gen
    seg.set_reference(older)                                # released: the reference it left no longer asks it
    shared.set([[('b', -3.0, 2.0)]])
    with pytest.raises(ValueError, match='labels'):
        EventMetrics(['x', 'y'], 10.0, device='cpu').set_reference(shared)
    with pytest.raises(ValueError, match='carries its own durations'):
        psds.set_reference(shared, DURATIONS)


# ---------------------------------------------------------------------------------------------------------------- recordings
REFERENCE = {'empty.wav': [], 'a.wav': [('c', 5.0, 9.0), ('a', 20.0, 21.0), ('b', 4.0, 6.0), ('a', 1.0, 3.5), (1, 0.5, 3.0), ('b', 7.0, 7.0)]}


def _recordings(reference=REFERENCE, **kw):
    from sound_event_detection_transformer_amd.utilities.scoring import RecordingReference
    return RecordingReference(LABELS, 'cpu').set(reference, **kw)


def test_recording_table_arrays_constants_and_index():
    r = _recordings()
    t = r.table
    assert (t['n_rec'], t['n_events']) == (2, 6) and sorted(t) == ['end', 'n_events', 'n_rec', 'off', 'on']
    assert t['off'].dtype == torch.int32 and t['off'].tolist() == [0, 0, 0, 0, 2, 5, 6]
    assert t['on'].dtype == torch.float64 and t['on'].tolist() == [1.0, 20.0, 0.5, 4.0, 7.0, 5.0]     # per class, sorted by onset
    assert t['end'].dtype == torch.float64 and t['end'].tolist() == [3.5, 21.0, 3.0, 6.0, 7.0, 9.0]
    assert r.host['names'] == ['empty.wav', 'a.wav'] and r.host['max_end'].tolist() == [0.0, 21.0]
    assert r.recording_index(['a.wav', 'nobody.wav', 'empty.wav']).tolist() == [1, -1, 0]
    assert r.recording_index([]).dtype == np.int32
    assert r.with_pmax() is t and t['pmax'].tolist() == [3.5, 21.0, 3.0, 6.0, 7.0, 9.0]
    n, dur = r.constants()
    assert n.tolist() == [[0, 0, 0], [2, 2, 1]] and dur.tolist() == [[0.0, 0.0, 0.0], [3.5, 4.5, 4.0]]   # ('b', 7, 7) is left out
    overlapping = _recordings({'r': [('a', 0.0, 9.0), ('a', 1.0, 2.0), ('a', 3.0, 4.0)]})
    assert overlapping.with_pmax()['pmax'].tolist() == [9.0, 9.0, 9.0]
    e = _recordings({})
    assert (e.table['n_rec'], e.table['n_events']) == (0, 0) and e.table['off'].tolist() == [0] and e.table['on'].numel() == 1


@pytest.mark.parametrize('events,segments,message', [
    ([('z', 0.0, 1.0)], False, "set_reference: recording 'r.wav': class 'z' is not one of the 3 labels"),
    ([(3, 0.0, 1.0)], False, "set_reference: recording 'r.wav': class 3 is not one of the 3 labels"),
    ([('a', 0.0, float('inf'))], False, "set_reference: recording 'r.wav': non-finite event time (0.0, inf)"),
    ([('a', -1.0, 2.0)], True, "set_reference: recording 'r.wav': negative event time (-1.0, 2.0) in a segment-based evaluation"),
])
def test_recording_refusals_keep_their_messages(events, segments, message):
    from sound_event_detection_transformer_amd.utilities.recording_metrics import RecordingMetrics
    with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
        _recordings({'ok.wav': [], 'r.wav': events}, segments=segments)
    with pytest.raises(ValueError, match='^' + re.escape(message) + '$'):
        RecordingMetrics(_decoder(), time_resolution=1.0 if segments else None, device='cpu').set_reference({'r.wav': events})


def test_a_shared_recording_reference():
    """both recording scorers on one RecordingReference; the one that counts segments refuses negative times on it, the other does not"""
    from sound_event_detection_transformer_amd.utilities import recording_metrics, recording_psds, scoring
    assert recording_metrics.reference_table is scoring.reference_table and recording_metrics.status_error is scoring.status_error
    assert recording_psds.prefix_max is scoring.prefix_max and recording_psds.reference_constants is scoring.reference_constants
    assert callable(recording_metrics.segment_words)
    dec = _decoder()
    shared = _recordings()
    m = recording_metrics.RecordingMetrics(dec, time_resolution=1.0, device='cpu').set_reference(shared)
    p = recording_psds.RecordingPsds(dec, device='cpu').set_reference(shared)
    assert m.reference is p.reference is shared and m.host is shared.host and m.table is shared.table
    assert p.table is shared.table and 'pmax' in p.table
    assert m.recording_index(['a.wav', 'x']).tolist() == p.recording_index(['a.wav', 'x']).tolist() == [1, -1]
    idx, dur = p.account(['a.wav', 'nobody.wav', 'empty.wav'], [30.0, 10.0, 10.0])
    assert idx.tolist() == [1, -1, 0] and p.n_gt.tolist() == [2, 2, 1] and p.gt_dur.tolist() == [3.5, 4.5, 4.0] and p.total_dur == 40.0
    negative = _recordings({'q.wav': [], 'r.wav': [('b', 3.0, 4.0), ('a', -1.0, 2.0)]})
    recording_psds.RecordingPsds(dec, device='cpu').set_reference(negative)
    recording_metrics.RecordingMetrics(dec, device='cpu').set_reference(negative)
    with pytest.raises(ValueError, match='negative event time'):
        recording_metrics.RecordingMetrics(dec, time_resolution=1.0, device='cpu').set_reference(negative)
    table = shared.table                                    # m counts segments and holds ``shared``: it is asked whoever sets it
    with pytest.raises(ValueError, match='negative event time'):
        p.set_reference({'q.wav': [], 'r.wav': [('b', 3.0, 4.0), ('a', -1.0, 2.0)]})
    assert shared.table is table and shared.host['names'] == ['empty.wav', 'a.wav']
    with pytest.raises(ValueError, match='labels'):
        recording_psds.RecordingPsds(dec, device='cpu').set_reference(scoring.RecordingReference(['x'], 'cpu').set({}))


def test_read_back_splits_one_copy_and_raises_through_status_error():
    from sound_event_detection_transformer_amd.utilities.scoring import read_back
    a, b = torch.arange(6, dtype=torch.int64).reshape(2, 3), torch.tensor([[7]], dtype=torch.int64)
    got = read_back([a, b])
    assert [g.tolist() for g in got] == [a.tolist(), b.tolist()] and all(g.dtype == np.int64 for g in got)
    ok = (torch.zeros((2, 2), dtype=torch.int32), ['x.wav', 'y.wav'], [0.3, 0.7], 'launch one')
    bad = (torch.tensor([[0, 0], [0, 4]], dtype=torch.int32), ['x.wav', 'y.wav'], [0.3, 0.7], 'launch two')
    assert [g.tolist() for g in read_back([a], [ok])] == [a.tolist()]
    with pytest.raises(RuntimeError, match=re.escape("launch two: recording 'y.wav' at threshold 0.7: status 4 (an event list is not ascending")):
        read_back([a, b], [ok, bad])


# ---------------------------------------------------------------------------------------------------------------- the sharing cases
# tests/test_scoring_shared_gpu.py runs these through the scorers once with one shared reference and once with separate ones; here
# the restatements show that the inputs count something everywhere, so that equality there is not vacuous
GRID4 = [0.2, 0.4, 0.6, 0.8]


def clip_sharing_case():
    """B = 5, Q = 8, C = 3, K = 4.  reference (per clip [(class index, onset, offset)]), the batch's clip indices (clip 1 is given as
    None, clip 2 is empty, the last entry is outside the table), per batch entry its detections [(class, onset, offset, score)]"""
    reference = [[(0, 1.0, 3.0), (1, 5.0, 9.0)], None, [], [(2, 2.0, 6.0), (0, 7.0, 8.0)]]
    dets = [[(0, 1.0, 3.0, 0.9),                       # the reference event itself: a true positive everywhere
             (1, 5.125, 7.0, 0.5),                     # onset inside the collar, offset not: an event-based miss; passes the DTC, fails the GTC
             (2, 0.5, 3.5, 0.7)],                      # no reference of class 2 in this clip: a cross trigger on class 0 and a false positive
            [(0, 1.0, 2.0, 0.9)],                      # a clip without a reference row: clip level only
            [(1, 2.0, 4.0, 0.65)],                     # an empty reference: a false positive
            [(2, 2.125, 5.875, 0.85), (0, 7.0, 8.0, 0.3)],
            [(2, 1.0, 2.0, 0.9)]]                      # index -1
    return reference, [0, 1, 2, 3, -1], dets


def host_records(dets, grid, C, Q=8):
    """the detections decoded on the host at every threshold of ``grid``: predictions.unpack's list, as tests/sweep_ref.counts takes it"""
    import sweep_ref as SR
    events = []
    for t in grid:
        rows = [(b,) + e[:3] for b, clip in enumerate(dets)
                for e in SR.decode_strong([d[3] for d in clip], [d[0] for d in clip], [d[1:3] for d in clip], [t] * C, max_len=10.0)]
        events.append({k: np.asarray([r[i] for r in rows]) for i, k in enumerate(('clip', 'cls', 'onset', 'offset'))})
    return events


def clip_sharing_counts():
    """(ev, tag [K, C, 3], psds counts [K, C, C + 1]) of clip_sharing_case by the restatements"""
    import psds_ref
    import sweep_ref as SR
    reference, idx, dets = clip_sharing_case()
    events = host_records(dets, GRID4, 3)
    ev, tag = SR.counts(events, idx, reference, 3)
    rows = [[(idx[b], c, on, off) for b, c, on, off in zip(e['clip'].tolist(), e['cls'].tolist(), e['onset'].tolist(), e['offset'].tolist())]
            for e in events]
    return ev, tag, np.asarray(psds_ref.counts(rows, reference, [10.0] * 4, LABELS), np.int64)


def test_the_clip_sharing_case_counts_everywhere():
    ev, tag, counts = clip_sharing_counts()
    assert ev[0].tolist() == [[2, 2, 2], [0, 1, 2], [1, 1, 2]]              # {tp, n_ref, n_sys} per class at 0.2; clips 0, 2 and 3 only
    assert ev[3, :, 0].sum() == 2 and ev[:, :, 0].sum() > 0 and (ev[0] != ev[3]).any()       # the thresholds differ
    assert tag[0].sum(0).tolist() == [4, 4, 0] and tag[1, :, 2].sum() == 1   # clip-level tp and fp; a fn once 0.3 is below the threshold
    K, C = 4, 3
    diagonal, world = counts[:, np.arange(C), np.arange(C)], counts[:, :, C]
    cross = counts[:, :, :C].sum() - diagonal.sum()
    assert diagonal[0].tolist() == [2, 0, 1] and world[0].tolist() == [0, 1, 1] and counts[0, 2, 0] == 1 and cross == 3
    assert (counts[0] != counts[3]).any() and diagonal[3].sum() == 2


def test_the_recording_sharing_case_counts_everywhere():
    """R = 3, C = 3, K = 2, cap = 4: tests/test_recording_psds_gpu.py's small case (one recording absent, one annotated empty)"""
    import recording_metrics_ref as M
    import recording_psds_ref as P
    from test_recording_psds_gpu import _small_case
    est, reference, filenames, durations = _small_case()
    labels = ['c0', 'c1', 'c2']
    assert len(filenames) == 3 and 'nobody.wav' not in reference and reference['empty.wav'] == []
    ev, tag, seg, sdi = M.recording_counts(est, reference, filenames, labels, 2, rho=1.0)
    assert ev[:, :, 0].sum() > 0 and all(tag[:, :, i].sum() > 0 for i in range(3)) and seg[:, :, 0].sum() > 0 and sdi.any(0).all()
    counts = P.oracle_counts(est, reference, filenames, durations, labels, 2)
    assert np.trace(counts[0][:, :3]) > 0 and counts[0][:, 3].sum() > 0 and counts[0][:, :3].sum() > np.trace(counts[0][:, :3])
