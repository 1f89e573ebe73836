"""GPU: scorers that hold ONE reference (utilities/scoring.py: ClipReference, RecordingReference) count what scorers with a reference
each count: every counter tensor bit for bit, the statuses and the PSDS constants.  No model: synthetic PostProcess tensors and
hand-written stitched lists, the cases of tests/test_scoring_cpu.py, where the restatements show that they count something everywhere
(true positives, cross triggers, false positives, clips and recordings outside the reference, several thresholds)."""
import numpy as np
import pytest
import torch

import recording_metrics_ref as M
from test_psds_gpu import _clips
from test_recording_psds_gpu import GUARD, _device, _small_case
from test_scoring_cpu import GRID4, LABELS, clip_sharing_case, clip_sharing_counts

pytestmark = pytest.mark.gpu


def _clip_scorers(shared):
    """the four consumers of one batch: EventMetrics.update, EventDecoder.decode, SweepEventMetrics.update, PsdsMetrics.update"""
    from sound_event_detection_transformer_amd.utilities.metrics import EventMetrics
    from sound_event_detection_transformer_amd.utilities.operating_points import SweepEventMetrics
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.psds import PsdsMetrics
    from sound_event_detection_transformer_amd.utilities.scoring import ClipReference
    reference, idx, dets = clip_sharing_case()
    named = [None if ev is None else [(LABELS[c], on, off) for c, on, off in ev] for ev in reference]
    decoder = EventDecoder(LABELS, 10.0, thresholds=GRID4)
    scorers = [EventMetrics(LABELS, 10.0, time_resolution=1.0), SweepEventMetrics(decoder), PsdsMetrics(decoder)]
    one = ClipReference(LABELS, decoder.device).set(named, default_duration=10.0) if shared else None
    for m in scorers:
        m.set_reference(one if shared else named)
    results = {1: tuple(torch.from_numpy(t).cuda() for t in _clips(dets, 8))}
    metrics, sweep, psds = scorers
    metrics.update(results, None, idx)
    decoded = decoder.decode(results, None)
    sweep.update(decoded, idx)
    psds.update(decoded, idx)
    torch.cuda.synchronize()
    return scorers


def test_clip_scorers_on_one_shared_reference():
    """B = 5, Q = 8, C = 3, K = 4; clip indices with a clip given as None, an empty clip and -1"""
    shared, separate = _clip_scorers(True), _clip_scorers(False)
    assert len({id(m.reference) for m in shared}) == 1 and len({id(m.reference) for m in separate}) == 3
    for a, b in zip(shared, separate):
        assert len(a.counters()) == len(b.counters()) and (a.n_clips, a.max_ref) == (b.n_clips, b.max_ref) == (4, 2)
        for x, y in zip(a.counters(), b.counters()):
            assert torch.equal(x, y) and bool(x.any()), type(a).__name__
    assert shared[0].n_seg_words == separate[0].n_seg_words == 1
    psds = shared[2]
    assert np.array_equal(psds.n_gt, separate[2].n_gt) and np.array_equal(psds.gt_dur, separate[2].gt_dur)
    assert psds.total_dur == separate[2].total_dur == 30.0
    # and both are what the restatements count for these inputs
    ev, tag, counts = clip_sharing_counts()
    assert np.array_equal(shared[1].counts()[0][0], ev) and np.array_equal(shared[1].counts()[1][0], tag)
    assert np.array_equal(psds.counts_host()[0], counts)
    assert np.array_equal(shared[0].counts()[0][0], ev[1])          # EventMetrics decodes at 0.5, and no score lies in [0.4, 0.5)


def _recording_scorers(shared):
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording_metrics import RecordingMetrics
    from sound_event_detection_transformer_amd.utilities.recording_psds import RecordingPsds
    from sound_event_detection_transformer_amd.utilities.scoring import RecordingReference
    est, reference, filenames, durations = _small_case()
    labels, K, C, cap = ['c0', 'c1', 'c2'], 2, 3, 4
    decoder = EventDecoder(labels, 10.0, thresholds=[1 / 3, 2 / 3])
    scorers = [RecordingMetrics(decoder, time_resolution=1.0), RecordingPsds(decoder)]
    one = RecordingReference(labels, decoder.device).set(reference) if shared else None
    stitched = {1: _device(*M.stitch_buffers(est, K, len(filenames), C, cap, fill=GUARD))}
    for m in scorers:
        m.set_reference(one if shared else reference)
        m.update(stitched, cap, filenames, durations=durations)
    torch.cuda.synchronize()
    return scorers


def test_recording_scorers_on_one_shared_reference():
    """R = 3 hand-written stitched lists, K = 2, C = 3, cap = 4; one recording absent from the reference, one annotated empty"""
    shared, separate = _recording_scorers(True), _recording_scorers(False)
    assert shared[0].reference is shared[1].reference and separate[0].reference is not separate[1].reference
    for a, b in zip(shared, separate):
        for x, y in zip(a.counters(), b.counters()):
            assert torch.equal(x, y) and bool(x.any()), type(a).__name__
        assert len(a._status) == len(b._status) > 0
        for s, t in zip(a._status, b._status):
            assert torch.equal(s[0], t[0]) and s[1:] == t[1:]
        assert a.recording_index(['a.wav', 'nobody.wav', 'empty.wav']).tolist() == [1, -1, 0]
    p, q = shared[1], separate[1]
    assert p.n_gt.tolist() == q.n_gt.tolist() == [2, 2, 1] and p.gt_dur.tolist() == q.gt_dur.tolist() == [3.5, 4.5, 4.0]
    assert p.total_dur == q.total_dur == 40.0
    for a, b in zip(shared[0].counts() + shared[0].segment_counts(), separate[0].counts() + separate[0].segment_counts()):
        assert np.array_equal(a, b)                                  # read back through the statuses: none is raised
    assert np.array_equal(p.counts_host(), q.counts_host())
