"""CPU: the host half of "Scoring recordings" (DESIGN.md section 4).  The block decomposition and the word sweep the kernels of
csrc/recmetrics.hip follow (restated in tests/recording_metrics_ref.py) give the counts of the clip-level oracles applied to a whole
recording; the reference table, the refusals, compute()'s finish and the threshold choice of
utilities.recording_metrics.RecordingMetrics."""
import numpy as np
import pytest

import event_metrics_ref as E
import recording_metrics_ref as M
import segment_metrics_ref as S

LABELS = ['a', 'b', 'c']


def _dense_lists(rng, n_ref, n_est, span, C=2):
    """seeded lists dense enough that blocks hold many events: references may overlap, the estimates of a class are disjoint"""
    refs = [(int(rng.integers(0, C)), float(on), float(on + rng.choice([0.05, 0.3, 1.0, 4.0]))) for on in rng.uniform(0, span, n_ref // 2)]
    ests = []
    for c in range(C):
        t = 0.0
        for _ in range(n_est):
            t += float(rng.choice([0.0, 0.05, 0.15, 0.3, 2.0]))
            d = float(rng.choice([0.05, 0.1, 0.3, 1.0]))
            ests.append((c, t, t + d))
            t += d
    for c, on, off in ests:                                                # references near estimates, so that hits exist
        if len(refs) < n_ref and rng.random() < 0.7:
            refs.append((c, on + float(rng.uniform(-0.25, 0.25)), off + float(rng.uniform(-0.25, 0.25))))
    return M.sort_refs(refs), ests


# ---------------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize('optimal', [True, False])
def test_block_decomposition_equals_the_whole_list_matchers(optimal):
    rng = np.random.default_rng(11)
    several = hits = 0
    for case in range(40):
        refs, ests = _dense_lists(rng, int(rng.integers(0, 60)), int(rng.integers(0, 30)), float(rng.choice([5.0, 20.0, 60.0])))
        got, status = M.block_event_counts(refs, ests, 2, 0.2, 0.2, optimal)
        want = E.clip_event_counts(refs, ests, 2, 0.2, 0.2, optimal)
        assert status == 0 and np.array_equal(got, want), (case, got.tolist(), want.tolist())
        several += len(M.blocks([e[1] for e in ests if e[0] == 0], [e[1] for e in refs if e[0] == 0], 0.2)[0]) > 1
        hits += int(want[:, 0].sum())
    assert several >= 20 and hits >= 100, (several, hits)


def exact_collar_cases():
    """(t_collar, reference, estimate, blocks, tp): consecutive onsets whose float64 difference is exactly t_collar (one block, a
    hit) and one ulp above (a cut, no hit)"""
    cases = []
    for collar, a in ((0.2, 0.0), (0.25, 1.0)):
        b = a + collar
        assert b - a == collar
        up = float(np.nextafter(b, 9.0))
        assert up - a > collar
        cases += [(collar, (0, a, a + 1.0), (0, b, b + 1.0), 1, 1), (collar, (0, a, a + 1.0), (0, up, up + 1.0), 0, 0),
                  (collar, (0, b, b + 1.0), (0, a, a + 1.0), 1, 1), (collar, (0, up, up + 1.0), (0, a, a + 1.0), 0, 0)]
    return cases


def test_cut_at_exactly_the_collar_and_one_ulp_above():
    for collar, ref, est, n_joint, tp in exact_collar_cases():
        bl, status = M.blocks([est[1]], [ref[1]], collar)
        assert status == 0 and sum(1 for _, a, _, b in bl if a and b) == n_joint, (collar, ref, est, bl)
        for optimal in (True, False):
            assert M.block_event_counts([ref], [est], 1, collar, 0.2, optimal)[0].tolist() == [[tp, 1, 1]]
            assert E.clip_event_counts([ref], [est], 1, collar, 0.2, optimal).tolist() == [[tp, 1, 1]]


def augmenting_case():
    """references r0, r1 in table order and disjoint estimates e0, e1 in onset order: r0 hits both, r1 hits e0 only - greedy gives r0
    the estimate r1 needs"""
    refs = [(0, 0.78, 0.98), (0, 0.79, 0.84)]
    ests = [(0, 0.8, 0.9), (0, 0.95, 1.05)]
    return refs, ests


def test_greedy_in_the_defined_order_finds_one_fewer_than_the_maximum():
    refs, ests = augmenting_case()
    assert M.sort_refs(refs) == refs and ests[0][2] <= ests[1][1]
    assert [[E.hit(r, e) for e in ests] for r in refs] == [[True, True], [True, False]]
    assert E.clip_event_counts(refs, ests, 1, optimal=True).tolist() == [[2, 2, 2]]
    assert E.clip_event_counts(refs, ests, 1, optimal=False).tolist() == [[1, 2, 2]]
    assert M.block_event_counts(refs, ests, 1, optimal=True)[0].tolist() == [[2, 2, 2]]
    assert M.block_event_counts(refs, ests, 1, optimal=False)[0].tolist() == [[1, 2, 2]]


def test_block_capacity():
    est = [0.01 * i for i in range(64)]
    ref = [0.005 + 0.01 * i for i in range(64)]
    assert M.blocks(est, ref, 0.2) == ([(0, 64, 0, 64)], 0)
    assert M.blocks(est + [0.64], ref, 0.2)[1] == M.OVER_CAPACITY and M.blocks(est, ref + [0.645], 0.2)[1] == M.OVER_CAPACITY
    assert M.blocks(est + [0.9], ref + [0.91], 0.2) == ([(0, 64, 0, 64), (64, 1, 64, 1)], 0)        # a 65th behind a cut is the next block
    assert M.blocks(est + [0.9, 0.95], ref, 0.2) == ([(0, 64, 0, 64)], 0)                           # what is left of one list is not walked


# ---------------------------------------------------------------------------------------------------------------- segments
@pytest.mark.parametrize('rho', [1.0, 0.1])
def test_word_sweep_equals_the_event_roll(rho):
    rng = np.random.default_rng(23)
    for case in range(12):
        span = float(rng.choice([3.0, 6.4, 13.0])) * (10 if rho == 1.0 else 1)
        refs, ests = _dense_lists(rng, int(rng.integers(0, 25)), int(rng.integers(0, 12)), span)
        refs = M.sort_refs([(c, max(on, 0.0), max(off, 0.0)) for c, on, off in refs])      # no negative times in a segment-based evaluation
        ests = [e for e in ests if e[2] <= span + 2]
        words = M.n_words(span + 2, refs, rho)
        cw, sdi = M.sweep_segment_counts(refs, ests, 2, rho, words)
        want_cw, want_sdi = S.clip_segment_counts(refs, ests, 2, rho)
        assert np.array_equal(cw, want_cw) and np.array_equal(sdi, want_sdi), (case, cw.tolist(), want_cw.tolist())
    refs, ests = [(0, 0.3, 6.4), (0, 0.5, 0.6), (1, 12.8, 13.0)], [(0, 0.0, 0.3), (1, 6.4, 12.8)]      # 0.3 / 0.1: floor 2; word edges
    cw, sdi = M.sweep_segment_counts(refs, ests, 2, rho, M.n_words(13.0, refs, rho))
    want = S.clip_segment_counts(refs, ests, 2, rho)
    assert np.array_equal(cw, want[0]) and np.array_equal(sdi, want[1])


# ---------------------------------------------------------------------------------------------------------------- the table
def test_reference_table_sorting_csr_empty_and_absent():
    from sound_event_detection_transformer_amd.utilities.recording_metrics import reference_table, segment_words
    ref = {'one.wav': [('b', 5.0, 6.0), ('a', 2.0, 9.0), ('b', 1.0, 3.0), ('b', 1.0, 2.0), (2, 0.5, 0.75), ('b', 1.0, 2.0)],
           'empty.wav': [], 'two.wav': [('c', 100.0, 130.5)]}
    t = reference_table(ref, LABELS)
    assert t['names'] == ['one.wav', 'empty.wav', 'two.wav'] and t['index'] == {'one.wav': 0, 'empty.wav': 1, 'two.wav': 2}
    assert t['off'].dtype == np.int32 and t['off'].tolist() == [0, 1, 5, 6, 6, 6, 6, 6, 6, 7]
    assert t['on'].dtype == np.float64 and t['on'].tolist() == [2.0, 1.0, 1.0, 1.0, 5.0, 0.5, 100.0]
    assert t['end'].tolist() == [9.0, 2.0, 2.0, 3.0, 6.0, 0.75, 130.5]                                   # (onset, offset, input order)
    assert t['max_end'].tolist() == [9.0, 0.0, 130.5] and 'absent.wav' not in t['index']
    empty = reference_table({}, LABELS)
    assert empty['off'].tolist() == [0] and empty['on'].size == 0 and empty['names'] == []
    assert segment_words(10.0, 0.0, 1.0) == 1 and segment_words(64.0, 0.0, 1.0) == 1 and segment_words(64.5, 0.0, 1.0) == 2
    assert segment_words(10.0, 130.5, 1.0) == 3 and segment_words(3600.0, 0.0, 0.01) == 5625 and segment_words(0.3, 0.0, 0.1) == 1


def test_refusals():
    from sound_event_detection_transformer_amd.utilities.recording_metrics import reference_table, segment_words, status_error
    with pytest.raises(ValueError, match="'x.wav'.*class 'zebra' is not one of the 3 labels"):
        reference_table({'x.wav': [('zebra', 0.0, 1.0)]}, LABELS)
    with pytest.raises(ValueError, match='class 3 is not one'):
        reference_table({'x.wav': [(3, 0.0, 1.0)]}, LABELS)
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match="'x.wav'.*non-finite"):
            reference_table({'x.wav': [('a', 0.0, bad)]}, LABELS)
    assert reference_table({'x.wav': [('a', -1.0, 1.0)]}, LABELS)['on'].tolist() == [-1.0]             # event-based only: allowed
    with pytest.raises(ValueError, match='negative event time'):
        reference_table({'x.wav': [('a', -1.0, 1.0)]}, LABELS, segments=True)
    with pytest.raises(ValueError, match='int32 indexing'):
        segment_words(1e12, 0.0, 0.001)
    assert status_error(np.zeros((2, 2), np.int32), ['p', 'q'], [0.3, 0.7], 'x') is None
    for code, why in ((1, 'not complete'), (2, 'one block'), (4, 'not ascending')):
        st = np.zeros((2, 2), np.int32)
        st[1, 0] = code
        err = status_error(st, ['p.wav', 'q.wav'], [0.3, 0.7], 'recording_event_counts')
        assert isinstance(err, RuntimeError) and "'p.wav'" in str(err) and 'threshold 0.7' in str(err) and f'status {code}' in str(err) \
            and why in str(err)


# ---------------------------------------------------------------------------------------------------------------- the finish
def _host_metrics(K=3, rho=None, **kw):
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording_metrics import RecordingMetrics
    dec = EventDecoder(LABELS, 10.0, thresholds=[0.3, 0.5, 0.7][:K], fusion_strategy=(1, 2), device='cpu')
    return RecordingMetrics(dec, time_resolution=rho, device='cpu', **kw)


def test_compute_finishes_hand_made_counters_with_finalize():
    from sound_event_detection_transformer_amd.utilities.metrics import finalize
    m = _host_metrics(rho=1.0)
    assert m.ev.shape == (2, 3, 3, 3) and m.sdi.shape == (2, 3, 3) and not any(t.any() for t in m.counters())
    rng = np.random.default_rng(3)
    ev = rng.integers(0, 9, (2, 3, 3, 3))
    ev[..., 0] = np.minimum(ev[..., 0], np.minimum(ev[..., 1], ev[..., 2]))
    ev[:, :, 2, 1:] = 0                                                    # class c: in no reference and never detected
    tag, seg, sdi = rng.integers(0, 4, (2, 3, 3, 3)), rng.integers(0, 50, (2, 3, 3, 3)), rng.integers(0, 20, (2, 3, 3))
    tag[:, :, 2] = 0
    import torch
    for dst, src in ((m.ev, ev), (m.tag, tag), (m.seg, seg), (m.sdi, sdi)):
        dst.copy_(torch.from_numpy(src))
    res = m.compute()
    assert set(res) == {1, 2} and all(len(res[f]) == 3 for f in res)
    for i, f in enumerate((1, 2)):
        for k in range(3):
            want = finalize(ev[:, k], tag[:, k], LABELS, (1, 2), at_counted=False, seg=seg[:, k], sdi=sdi[:, k])[f]
            assert res[f][k] == want and set(want['class_wise']) == {'a', 'b'} and 'segment' in want and 'clip' in want
            tp, nr, ns = (int(v) for v in ev[i, k, 0])
            assert want['class_wise']['a']['f1'] == (2 * tp / (nr + ns) if nr + ns else 0.0)
    got = m.counts()
    assert np.array_equal(got[0], ev) and np.array_equal(got[1], tag) and np.array_equal(m.segment_counts()[1], sdi)
    m.reset()
    assert not any(t.any() for t in m.counters())
    plain = _host_metrics()
    assert plain.segment_counts() is None and 'segment' not in plain.compute()[1][0]
    with pytest.raises(RuntimeError, match='set_reference'):
        plain.update({}, 4, ['x.wav'])
    for kw in (dict(t_collar=-0.1), dict(t_collar=float('nan')), dict(rho=0.0), dict(rho=float('inf'))):
        with pytest.raises(ValueError):
            _host_metrics(**kw)


def test_class_wise_thresholds_is_select_class_wise_on_ev():
    import torch
    from sound_event_detection_transformer_amd.utilities.operating_points import select_class_wise
    m = _host_metrics()
    ev = np.zeros((2, 3, 3, 3), np.int64)
    ev[1, :, 0] = [[2, 10, 30], [6, 10, 12], [4, 10, 5]]                   # class a: best at 0.5
    ev[1, :, 1] = [[5, 6, 7], [5, 6, 6], [1, 6, 1]]                        # class b: best at 0.5 too; class c has no reference
    m.ev.copy_(torch.from_numpy(ev))
    got, want = m.class_wise_thresholds(2), select_class_wise(ev[1], np.asarray([0.3, 0.5, 0.7], np.float32))
    assert got['index'].tolist() == want['index'].tolist() == [1, 1, -1] and got['f1'] == want['f1'] > 0
    assert got['thresholds'].tolist() == want['thresholds'].tolist() and got['class_f1'].tolist() == want['class_f1'].tolist()
    assert m.class_wise_thresholds(1)['f1'] == 0.0
