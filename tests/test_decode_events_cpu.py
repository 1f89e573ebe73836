"""CPU: the host half of the device decode (utilities/predictions.py) on a hand-written packed buffer, the restatement of decode_strong
(tests/event_metrics_ref.py) against the reference's own function at a grid of thresholds (fixture G23), and the new entry point in
the C ABI.  The kernel itself is compared with the same restatement and fixtures in tests/test_decode_events_gpu.py."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import event_metrics_ref as R

G23_SHAPES = ((1, 1), (21, 10), (64, 63))


# ---------------------------------------------------------------------------------------------------------------- decode_strong
@pytest.mark.parametrize('Q,C', G23_SHAPES)
@pytest.mark.parametrize('del_overlap', [1, 0])
def test_restatement_matches_the_reference_at_every_threshold(Q, C, del_overlap):
    """G23: BoxEncoder.decode_strong at thresholds 0.1 .. 0.9 (Python floats) on scores that sit on, just above and just below
    float32(threshold) - the same events in the same order, bit for bit.  (The restatement was pinned at 0.5 only.)"""
    g = np.load(os.path.join(GOLDEN, 'g23_decode_sweep.npz'))
    S, L, X = g[f'q{Q}c{C}_scores'], g[f'q{Q}c{C}_labels'], g[f'q{Q}c{C}_boxes']
    total = 0
    for i, t in enumerate(g['thresholds']):
        want = g[f'q{Q}c{C}_del{del_overlap}_t{i}']
        got = [(b, c, on, off, sc) for b in range(len(S))
               for c, on, off, sc in R.decode_strong(S[b], L[b], X[b], threshold=float(t), del_overlap=bool(del_overlap))]
        assert len(got) == len(want), (t, len(got), len(want))
        assert np.array_equal(np.array(got, dtype=np.float64).reshape(-1, 5), want.astype(np.float64)), t
        total += len(got)
    assert total > (100 if Q == 1 else 1000)


def test_fixture_scores_sit_on_the_float32_thresholds():
    """the rows the threshold's rounding to float32 decides are there: a score equal to float32(0.7) is kept at threshold 0.7 with
    del_overlap (>=, and float32(0.7) < 0.7 in float64) and dropped without (>)"""
    g = np.load(os.path.join(GOLDEN, 'g23_decode_sweep.npz'))
    S, X = g['q21c10_scores'], g['q21c10_boxes']
    i = list(g['thresholds']).index(0.7)
    assert float(np.float32(0.7)) < 0.7
    on_edge = (S == np.float32(0.7)) & ((X[..., 1] - X[..., 0]) >= np.float32(0.2))
    assert on_edge.sum() > 5
    rows1, rows0 = g[f'q21c10_del1_t{i}'], g[f'q21c10_del0_t{i}']
    assert not (rows0[:, 4] == np.float32(0.7)).any()
    assert (rows1[:, 4] == np.float32(0.7)).any()


# ---------------------------------------------------------------------------------------------------------------- unpacking
def _packed(records, K, B, Q):
    """records {(k, b): [(class, onset, offset, score, query)]} -> the buffer sedt_decode_events writes, filler included"""
    p = np.zeros((K, B, 1 + 5 * Q), dtype=np.int32)
    slots = p[:, :, 1:].reshape(K, B, Q, 5)
    slots[..., 0] = slots[..., 4] = -1
    for (k, b), ev in records.items():
        p[k, b, 0] = len(ev)
        for s, (c, on, off, sc, q) in enumerate(ev):
            slots[k, b, s, 0], slots[k, b, s, 4] = c, q
            slots[k, b, s, 1:4] = np.array([on, off, sc], dtype=np.float32).view(np.int32)
    return p


class _Fetched(object):
    def __init__(self, tags, events):
        self.tags, self.events = tags, events

    def rows(self):
        return self.tags, self.events


def test_unpack_prediction_set_tsv_and_tag_table(tmp_path):
    """K = 2, B = 3, Q = 3, one fusion strategy: clip 0 full (n = Q), clip 1 empty, clip 2 one event at the low threshold only"""
    from sound_event_detection_transformer_amd.utilities import predictions as P
    labels = ['dog', 'car', 'bell']
    K, B, Q = 2, 3, 3
    rec = {(0, 0): [(2, 0.0, 1.5, 0.9, 1), (0, 0.25, 0.75, 0.5, 0), (0, 2.0, 10.0, 0.7, 2)], (0, 2): [(1, 3.0, 3.0, 0.3, 2)],
           (1, 0): [(2, 0.0, 1.5, 0.9, 1)]}
    packed = _packed(rec, K, B, Q)
    ev = P.unpack(packed, Q)
    assert len(ev) == K and ev[0]['clip'].tolist() == [0, 0, 0, 2] and ev[0]['query'].tolist() == [1, 0, 2, 2]
    assert ev[0]['onset'].dtype == np.float32 and ev[1]['cls'].tolist() == [2] and ev[1]['clip'].tolist() == [0]
    packed[0, 0, 1] = 77                                    # the result is a copy: the buffer may be overwritten afterwards
    assert ev[0]['cls'].tolist() == [2, 0, 0, 1]
    packed[0, 0, 1] = 2
    with pytest.raises(ValueError):
        bad = packed.copy()
        bad[0, 1, 0] = Q + 1
        P.unpack(bad, Q)

    tags = np.array([[1, 0, 1], [0, 0, 0], [0, 1, 0]], dtype=np.int64)
    table, sets = P.TagTable(), {1: P.PredictionSet(labels, [0.3, 0.8])}
    P.collect(_Fetched(tags, {1: ev}), ['a.wav', 'b.wav', 'c.wav'], table, sets, labels)
    P.collect(_Fetched(None, {1: P.unpack(_packed({(1, 1): [(1, 4.0, 5.0, 0.95, 0)]}, K, 2, Q), Q)}), ['d.wav', 'e.wav'], table, sets,
              labels)                                       # a second, shorter batch without tags
    ps = sets[1]
    assert len(ps) == 2 and [t.threshold for t in ps] == [0.3, 0.8]
    f = lambda v: float(np.float32(v))
    assert ps.to_rows() == ps.at(0).to_rows() == [('bell', 0.0, 1.5, f(0.9), 'a.wav'), ('dog', 0.25, 0.75, 0.5, 'a.wav'),
                                                  ('dog', 2.0, 10.0, f(0.7), 'a.wav'), ('car', 3.0, 3.0, f(0.3), 'c.wav')]
    assert ps.to_rows(1) == [('bell', 0.0, 1.5, f(0.9), 'a.wav'), ('car', 4.0, 5.0, f(0.95), 'e.wav')]
    assert ps.at(1).score.dtype == np.float32 and len(ps.at(1)) == 2
    ps.write_tsv(tmp_path / 'p.tsv')
    assert (tmp_path / 'p.tsv').read_text() == ('event_label\tonset\toffset\tscore\tfilename\n'
                                                'bell\t0.0\t1.5\t0.9\ta.wav\n'
                                                'dog\t0.25\t0.75\t0.5\ta.wav\n'
                                                'dog\t2.0\t10.0\t0.7\ta.wav\n'
                                                'car\t3.0\t3.0\t0.3\tc.wav\n')
    ps.write_tsv(tmp_path / 'p1.tsv', k=1)
    assert (tmp_path / 'p1.tsv').read_text().splitlines()[1:] == ['bell\t0.0\t1.5\t0.9\ta.wav', 'car\t4.0\t5.0\t0.95\te.wav']
    assert table.to_rows() == [('dog', 'a.wav', 0, 0), ('bell', 'a.wav', 0, 0), ('car', 'c.wav', 0, 0)]
    assert not table.empty and P.TagTable().empty and P.TagTable().to_rows() == []
    df = ps.to_dataframe(1)
    assert list(df.columns) == ['event_label', 'onset', 'offset', 'score', 'filename'] and df['filename'].tolist() == ['a.wav', 'e.wav']
    assert [ps.at(k).to_dataframe().shape for k in range(2)] == [(4, 5), (2, 5)]          # the operating-point list of a PSDS sweep
    assert list(table.to_dataframe().columns) == ['event_label', 'filename', 'onset', 'offset']
    empty = P.PredictionSet(labels, [0.5])
    assert empty.to_rows() == [] and empty.to_dataframe().shape == (0, 5)


def test_decoder_host_side_checks():
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    d = EventDecoder(['a', 'b', 'c'], 10.0, thresholds=(0.1, 0.7), device='cpu')
    assert d.K == 2 and d.thresholds.dtype.is_floating_point and d.threshold_values.dtype == np.float32
    assert d.decode_weak(np.array([1, 0, 1])) == ['a', 'c']                       # BoxEncoder.decode_weak: tag == 1
    d.set_thresholds([0.2, 0.9])
    assert d.thresholds.tolist() == [float(np.float32(0.2)), float(np.float32(0.9))]
    with pytest.raises(ValueError):
        d.set_thresholds([0.5])                                                   # another K needs another decoder (and graph)
    with pytest.raises(ValueError):
        EventDecoder(['a'], 0.1, device='cpu')                                    # float32 does not hold 0.1 exactly
    EventDecoder(['a'], float('inf'), device='cpu')                               # no clip
    with pytest.raises(ValueError):
        EventDecoder(['a'], 10.0, thresholds=(), device='cpu')
    with pytest.raises(RuntimeError):
        d.fetch()


def test_decode_has_no_cpu_fallback():
    import torch
    from sound_event_detection_transformer_amd import ops
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ops.decode_events(torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, 2), torch.tensor([0.5]), 3)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_declares_binds_and_exports_decode_events():
    from sound_event_detection_transformer_amd import _build, lib
    assert 'decode.hip' in _build.SOURCES
    hdr = open(os.path.join(ROOT, 'include', 'sedt_hip.h')).read()
    assert re.search(r'\bint sedt_decode_events\s*\(', hdr)
    proto = re.search(r'int sedt_decode_events\s*\((.*?)\);', hdr, flags=re.S).group(1)
    assert 'sedt_decode_events' in lib.SIGNATURES and len(lib.SIGNATURES['sedt_decode_events'][1]) == len(proto.split(','))
    _build.build()
    assert hasattr(lib.load(), 'sedt_decode_events')
