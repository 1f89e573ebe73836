"""CPU: live streams, the host half.  stream_plan / stream_finish against window_plan around every edge of the plan; the NumPy
restatement of the one-window step with carried state (tests/stream_ref.py) against the offline restatement
(tests/recording_ref.py) on seeded random record buffers; every status word; the refusals at construction."""
import types

import numpy as np
import pytest

import recording_ref as R
import stream_ref as SR

G = 1.0 / 64.0
WIN, MIN = 16, 3


def _chunkings(n):
    yield [1] * n                                                       # 1-sample chunks
    yield [7] * (n // 7) + ([n % 7] if n % 7 else [])                   # prime-sized
    yield [n]                                                           # one chunk, larger than a window from n = window + 1 on
    yield [WIN + 5] * (n // (WIN + 5)) + ([n % (WIN + 5)] if n % (WIN + 5) else [])


@pytest.mark.parametrize('hop', [6, 16])
def test_stream_plan_and_finish_are_window_plan(hop):
    from sound_event_detection_transformer_amd.utilities.recording import window_plan
    from sound_event_detection_transformer_amd.utilities.stream import stream_finish, stream_plan
    edges = [MIN - 1, MIN, WIN - 1, WIN, WIN + 1, WIN + hop - 1, WIN + hop, WIN + hop + 1, WIN + 5 * hop, WIN + 5 * hop + 1]
    for n in edges:
        for chunks in _chunkings(n):
            assert sum(chunks) == n
            got, received = [], 0
            for c in chunks:
                got += stream_plan(received, received + c, WIN, hop).tolist()
                received += c
            if n < MIN:
                with pytest.raises(ValueError, match='shorter than'):
                    stream_finish(n, WIN, hop, MIN)
                with pytest.raises(ValueError, match='shorter than'):
                    window_plan(n, WIN, hop, MIN)
                continue
            last = stream_finish(n, WIN, hop, MIN)
            if last is not None:
                assert last[1] == min(n, WIN)
                got.append(last[0])
            assert got == window_plan(n, WIN, hop, MIN).tolist() == R.window_plan(n, WIN, hop, MIN), (n, chunks[:3], got)
    assert stream_finish(0, WIN, hop, MIN) is None and stream_plan(0, 0, WIN, hop).tolist() == []
    assert stream_finish(WIN - 1, WIN, hop, MIN) == (0, WIN - 1) and stream_finish(WIN, WIN, hop, MIN) is None
    assert stream_finish(WIN + 1, WIN, hop, MIN) == (1, WIN)
    with pytest.raises(ValueError, match='hop'):
        stream_plan(0, 5, WIN, WIN + 1)


def _random_stream(rng):
    """one stream's record buffer on the 1/64 s grid: windows 0 .. 2 s apart, events up to 1.5 s long"""
    W, Q, C = int(rng.integers(1, 10)), int(rng.integers(1, 9)), int(rng.integers(1, 5))
    t = np.cumsum(np.concatenate([[0], rng.integers(0, 5, W - 1) * 32])) * G
    dur = float(t[-1] + rng.integers(1, 5 * 64) * G)
    rec = np.zeros((W, 1 + 5 * Q), np.int32)
    slots = rec[:, 1:].reshape(W, Q, 5)
    rec[:, 0] = rng.integers(0, Q + 1, W)
    odd = rng.random(W) < 0.03
    rec[:, 0][odd] = rng.choice([-1, Q + 1], int(odd.sum()))
    cls = rng.integers(0, C, (W, Q))
    bad = rng.random((W, Q)) < 0.03
    cls[bad] = rng.choice([-1, C], int(bad.sum()))
    on = rng.integers(0, 3 * 64, (W, Q)) * G
    length = rng.choice([0, 1, 2, 8, 16, 32, 64, 96], (W, Q)) * G
    slots[..., 0] = cls
    slots[..., 1] = on.astype(np.float32).view(np.int32)
    slots[..., 2] = (on + length).astype(np.float32).view(np.int32)
    slots[..., 3] = (rng.integers(1, 5, (W, Q)) / 4).astype(np.float32).view(np.int32)
    slots[..., 4] = rng.integers(0, Q, (W, Q))
    return rec, t, dur, C, float(rng.choice([0.0, 0.0, G, 4 * G]))


def test_carried_state_equals_the_offline_sweep():
    rng = np.random.default_rng(4711)
    cases, merged = 200, 0
    for _ in range(cases):
        rec, t, dur, C, gap = _random_stream(rng)
        count, status, ev = R.stitch(rec[None], [0, len(t)], t, [dur], C, gap)
        assert status[0, 0] == 0
        want = {c: ev[(0, 0, c)] for c in range(C) if (0, 0, c) in ev}
        for last in (SR.FLUSH, SR.ADD_FLUSH):
            st, got = SR.run(rec, t, [dur] * len(t), C, gap, last)
            assert st == 0 and got == want, (last, got, want)
            assert [len(got.get(c, [])) for c in range(C)] == count[0, 0].tolist()
        merged += any(e[3] > 1 for lst in want.values() for e in lst)
    assert 2 * merged > cases, (merged, cases)                          # more than half of the cases merge


def test_events_leave_once_and_in_class_onset_order():
    """an event leaves at the first window that starts past its offset + merge_gap, each launch's events are in (class, onset) order"""
    Q, C = 4, 3
    rec = R.pack([[(2, 1.0, 2.0, 0.5), (0, 3.0, 4.0, 0.6), (0, 0.5, 1.0, 0.7)], [(0, 0.0, 1.0, 0.9)], []], Q)[0]
    st = SR.Stream(C)
    assert SR.step(st, SR.ADD, rec[0], 0.0, 20.0, 0, Q, C, 0.0) == []
    got = SR.step(st, SR.ADD, rec[1], 3.5, 20.0, 1, Q, C, 0.0)           # 0.5 .. 1 and 1 .. 2 are final; 3 .. 4 merges with 3.5 .. 4.5
    assert got == [(0.5, 1.0, np.float32(0.7), 1, 0, 2, 0), (1.0, 2.0, np.float32(0.5), 1, 0, 0, 2)]
    assert SR.step(st, SR.SKIP, None, 0.0, 0.0, 0, Q, C, 0.0) == []
    assert SR.step(st, SR.ADD, rec[2], 4.5, 20.0, 2, Q, C, 0.0) == []    # off + gap == t_w: still open
    assert SR.step(st, SR.FLUSH, None, 0.0, 0.0, 0, Q, C, 0.0) == [(3.0, 4.5, np.float32(0.9), 2, 1, 0, 0)]
    assert st.count == [2, 0, 1] and st.open == [] and st.seen == 3


def test_every_status_word_and_its_stickiness():
    Q, C = 4, 2
    ok = R.pack([[(0, 1.0, 2.0, 0.5)]], Q)[0, 0]
    early = R.pack([[(0, -1.0, 2.0, 0.5)]], Q)[0, 0]
    for want, feed in ((SR.UNORDERED, [(ok, 5.0, True), (ok, 4.0, True)]), (SR.UNORDERED, [(ok, float('nan'), True)]),
                       (SR.EARLY, [(early, 0.0, True)]), (SR.ROW, [(ok, 0.0, False)])):
        st = SR.Stream(C)
        for rec, t, row_ok in feed:
            out = SR.step(st, SR.ADD, rec, t, 20.0, 0, Q, C, 0.0, row_ok)
        assert st.status == want and out == []
        assert SR.step(st, SR.ADD, ok, 9.0, 20.0, 1, Q, C, 0.0) == [] and SR.step(st, SR.FLUSH, None, 0, 0, 0, Q, C, 0.0) == []
        assert st.status == want                                          # sticky: nothing more is emitted
    # overflow: ten windows of 64 disjoint events all still open fill the set to its last entry, an eleventh overflows it
    wins = [[(0, 0.1 + 0.15 * s + 0.011 * w, 0.105 + 0.15 * s + 0.011 * w, 0.5 + s / 256) for s in range(64)] for w in range(11)]
    rec = R.pack(wins, 64)[0]
    st = SR.Stream(1)
    for w in range(11):
        assert SR.step(st, SR.ADD, rec[w], w * 1e-3, 20.0, w, 64, 1, 0.0) == []
        assert st.status == (SR.OVERFLOW if w == 10 else 0) and (len(st.open) == 64 * (w + 1) or w == 10)
    assert R.stitch(rec[None], [0, 11], np.arange(11) * 1e-3, [20.0], 1, 0.0)[1].tolist() == [[R.OVERFLOW]]
    # the first window of a stream may start anywhere, an equal start is ascending
    st = SR.Stream(C)
    SR.step(st, SR.ADD, ok, 7.0, 20.0, 0, Q, C, 0.0), SR.step(st, SR.ADD, ok, 7.0, 20.0, 1, Q, C, 0.0)
    assert st.status == 0 and st.open[0]['n'] == 2


def _fakes(K=3):
    decoder = types.SimpleNamespace(max_len=10.0, K=K, fusion=(1,), C=10, device='cpu')
    transform = types.SimpleNamespace(time_mask=False, freq_mask=False, freq_shift=False)
    mel = types.SimpleNamespace(sr=16000, hop=160, F=64, min_samples=513)
    return decoder, mel, transform


def test_depth_is_refused_at_construction():
    from sound_event_detection_transformer_amd.utilities.stream import StreamDetector, check_stream_depth
    decoder, mel, transform = _fakes()
    # 10 s / 1.25 s: eight earlier windows reach a regular window and a closing one a sample later; with merge_gap 0.01 the closing
    # window is reached by nine
    assert check_stream_depth(160000, 20000, 16000, 10.0, 0.0) == 8
    with pytest.raises(ValueError, match='StreamDetector: 9 earlier windows'):
        check_stream_depth(160000, 20000, 16000, 10.0, 0.01)
    with pytest.raises(ValueError, match='StreamDetector: 9 earlier windows'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 1.25, n_streams=2, merge_gap=0.01)
    with pytest.raises(ValueError, match='earlier windows'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 1.0, n_streams=2)
    # the recording detector's own checks
    with pytest.raises(ValueError, match='max_len_seconds'):
        StreamDetector(None, None, decoder, mel, transform, 5.0, 5.0, n_streams=2)
    with pytest.raises(ValueError, match='hop_seconds'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 11.0, n_streams=2)
    with pytest.raises(ValueError, match='merge_gap'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 5.0, n_streams=2, merge_gap=-1.0)
    with pytest.raises(ValueError, match='n_streams'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 5.0, n_streams=0)
    with pytest.raises(ValueError, match='distinct names'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 5.0, n_streams=2, names=['a', 'a'])


def test_state_size_is_refused_with_its_size():
    from sound_event_detection_transformer_amd import _build, ops
    from sound_event_detection_transformer_amd.utilities.stream import MAX_STATE_BYTES, StreamDetector, check_state_bytes
    _build.build()
    one = ops.stitch_stream_state_bytes(1, 1)
    assert one == 4 * (72 + 12 * ops.STREAM_OPEN) and ops.stitch_stream_state_bytes(3, 5) == 15 * one
    assert check_state_bytes(50, 64) == 50 * 64 * one <= MAX_STATE_BYTES
    with pytest.raises(ValueError, match=f'1024 thresholds x 64 streams takes {1024 * 64 * one} bytes'):
        check_state_bytes(1024, 64)
    decoder, mel, transform = _fakes(K=1024)
    with pytest.raises(ValueError, match=f'{1024 * 64 * one} bytes'):
        StreamDetector(None, None, decoder, mel, transform, 10.0, 5.0, n_streams=64)
