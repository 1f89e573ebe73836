"""GPU: live streams.  The waveform rings (csrc/stream.hip through ops.stream_append / ops.stream_cut) bit-exact against NumPy slices
of the concatenated input; the stitch sweep one window per launch (ops.stitch_stream) against BOTH the offline kernel
(ops.stitch_events on the same records) and the NumPy restatement (tests/stream_ref.py) - equal words, counts and status - on the
hand-built cases of tests/test_recording_gpu.py replayed one window per launch; then utilities.stream.StreamDetector end to end on a
C2 model's own outputs against the offline path."""
import numpy as np
import pytest
import torch

import recording_ref as R
import stream_ref as SR

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
G = 1.0 / 64.0
S3 = 3


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda()


# ---------------------------------------------------------------------------------------------------------------- rings
RING, WINDOW = 40, 16


def _append(ring, pos, pieces):
    """pieces [(stream, samples)] appended at the streams' write positions ``pos`` (updated) in ONE launch"""
    from sound_event_detection_transformer_amd import ops
    jobs, flat, off = [], [], 0
    for s, x in pieces:
        jobs.append((s, pos[s] % RING, off, len(x)))
        flat.append(np.asarray(x, np.float32))
        off += len(x)
        pos[s] += len(x)
    h = np.asarray(jobs, np.int32).reshape(-1, 4)
    src = _dev(np.concatenate(flat) if flat else np.zeros(1, np.float32), torch.float32)
    ops.stream_append(src, h, _dev(h.reshape(-1), torch.int32) if len(h) else None, ring)


def _cut(ring, jobs, B=S3, window=WINDOW):
    from sound_event_detection_transformer_amd import ops
    wave = torch.full((B, window), float('nan')).cuda()
    wave.view(torch.int32).fill_(GUARD)                                   # a guard pattern under everything the launch must write
    h = np.asarray(jobs, np.int32).reshape(-1, 4)
    ops.stream_cut(ring, h, _dev(h.reshape(-1), torch.int32) if len(h) else None, wave)
    torch.cuda.synchronize()
    return wave.cpu().numpy()


def test_appends_at_the_wrap_point_and_cuts_across_it():
    rng = np.random.default_rng(3)
    x = [rng.standard_normal(200).astype(np.float32) for _ in range(S3)]
    ring, ref, pos = torch.zeros((S3, RING)).cuda(), SR.Rings(S3, RING), [0] * S3
    # stream 0 ends exactly at the wrap point, stream 1 one before it, stream 2 one past it; then all of them move on across it
    for sizes in ((30, 30, 30), (10, 9, 11), (1, 2, 16), (39, 40, 23), (17, 0, 1)):
        pieces = [(s, x[s][pos[s]:pos[s] + n]) for s, n in enumerate(sizes) if n]
        for s, p in pieces:
            ref.append(s, pos[s] % RING, p)
        _append(ring, pos, pieces)
        torch.cuda.synchronize()
        got = ring.cpu().numpy()
        assert np.array_equal(got, ref.buf)
        for s in range(S3):                                               # the ring holds the stream's last RING samples, in place
            for i in range(max(pos[s] - RING, 0), pos[s]):
                assert got[s, i % RING] == x[s][i]
    assert pos == [97, 81, 81]
    # cuts at the due windows of hop 6 and 16 that are still inside the ring, rows in another order than the streams
    for hop in (6, 16):
        for s in range(S3):
            starts = [w * hop for w in range(pos[s] // hop + 1) if w * hop >= pos[s] - RING and w * hop + WINDOW <= pos[s]]
            assert len(starts) >= (2 if hop == 16 else 4)
            for st in starts:
                row = (s + 1) % S3
                wave = _cut(ring, [(s, st % RING, WINDOW, row)])
                assert np.array_equal(wave[row], x[s][st:st + WINDOW]) and not wave[[r for r in range(S3) if r != row]].any()
    # and at every start the ring still holds: every alignment, every way of straddling the wrap point
    straddle = 0
    for st in range(pos[1] - RING, pos[1] - WINDOW + 1):
        wave = _cut(ring, [(s, (st + pos[s] - pos[1]) % RING, WINDOW, s) for s in range(S3)])
        for s in range(S3):
            a = st + pos[s] - pos[1]
            assert np.array_equal(wave[s], x[s][a:a + WINDOW]), (s, a)
            straddle += a % RING + WINDOW > RING
    assert straddle >= WINDOW - 1
    # all rows in one launch, one of them short: zero-padded, the guard pattern gone everywhere
    jobs = [(0, 81 % RING, 16, 2), (1, 70 % RING, 5, 0), (2, 65 % RING, 16, 1)]
    wave = _cut(ring, jobs)
    assert np.array_equal(wave, ref.cut(jobs, S3, WINDOW))
    assert np.array_equal(wave[2], x[0][81:97]) and np.array_equal(wave[0, :5], x[1][70:75]) and not wave[0, 5:].any()
    assert np.array_equal(wave[1], x[2][65:81])
    assert not _cut(ring, [(1, 3, 0, 1)]).any()                           # a job of length 0
    # an empty job list: every row zeroed, and an append of nothing leaves the rings alone
    assert not _cut(ring, []).any()
    before = ring.clone()
    _append(ring, pos, [])
    assert torch.equal(ring, before)


def test_int16_chunks_are_widened_on_the_way():
    from sound_event_detection_transformer_amd import ops
    from sound_event_detection_transformer_amd.utilities.recording import stage_recordings
    rng = np.random.default_rng(4)
    a, b = rng.integers(-32768, 32768, 23).astype(np.int16), rng.standard_normal(9).astype(np.float32)
    c = torch.from_numpy(rng.integers(-32768, 32768, 7).astype(np.int16)).cuda()          # a device chunk is taken as it is
    flat, off, ns, _keep = stage_recordings([a, b, c], torch.device('cuda'))
    ring = torch.zeros((S3, RING)).cuda()
    h = np.asarray([(s, 30, int(off[s]), ns[s]) for s in range(S3)], np.int32)
    ops.stream_append(flat, h, _dev(h.reshape(-1), torch.int32), ring)
    torch.cuda.synchronize()
    got = ring.cpu().numpy()
    want = [a.astype(np.float32) / np.float32(32768), b, c.cpu().numpy().astype(np.float32) / np.float32(32768)]
    for s in range(S3):
        assert np.array_equal(got[s, (30 + np.arange(ns[s])) % RING], want[s])


def test_ring_arguments_are_checked_on_the_host():
    from sound_event_detection_transformer_amd import ops
    ring, src, wave = torch.zeros((S3, RING)).cuda(), torch.zeros(64).cuda(), torch.zeros((S3, WINDOW)).cuda()

    def app(job, **kw):
        h = np.asarray([job], np.int32)
        ops.stream_append(kw.get('src', src), h, _dev(h.reshape(-1), torch.int32), ring)

    def cut(jobs, w=wave, r=ring):
        h = np.asarray(jobs, np.int32).reshape(-1, 4)
        ops.stream_cut(r, h, _dev(h.reshape(-1), torch.int32), w)
    for job, msg in (((3, 0, 0, 4), 'stream 3'), ((-1, 0, 0, 4), 'stream -1'), ((0, 40, 0, 4), 'write position 40'), ((0, -1, 0, 4), 'position -1'),
                     ((0, 0, 0, 41), '41 samples'), ((0, 0, 61, 4), 'outside the staged 64'), ((0, 0, -1, 4), 'outside the staged')):
        with pytest.raises(RuntimeError, match='stream_append.*' + msg):
            app(job)
    for jobs, msg in (([(3, 0, 4, 0)], 'stream 3'), ([(0, 40, 4, 0)], 'read position 40'), ([(0, 0, 17, 0)], 'length 17'), ([(0, 0, -1, 0)], 'length -1'),
                      ([(0, 0, 4, 3)], 'row 3'), ([(0, 0, 4, -1)], 'row -1'), ([(0, 0, 4, 1), (1, 0, 4, 1)], 'row 1 has a job'),
                      ([(0, 0, 4, 0)] * 4, 'n_jobs=4')):
        with pytest.raises(RuntimeError, match='stream_cut.*' + msg):
            cut(jobs)
    with pytest.raises(RuntimeError, match='stream_cut.*window=41'):
        cut([(0, 0, 4, 0)], w=torch.zeros((S3, 41)).cuda())


# ---------------------------------------------------------------------------------------------------------------- stitch_stream
class Streams(object):
    """K x S streams on the device: state, status, and one emit buffer filled with the guard pattern for the whole test"""

    def __init__(self, K, S, C, Q, gap=0.0, emit_cap=64):
        from sound_event_detection_transformer_amd import ops
        self.K, self.S, self.C, self.Q, self.gap, self.cap = K, S, C, Q, gap, emit_cap
        self.state, self.status = ops.stitch_stream_state(K, S, 'cuda')
        self.emit = torch.full((K, S, emit_cap, 10), GUARD, dtype=torch.int32).cuda()
        self.count = torch.zeros((K, S), dtype=torch.int32).cuda()

    def launch(self, records, feed):
        """records [K, B, 1 + 5 Q]; feed {stream: (action, row, t_w, dur, window index)}, every other stream is skipped"""
        from sound_event_detection_transformer_amd import ops
        action, row, win = np.zeros(self.S, np.int32), np.zeros(self.S, np.int32), np.zeros(self.S, np.int32)
        t, dur = np.zeros(self.S), np.zeros(self.S)
        for s, (a, r, tw, d, w) in feed.items():
            action[s], row[s], t[s], dur[s], win[s] = a, r, tw, d, w
        ops.stitch_stream(_dev(np.ascontiguousarray(records, np.int32), torch.int32), _dev(action, torch.int32), _dev(row, torch.int32),
                          _dev(t, torch.float64), _dev(dur, torch.float64), _dev(win, torch.int32), self.C, self.gap, self.state, self.emit,
                          self.count, self.status)

    def host(self):
        torch.cuda.synchronize()
        return self.emit.cpu().numpy(), self.count.cpu().numpy(), self.status.cpu().numpy()


def _offline(rec, t, dur, C, gap, cap=700):
    """ops.stitch_events on one recording's records [K, W, row]: (count [K, C], out [K, C, cap, 8], status [K])"""
    from sound_event_detection_transformer_amd import ops
    W = len(t)
    count, out, status = ops.stitch_events(_dev(np.ascontiguousarray(rec, np.int32), torch.int32), _dev([0, W], torch.int32),
                                           _dev(np.asarray(t, np.float64) if W else np.zeros(1), torch.float64), _dev([dur], torch.float64), C, gap, cap,
                                           n_windows=W)
    torch.cuda.synchronize()
    return count.cpu().numpy()[:, 0], out.cpu().numpy()[:, 0], status.cpu().numpy()[:, 0]


def _by_class(words, C):
    """emitted words [n, 10] -> per class the eight event words, in emission order"""
    return [words[words[:, 8] == c][:, :8] for c in range(C)]


def _replay(rec, t, dur, C, gap=0.0, emit_cap=700, check_offline=True):
    """the records [K, W, row] of ONE recording replayed one window per launch on three streams with three schedules - stream 0: a
    window every launch, then a flush; stream 1: a window every other launch (skipped in between), the last one with action 3;
    stream 2: starts a launch later, action 1 then 2 - their rows permuted.  Every stream against the offline kernel and against
    the restatement: words, counts per class, status; the emit buffer past the counts still the guard pattern."""
    rec = np.ascontiguousarray(rec, np.int32)
    K, W = rec.shape[0], rec.shape[1]
    Q = (rec.shape[2] - 1) // 5
    st = Streams(K, S3, C, Q, gap, emit_cap)
    when = [{w: w for w in range(W)}, {2 * w: w for w in range(W)}, {w + 1: w for w in range(W)}]
    flush_at = [W, None, W + 1]
    for l in range(max(2 * W, W + 2)):
        feed, batch = {}, np.zeros((K, S3, rec.shape[2]), np.int32)
        for s in range(S3):
            row = (s + 1) % S3
            if l in when[s]:
                w = when[s][l]
                batch[:, row] = rec[:, w]
                feed[s] = (SR.ADD_FLUSH if s == 1 and w == W - 1 else SR.ADD, row, t[w], dur, w)
            elif l == flush_at[s]:
                feed[s] = (SR.FLUSH, 0, 0.0, 0.0, 0)
        if feed:
            st.launch(batch, feed)
    emit, count, status = st.host()
    if check_offline:
        off_count, off_out, off_status = _offline(rec, t, dur, C, gap)
    for k in range(K):
        ref_status, ref = SR.run(rec[k], t, [dur] * W, C, gap)
        for s in range(S3):
            assert status[k, s] == ref_status, (k, s, status[k, s], ref_status)
            assert (emit[k, s, count[k, s]:] == GUARD).all()
            if ref_status:
                continue
            got = _by_class(emit[k, s, :count[k, s]], C)
            for c in range(C):
                want = SR.emit_words([e + (c,) for e in ref.get(c, [])])[:, :8]
                assert np.array_equal(got[c], want), (k, s, c)
                if check_offline:
                    assert off_status[k] == 0 and off_count[k, c] == len(got[c]) and np.array_equal(off_out[k, c, :len(got[c])], got[c]), (k, s, c)
            assert (emit[k, s, :count[k, s], 9] == 0).all() and count[k, s] == sum(len(v) for v in ref.values())
        if check_offline and ref_status:
            assert off_status[k] == ref_status
    return emit, count, status


def test_chain_and_bridge_one_window_per_launch():
    w0 = [(0, 1.0, 4.5, 0.6), (2, 6.0, 7.0, 0.5)]
    w1 = [(0, 0.5, 4.5, 0.9), (2, 4.0, 5.0, 0.6)]
    w2 = [(0, 0.25, 3.5, 0.7), (2, 2.5 - G, 4.5, 0.8, 5)]
    for K in (1, 2):
        rec = R.pack([w0, w1, w2], 8, K)
        if K == 2:
            rec[1, 0, 0] = 1                                              # the higher threshold keeps one event of window 0
            rec[1, 1, 0] = 0                                              # and nothing of window 1
        emit, count, _ = _replay(rec, [0.0, 4.0, 8.0], 20.0, 4)
        assert count[0].tolist() == [4, 4, 4] and (emit[0, :, :4, 5].max(axis=1) == 3).all()        # the chain of class 0: n_merged 3
        _replay(rec, [0.0, 4.0, 4.0 + G], 20.0, 4)


def test_equal_onsets_scores_and_the_gap_by_one_ulp():
    _replay(R.pack([[(1, 2.0, 3.0, 0.5, 4)], [(1, 1.0, 2.5, 0.5, 9)], [(1, 0.5, 1.0, 0.5, 2), (1, 0.0, 3.0, 0.5, 3)]], 8), [0.0, 1.0, 2.0], 20.0, 4)
    _replay(R.pack([[(1, 2.0, 3.0, 0.5, 4)], [(1, 1.0, 2.5, np.nextafter(np.float32(0.5), np.float32(1)), 9)]], 8), [0.0, 1.0], 20.0, 4)
    gap = 0.3
    reach = 2.0 + gap
    for on, n in ((reach, 1), (np.nextafter(reach, 9.0), 2), (np.nextafter(reach, 0.0), 1)):
        t1 = on - 0.5
        assert t1 + 0.5 == on
        _, count, _ = _replay(R.pack([[(0, 1.0, 2.0, 0.5)], [(0, 0.5, 1.5, 0.5)]], 8), [0.0, t1], 20.0, 4, gap=gap)
        assert count[0].tolist() == [n] * 3


def test_bad_counts_classes_zero_length_and_clipped_events():
    C = 3
    rec = R.pack([[(0, 1.0, 2.0, 0.9)], [(0, 0.5, 1.0, 0.9)], [(0, 0.0, 1.0, 0.9)],
                  [(C, 0.0, 1.0, 0.9), (-1, 0.0, 1.0, 0.9), (2, 0.0, 1.0, 0.9), (2 ** 30, 0.0, 1.0, 0.9), (-2 ** 31, 0.0, 1.0, 0.9)]], 8)
    rec[0, 1, 0] = -1
    rec[0, 2, 0] = 8 + 1
    _, count, _ = _replay(rec, [0.0, 1.0, 2.0, 8.0], 20.0, C)
    assert count[0].tolist() == [2] * 3
    nan = R.pack([[(0, 1.0, 2.0, float('nan')), (0, 1.5, 2.5, 0.4), (1, float('nan'), 2.0, 0.9), (1, 1.0, float('nan'), 0.9)]], 8)
    _replay(nan, [0.0], 20.0, 2)
    w = [(0, 3.0, 3.0, 0.9), (0, 5.0, 4.0, 0.9), (1, 8.0, 10.0, 0.5), (2, 9.5, 10.0, 0.5), (3, 9.25, 9.75, 0.5), (3, 9.0, 9.25 + G, 0.6)]
    _, count, _ = _replay(R.pack([w], 8), [0.0], 9.25, 4)
    assert count[0].tolist() == [2] * 3
    _replay(R.pack([[(0, 1.0, 2.0, 0.5)], [(0, 1.0, 2.0, 0.5)]], 8), [0.0, 9.5], 9.25, 4)       # a window past the end adds nothing
    _replay(R.pack([[]], 8), [0.0], 5.0, 4)                                                      # an empty stream


def test_envelope_q64_c63():
    rng = np.random.default_rng(64)
    wins = [[(int(rng.integers(0, 63)) if s else 62, float(rng.integers(0, 640)) * G, 0.0, float(rng.integers(1, 9)) / 8) for s in range(64)]
            for _ in range(4)]
    wins = [[(c, on, on + float(rng.integers(1, 40)) * G, sc) for c, on, _, sc in w] for w in wins]
    _, count, status = _replay(R.pack(wins, 64), [0.0, 5.0, 10.0, 12.5], 22.5, 63, gap=G)
    assert not status.any() and (count > 100).all()


def test_working_set_at_576_640_and_704_entries():
    wins = [[(0, 0.1 + 0.15 * s + 0.011 * w, 0.105 + 0.15 * s + 0.011 * w, 0.5 + s / 256) for s in range(64)] for w in range(11)]
    t = np.arange(11) * 1e-3
    for W, want in ((9, 0), (10, 0), (11, R.OVERFLOW)):
        _, count, status = _replay(R.pack(wins[:W], 64), t[:W], 20.0, 1)
        assert (status == want).all() and (count == (0 if want else 64 * W)).all()


def test_emit_cap_reached_and_passed():
    evs = [(1, 1.0 * i, 1.0 * i + 0.5, 0.5) for i in range(5)]
    rec = R.pack([evs], 8)
    for cap in (5, 4):
        st = Streams(1, S3, 2, 8, emit_cap=cap)
        st.launch(np.repeat(rec, S3, axis=1), {0: (SR.ADD_FLUSH, 0, 0.0, 20.0, 0)})
        emit, count, status = st.host()
        assert count.tolist() == [[5, 0, 0]] and not status.any()       # it keeps counting past the cap ...
        assert emit[0, 0, :cap, 0:4].view(np.float64)[:, 0].tolist() == [1.0 * i for i in range(cap)]
        assert (emit[0, 1:] == GUARD).all()                               # ... and the slots behind it, the next stream's, are not touched
        # a second launch appends at the count
        st.launch(np.repeat(rec, S3, axis=1), {1: (SR.ADD, 1, 0.0, 20.0, 0)})
        st.launch(np.repeat(rec, S3, axis=1), {1: (SR.FLUSH, 0, 0.0, 0.0, 0), 0: (SR.ADD_FLUSH, 2, 30.0, 40.0, 1)})
        emit, count, _ = st.host()
        assert count.tolist() == [[10, 5, 0]] and (emit[0, 2] == GUARD).all() and (emit[0, 1, :cap, 8] == 1).all()


def test_every_status_word_is_raised_and_sticky():
    Q, C = 4, 2
    ok, early = R.pack([[(0, 1.0, 2.0, 0.5)]], Q)[0, 0], R.pack([[(0, -1.0, 2.0, 0.5)]], Q)[0, 0]
    cases = ((SR.UNORDERED, [(ok, 5.0, 0), (ok, 4.0, 0)]), (SR.UNORDERED, [(ok, float('nan'), 0)]), (SR.EARLY, [(early, 0.0, 0)]),
             (SR.ROW, [(ok, 0.0, S3)]), (SR.ROW, [(ok, 0.0, -1)]))
    for want, feeds in cases:
        st = Streams(1, S3, C, Q)
        batch = np.zeros((1, S3, 1 + 5 * Q), np.int32)
        for w, (rec, t, row) in enumerate(feeds):
            batch[0, 0] = rec
            batch[0, 1] = ok
            st.launch(batch, {0: (SR.ADD, row, t, 20.0, w), 2: (SR.ADD, 1, float(w), 20.0, w)})
        assert st.host()[2].tolist() == [[want, 0, 0]]
        batch[0, 0] = ok
        st.launch(batch, {0: (SR.ADD, 0, 50.0, 60.0, 5), 2: (SR.ADD, 1, 50.0, 60.0, 5)})
        st.launch(batch, {0: (SR.FLUSH, 0, 0.0, 0.0, 0), 2: (SR.FLUSH, 0, 0.0, 0.0, 0)})
        emit, count, status = st.host()
        assert status.tolist() == [[want, 0, 0]] and count[0, 0] == 0 and (emit[0, 0] == GUARD).all()      # sticky: nothing more
        assert count[0, 2] == 2                                           # the stream beside it is not touched by that
        # an equal start is ascending, and the first window of a stream may start anywhere
    st = Streams(1, S3, C, Q)
    batch = np.zeros((1, S3, 1 + 5 * Q), np.int32)
    batch[0, 0] = ok
    for w in range(2):
        st.launch(batch, {1: (SR.ADD, 0, 7.0, 20.0, w)})
    st.launch(batch, {1: (SR.FLUSH, 0, 0.0, 0.0, 0)})
    emit, count, status = st.host()
    assert not status.any() and count.tolist() == [[0, 1, 0]] and emit[0, 1, 0, 5] == 2


def test_reset_then_reuse_and_identical_bytes():
    from sound_event_detection_transformer_amd import ops
    rng = np.random.default_rng(9)
    wins = [[(int(rng.integers(0, 4)), float(rng.integers(0, 192)) * G, 0.0, float(rng.integers(1, 5)) / 4) for _ in range(8)] for _ in range(6)]
    wins = [[(c, on, on + float(rng.choice([1, 8, 32, 64, 96])) * G, sc) for c, on, _, sc in w] for w in wins]
    rec, t = R.pack(wins, 8, 2), np.arange(6) * 1.0
    rec[1, :, 0] = 5

    def run(st, streams, first=0, last=6, flush=True):
        for w in range(first, last):
            st.launch(np.repeat(rec[:, w:w + 1], S3, axis=1), {s: (SR.ADD, s, t[w], 30.0, w) for s in streams})
        if flush:
            st.launch(np.repeat(rec[:, :1], S3, axis=1), {s: (SR.FLUSH, 0, 0.0, 0.0, 0) for s in streams})

    a, b = Streams(2, S3, 4, 8), Streams(2, S3, 4, 8)
    run(a, (0, 1, 2)), run(b, (0, 1, 2))
    ha, hb = a.host(), b.host()
    assert all(np.array_equal(x, y) for x, y in zip(ha, hb)) and torch.equal(a.state, b.state)        # identical sequences, identical bytes
    assert ha[1].min() > 0 and (ha[0][:, :, :, 5] > 1).any() and not ha[2].any()
    # stream 0 stops half way and is reset while stream 1 goes on: stream 0 then replays from time 0 and gives what `a` gave,
    # stream 1 is not disturbed by its neighbour's reset
    c = Streams(2, S3, 4, 8)
    run(c, (0, 1), 0, 3, flush=False)
    ops.stream_reset(c.state, c.status, _dev([1, 0, 0], torch.int32))
    c.count[:, 0] = 0
    run(c, (1,), 3, 6, flush=False)
    run(c, (0,))
    c.launch(np.repeat(rec[:, :1], S3, axis=1), {1: (SR.FLUSH, 0, 0.0, 0.0, 0)})
    hc = c.host()
    for s in (0, 1):
        assert np.array_equal(hc[1][:, s], ha[1][:, s])
        for k in range(2):
            assert np.array_equal(hc[0][k, s, :hc[1][k, s]], ha[0][k, s, :ha[1][k, s]])
    # a raised status is cleared by the reset as well
    c.launch(np.repeat(rec[:, :1], S3, axis=1), {2: (SR.ADD, 7, 0.0, 1.0, 0)})
    assert c.host()[2][:, 2].tolist() == [SR.ROW] * 2
    ops.stream_reset(c.state, c.status)
    assert not c.host()[2].any() and not c.state.view(-1, c.state.numel() // 6)[:, :72].any()


def test_stitch_stream_arguments_are_checked_on_the_host():
    from sound_event_detection_transformer_amd import ops
    st = Streams(1, S3, 3, 4, emit_cap=4)
    rec = np.zeros((1, S3, 1 + 5 * 4), np.int32)
    for attr, value, msg in (('C', 64, 'C=64'), ('C', 0, 'C=0'), ('gap', -0.1, 'merge_gap'), ('gap', float('nan'), 'merge_gap'),
                             ('gap', float('inf'), 'merge_gap')):
        old = getattr(st, attr)
        setattr(st, attr, value)
        with pytest.raises(RuntimeError, match='stitch_stream.*' + msg):
            st.launch(rec, {0: (SR.ADD, 0, 0.0, 1.0, 0)})
        setattr(st, attr, old)
    with pytest.raises(RuntimeError, match='Q=65'):
        st.launch(np.zeros((1, S3, 1 + 5 * 65), np.int32), {})
    st.emit = st.emit[:, :, :0].contiguous()
    with pytest.raises(RuntimeError, match='emit_cap=0'):
        st.launch(rec, {})
    st = Streams(1, S3, 3, 4, emit_cap=4)
    st.state = st.state[:-2].clone()
    with pytest.raises(RuntimeError, match='a state of .* bytes'):
        st.launch(rec, {})
    with pytest.raises(RuntimeError, match='stream_reset.*a state of'):
        ops.stream_reset(st.state, st.status)


# ---------------------------------------------------------------------------------------------------------------- end to end
WIN, HOP, SRATE = 160000, 80000, 16000
C2_CLASSES = 10
CHUNKS = (50000, 123457, 1, 200001, 0, 31)


@pytest.fixture(scope='module')
def c2():
    """the C2 f32 model of test_recording_gpu, the seeded-noise recording of 5 windows with a pulled-back last one, and a decoder whose
    thresholds are quantiles of the model's own scores (a fresh seeded model scores low)"""
    from test_recording_gpu import _c2_model
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import detect_step
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    model, _, post = _c2_model()
    try:
        fusion = (1, 2)
        labels = [f'c{i}' for i in range(C2_CLASSES)]
        mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
        n = WIN + 3 * HOP + 32000
        wave = (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(77))).numpy()
        starts = R.window_plan(n, WIN, HOP, mel.min_samples)
        assert len(starts) == 5 and starts[4] - starts[3] < HOP
        amp, nframes = mel([wave[s:s + WIN] for s in starts[:4]])
        scores = detect_step(model, post, transform(amp, nframes=nframes), torch.full((4,), 10.0).cuda(), fusion)[1][1][0].cpu().numpy()
        grid = [float(np.quantile(scores, q)) for q in (0.5, 0.7, 0.9)]
        yield dict(model=model, post=post, mel=mel, transform=transform, wave=wave, labels=labels, fusion=fusion,
                   decoder=lambda: EventDecoder(labels, 10.0, thresholds=grid, fusion_strategy=fusion))
    finally:
        runtime.set_compute_dtype('bf16')


def _push_all(det, waves, collect):
    """the waves pushed in irregular chunks (another rhythm per stream), then finish: every StreamEvents appended to ``collect``"""
    pos, i = [0] * len(waves), 0
    while any(p < len(w) for p, w in zip(pos, waves)):
        sizes = [min(CHUNKS[(i + 2 * s) % len(CHUNKS)], len(w) - pos[s]) for s, w in enumerate(waves)]
        chunks = [w[pos[s]:pos[s] + n] for s, (w, n) in enumerate(zip(waves, sizes))]
        if i % 3 == 1:
            chunks[0] = (torch.from_numpy(chunks[0]).cuda())              # a device chunk now and then
        collect.append(det.push(chunks).result())
        pos = [p + n for p, n in zip(pos, sizes)]
        i += 1
    collect.append(det.finish().result())


def _rows(collected, m, k, with_merged=True):
    """the rows of all pushes of one (fusion strategy, threshold), sorted as one table: stream, onset, class"""
    t = [e[m].at(k) for e in collected]
    cat = {c: np.concatenate([x[c] for x in t]) for c in ('event_label', 'onset', 'offset', 'score', 'filename', 'n_merged', 'stream', 'cls')}
    order = np.lexsort((cat['cls'], cat['onset'], cat['stream']))
    rows = list(zip(*[cat[c][order].tolist() for c in ('event_label', 'onset', 'offset', 'score', 'filename')]))
    return rows, cat['n_merged'][order].tolist()


def test_three_streams_end_to_end_and_again_after_finish(c2):
    from sound_event_detection_transformer_amd import ops
    from sound_event_detection_transformer_amd.utilities.stream import StreamDetector
    wave, fusion, C = c2['wave'], c2['fusion'], C2_CLASSES
    waves = [wave, wave[:100000], wave[40000:40000 + WIN + HOP]]         # 5 windows, one short window, 2 regular windows and no closing one
    names = ['long', 'short', 'exact']
    det = StreamDetector(c2['model'], c2['post'], c2['decoder'](), c2['mel'], c2['transform'], 10.0, 5.0, n_streams=3, names=names, merge_gap=0.25)
    det.keep_records = True
    first = []
    _push_all(det, waves, first)
    assert det.received.tolist() == [0, 0, 0] and det.done.tolist() == [0, 0, 0]
    # every stream's windows, as the detector fed them: their records, starts and durations
    per = {s: [] for s in range(3)}
    for recs, rows in det.kept:
        for s, (action, t, dur, w) in rows.items():
            if action & 1:
                assert w == len(per[s])
                per[s].append(({m: recs[m][:, s].cpu().numpy() for m in fusion}, t, dur))
    want_starts = [R.window_plan(len(w), WIN, HOP, c2['mel'].min_samples) for w in waves]
    assert [[round(t * SRATE) for _, t, _ in per[s]] for s in range(3)] == want_starts
    n_merged = n_events = 0
    for m in fusion:
        for s in range(3):
            rec = np.stack([r[m] for r, _, _ in per[s]], axis=1)          # [K, W, row]
            t, durs = [x[1] for x in per[s]], [x[2] for x in per[s]]
            total = len(waves[s]) / SRATE
            regular = max(len(waves[s]) - WIN, -HOP) // HOP + 1           # the condition of the duration policy, on the regular windows
            assert durs[-1] == total and all(t_w + 10.0 <= d for t_w, d in zip(t[:regular], durs[:regular]))
            off_count, off_out, off_status = _offline(rec, t, total, C, 0.25, cap=64)
            assert not off_status.any()
            for k in range(3):
                status, ref = SR.run(rec[k], t, durs, C, 0.25, SR.ADD_FLUSH if len(waves[s]) != WIN + HOP else SR.FLUSH)
                assert status == 0
                tab = [e[m].at(k) for e in first]
                mine = {c: np.concatenate([x[c][x['stream'] == s] for x in tab]) for c in ('onset', 'offset', 'score', 'n_merged', 'window', 'query', 'cls')}
                for c in range(C):
                    sel = mine['cls'] == c
                    got = list(zip(*[mine[f][sel].tolist() for f in ('onset', 'offset', 'score', 'n_merged', 'window', 'query')]))
                    want = [(on, off, float(sc), n, w, q) for on, off, sc, n, w, q in ref.get(c, [])]
                    assert got == want, (m, s, k, c)                      # the restatement, in emission order within the class
                    times, score, nm, win, q = ops.stitch_events_views(off_out[k, c, :off_count[k, c]])
                    assert got == list(zip(times[:, 0].tolist(), times[:, 1].tolist(), score.tolist(), nm.tolist(), win.tolist(), q.tolist()))
                    n_merged += sum(g[3] > 1 for g in got)
                    n_events += len(got)
    assert n_merged > 0 and n_events > 20
    tags = [e[1] for e in first if e[1].tags is not None and len(e[1].tags)]
    assert sum(len(t.tags) for t in tags) == 5 + 1 + 2 and all(t.tags.shape[1] == C for t in tags)
    # (c) finish() has reset rings and state: the same pushes again give the same rows
    det.keep_records, det.kept = False, []
    second = []
    _push_all(det, waves, second)
    for m in fusion:
        for k in range(3):
            assert _rows(first, m, k) == _rows(second, m, k)
    assert {r[4] for r in _rows(first, 1, 0)[0]} <= set(names)


def test_one_stream_is_the_recording_detector(c2):
    """one live stream against the offline path on the whole recording: identical rows and n_merged at every threshold.  The detect
    step does not admit B = 1 (its audio tags lose the batch axis), so both paths run at B = 2 with the other row zero: the stream
    detector pads its single stream with a zero row itself, the recording detector gets every window of the plan beside a window of zeros."""
    from sound_event_detection_transformer_amd.engine import detect_stream
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector, RecordingPredictions
    from sound_event_detection_transformer_amd.utilities.stream import StreamDetector
    wave, fusion, labels = c2['wave'], c2['fusion'], c2['labels']
    make = lambda: (c2['model'], c2['post'], c2['decoder'](), c2['mel'], c2['transform'], 10.0, 5.0)      # a decoder of its own each
    args = make()
    off = RecordingDetector(*args, batch_windows=2, merge_gap=0.25)
    plan = off.plan([len(wave)])
    assert plan[1].tolist() == R.window_plan(len(wave), WIN, HOP, c2['mel'].min_samples)
    rows_of = {m: [] for m in fusion}
    for start in plan[1].tolist():
        rec, _, _ = off.records([wave[start:start + WIN], np.zeros(WIN, np.float32)])
        for m in fusion:
            rows_of[m].append(rec[m][:, 0].clone())
    res, cap = off.stitch({m: torch.stack(rows_of[m], dim=1).contiguous() for m in fusion}, plan)
    torch.cuda.synchronize()
    dec = args[2]
    offline = {m: RecordingPredictions(labels, dec.threshold_values, ['mic'], *(t.cpu().numpy() for t in res[m]), cap) for m in fusion}
    det = StreamDetector(*make(), n_streams=1, names=['mic'], merge_gap=0.25)
    assert det.B == 2 and det._rd.wave.shape[0] == 2
    pieces = [[wave[a:a + 70001]] for a in range(0, len(wave), 70001)]
    got = list(detect_stream(det, iter(pieces)))
    assert len(got) == len(pieces) + 1
    total = 0
    for m in fusion:
        for k in range(3):
            rows, merged = _rows(got, m, k)
            assert rows == offline[m].to_rows(k) and merged == offline[m].at(k)['n_merged'].tolist(), (m, k)
            total += len(rows)
    assert total > 10
