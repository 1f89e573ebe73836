"""CPU: the host half of training on recordings (utilities/recording_clips.py) and the NumPy reference of sedt_cut_clips
(tests/recording_clips_ref.py) on hand-worked cases.  The kernel itself: tests/test_recording_clips_gpu.py."""
import numpy as np
import pytest
import torch

import recording_clips_ref as R

LABELS = ['Speech', 'Dog', 'Cat']


def _table(events):
    from sound_event_detection_transformer_amd.utilities.recording_clips import clip_event_table
    return clip_event_table({'a.wav': events}, LABELS)


# ---------------------------------------------------------------------------------------------------- the reference, by hand
def test_reference_window_edges():
    """sr = 1000, window = 2000 samples (W = 2 s), start = 3000: t0 = 3 s, t1 = 5 s"""
    cut = lambda ev, **kw: R.clip_targets(_table(ev), 0, 3000, 2000, 1000, 8, **kw)
    lab, box, st = cut([('Dog', 1.0, 3.0)])                      # ends exactly at t0: z - a = 0
    assert len(lab) == 0 and box.shape == (0, 2) and st == 0
    lab, box, st = cut([('Dog', 5.0, 6.0)])                      # starts exactly at t1
    assert len(lab) == 0 and st == 0
    lab, box, st = cut([('Cat', 2.0, 7.5)])                      # covers the whole window
    assert lab.tolist() == [2] and box.tolist() == [[0.5, 1.0]] and box.dtype == np.float32 and lab.dtype == np.int64
    lab, box, st = cut([('Speech', 3.5, 4.0)])                   # inside: centre 0.75 s of 2 s, length 0.5 s of 2 s
    assert lab.tolist() == [0] and box.tolist() == [[0.375, 0.25]]
    lab, box, st = cut([('Speech', 2.0, 3.25)])                  # clipped at the start: 0 .. 0.25 s
    assert box.tolist() == [[0.0625, 0.125]]


def test_reference_min_event_seconds_and_capacity():
    cut = lambda ev, m=8, **kw: R.clip_targets(_table(ev), 0, 3000, 2000, 1000, m, **kw)
    ev = [('Dog', 2.0, 3.25), ('Cat', 4.875, 9.0), ('Dog', 3.5, 3.625)]          # clipped lengths 0.25, 0.125, 0.125
    assert cut(ev, min_event_seconds=0.25)[0].tolist() == [1]                    # a clipped length equal to the minimum is kept
    assert cut(ev, min_event_seconds=0.125)[0].tolist() == [1, 1, 2]             # table order: by onset
    assert cut(ev, min_event_seconds=0.1251)[0].tolist() == [1]
    lab, box, st = cut(ev, m=3)
    assert st == 0 and len(lab) == 3
    lab, box, st = cut(ev, m=2)                                                  # one more than the tables hold: raised, first two kept
    assert st == 1 and lab.tolist() == [1, 1] and box[1].tolist() == [0.28125, 0.0625]
    lab, box, st = cut([('Dog', 3.1, 3.4), ('Dog', 3.2, 3.3)])                   # overlapping events of one class: both, as annotated
    assert lab.tolist() == [1, 1] and st == 0


def test_reference_wave_and_blob():
    recs = [np.arange(10, dtype=np.float32), np.arange(100, 103, dtype=np.float32)]
    from sound_event_detection_transformer_amd.utilities.recording_clips import clip_event_table
    table = clip_event_table({'a': [('Dog', 0.0, 0.004), ('Cat', 0.002, 0.003)], 'b': []}, LABELS)
    wave, targets, status = R.cut_clips(recs, table, [0, 1, 0], [0, 0, 8], 4, 1000, 4)
    assert wave.tolist() == [[0, 1, 2, 3], [100, 101, 102, 0], [8, 9, 0, 0]]
    assert [t[0].tolist() for t in targets] == [[1, 2], [], []] and status.tolist() == [0, 0, 0]
    off, lab, box, (o_lab, o_box, total) = R.blob(targets, 4)
    assert off.tolist() == [0, 2, 2, 2, 0, 2, 2, 2, 3, 3] and lab.tolist() == [1, 2] and (o_lab, o_box, total) == (40, 136, 232)


# ---------------------------------------------------------------------------------------------------- the host half
def test_clip_event_table_order_refusals_prefix_max():
    from sound_event_detection_transformer_amd.utilities.recording_clips import clip_event_table
    ref = {'a.wav': [('Dog', 5.0, 6.0), ('Speech', 1.0, 9.0), (2, 1.0, 2.0), ('Dog', 1.0, 2.0), ('Speech', 0.5, 0.75)],
           'quiet.wav': [],
           'b.wav': [('Cat', 3.0, 3.0), ('Dog', 0.0, 4.0)]}
    t = clip_event_table(ref, LABELS)
    assert t['names'] == ['a.wav', 'quiet.wav', 'b.wav'] and t['index'] == {'a.wav': 0, 'quiet.wav': 1, 'b.wav': 2}
    assert t['off'].tolist() == [0, 5, 5, 7] and t['off'].dtype == np.int32
    assert t['on'].tolist() == [0.5, 1.0, 1.0, 1.0, 5.0, 0.0, 3.0]                     # (onset, offset, input order), all classes together
    assert t['end'].tolist() == [0.75, 2.0, 2.0, 9.0, 6.0, 4.0, 3.0]
    assert t['cls'].tolist() == [0, 2, 1, 0, 1, 1, 2] and t['cls'].dtype == np.int32  # equal (onset, offset): input order
    assert t['pmax'].tolist() == [0.75, 2.0, 2.0, 9.0, 9.0, 4.0, 4.0]                  # the running maximum restarts per recording
    assert t['on'].dtype == t['end'].dtype == t['pmax'].dtype == np.float64
    with pytest.raises(ValueError, match="class 'Bird' is not one of the 3 labels"):
        clip_event_table({'a': [('Bird', 0.0, 1.0)]}, LABELS)
    with pytest.raises(ValueError, match='is not one of the 3 labels'):
        clip_event_table({'a': [(3, 0.0, 1.0)]}, LABELS)
    with pytest.raises(ValueError, match='non-finite event time'):
        clip_event_table({'a': [('Dog', 0.0, float('inf'))]}, LABELS)
    with pytest.raises(ValueError, match='non-finite event time'):
        clip_event_table({'a': [('Dog', float('nan'), 1.0)]}, LABELS)
    with pytest.raises(ValueError, match='ends before it starts'):
        clip_event_table({'a': [('Dog', 2.0, 1.0)]}, LABELS)
    empty = clip_event_table({'a': []}, LABELS)
    assert empty['off'].tolist() == [0, 0] and empty['on'].size == 0 and empty['pmax'].size == 0


def test_draw_picks_bounds_determinism_and_short_recordings():
    from sound_event_detection_transformer_amd.utilities.recording_clips import draw_picks
    ns, window = [5000, 700, 1003, 1004], 1003
    np.random.seed(11)
    rec, start = draw_picks(ns, window, 400)
    assert rec.dtype == np.int32 and start.dtype == np.int64 and rec.shape == start.shape == (400,)
    assert rec.min() >= 0 and rec.max() < 4 and start.min() >= 0
    room = np.maximum(np.asarray(ns) - window, 0)
    assert (start <= room[rec]).all() and (start + window <= np.maximum(np.asarray(ns)[rec], window)).all()
    assert (start[rec == 1] == 0).all() and (start[rec == 2] == 0).all()
    short = draw_picks([700, 1003, 800], window, 50)               # shorter than / as long as the window: always start 0
    assert not short[1].any() and set(short[0].tolist()) == {0, 1, 2}
    assert set(start[rec == 3].tolist()) <= {0, 1}
    assert (rec == 0).sum() > 350                                  # weights follow the number of start positions: 3998 of 4002
    np.random.seed(11)
    again = draw_picks(ns, window, 400)
    assert np.array_equal(again[0], rec) and np.array_equal(again[1], start)
    # the documented order of the draws: per clip one choice, then one randint
    np.random.seed(5)
    w = (room + 1) / (room + 1).sum()
    want = []
    for _ in range(6):
        r = np.random.choice(4, p=w)
        want.append((r, np.random.randint(0, room[r] + 1)))
    np.random.seed(5)
    got = draw_picks(ns, window, 6)
    assert list(zip(got[0].tolist(), got[1].tolist())) == want


@pytest.mark.parametrize('B,M', [(1, 1), (2, 32), (5, 3), (64, 32), (65, 63), (1024, 63)])
def test_blob_layout_is_the_target_tables(B, M):
    from sound_event_detection_transformer_amd.sedt import TargetTables
    from sound_event_detection_transformer_amd.utilities.recording_clips import blob_layout
    n_off, o_lab, n_lab_e, o_box, n_box_e, o_rat, total = TargetTables(B, B, B, torch.device('cpu'), max_targets=M)._lay
    assert blob_layout(B, M) == (n_off, o_lab, o_box, o_rat) and total == o_rat and n_lab_e == n_box_e == B * M
    assert R.blob([(np.zeros(0, np.int64), np.zeros((0, 2), np.float32))] * B, M)[3] == (o_lab, o_box, total)


def test_reference_blob_is_what_target_tables_lays_out():
    """the list-of-dicts route (TargetTables.load on the host) and the reference's blob agree on every live byte, and
    TargetTables.load(DeviceTargets) copies exactly that blob"""
    from sound_event_detection_transformer_amd.sedt import TargetTables
    from sound_event_detection_transformer_amd.utilities.recording_clips import DeviceTargets, blob_layout, clip_event_table
    table = clip_event_table({'a': [('Dog', 0.25, 1.5), ('Cat', 0.5, 0.75), ('Speech', 1.5, 3.0)], 'b': []}, LABELS)
    rec, start, B, M = [0, 1, 0], [0, 0, 1000], 3, 4
    _, targets, status = R.cut_clips([np.zeros(4000, np.float32), np.zeros(3000, np.float32)], table, rec, start, 2000, 1000, M)
    assert [len(t[0]) for t in targets] == [3, 0, 2] and not status.any()
    off, lab, box, (o_lab, o_box, total) = R.blob(targets, M)
    raw = np.zeros(total, np.uint8)
    raw[:off.nbytes] = off.view(np.uint8)
    raw[o_lab:o_lab + lab.nbytes] = lab.view(np.uint8)
    raw[o_box:o_box + box.nbytes] = box.reshape(-1).view(np.uint8)
    dt = DeviceTargets(torch.from_numpy(raw), torch.zeros(B, dtype=torch.int32), B, M, ['a', 'b', 'a'], 2.0)
    lst = dt.to_list()
    assert [t['labels'].tolist() for t in lst] == [t[0].tolist() for t in targets]
    assert all(np.array_equal(t['boxes'].numpy(), w[1]) and t['boxes'].dtype == torch.float32 for t, w in zip(lst, targets))
    assert all(float(t['orig_size']) == 2.0 for t in lst)
    by_list = TargetTables(B, B, B, torch.device('cpu'), max_targets=M).load(lst)
    by_blob = TargetTables(B, B, B, torch.device('cpu'), max_targets=M).load(dt)
    assert blob_layout(B, M)[3] == total
    for tab in (by_list, by_blob):
        assert tab.off.numpy().tolist() == off.tolist()
        assert tab.lab_cat[:len(lab)].numpy().tolist() == lab.tolist() and np.array_equal(tab.box_cat[:len(box)].numpy(), box)
    # preconditions of the device route
    with pytest.raises(NotImplementedError, match='dynamic-split tables'):
        TargetTables(B, B, B, torch.device('cpu'), max_targets=M, dynamic_split=True, with_ratio=True).load(dt)
    with pytest.raises(ValueError, match='max_targets=5'):
        TargetTables(B, B, B, torch.device('cpu'), max_targets=5).load(dt)
    with pytest.raises(ValueError, match='2 strong'):
        TargetTables(B, 2, B, torch.device('cpu'), max_targets=M).load(dt)
    with_ratio = TargetTables(B, B, B, torch.device('cpu'), max_targets=M, with_ratio=True)
    with_ratio.ratio_cat.fill_(0.25)
    assert with_ratio.load(dt).ratio_cat.eq(1.0).all() and with_ratio.off.numpy().tolist() == off.tolist()
    # a raised status names the clip's recording
    bad = DeviceTargets(torch.from_numpy(raw), torch.tensor([0, 0, 1], dtype=torch.int32), B, M, ['a', 'b', 'a'], 2.0)
    with pytest.raises(RuntimeError, match="clip 2 of recording 'a': status 1 .*max_targets"):
        bad.to_list()
    with pytest.raises(RuntimeError, match="clip 2 of recording 'a'"):
        bad.check()


def test_entry_point_refuses_outside_the_envelope():
    """1 <= B <= 1024 and 1 <= max_targets <= 63, refused with a message before a pointer is touched (every pointer here is null)"""
    from sound_event_detection_transformer_amd import _build, lib
    _build.build()
    l = lib.load()
    call = lambda B, M, window=160000: l.sedt_cut_clips(None, 0, None, None, 1, None, None, B, window, 16000, None, None, None, None, None, 0,
                                                        M, 0.0, None, None, None, None)
    for B, M in ((0, 32), (1025, 32), (-1, 32), (4, 0), (4, 64)):
        assert call(B, M) != 0
        msg = l.sedt_last_error().decode()
        assert f'B={B} max_targets={M} outside the envelope' in msg and '1024' in msg and '63' in msg, msg
    assert call(4, 32, window=0) != 0 and 'window=0' in l.sedt_last_error().decode()
    assert call(1024, 63) != 0 and 'null pointer' in l.sedt_last_error().decode()          # inside the envelope: the pointers are looked at
    assert lib.CLIPS_MAXB == 1024
