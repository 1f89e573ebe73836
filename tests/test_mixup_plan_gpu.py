"""GPU: sedt_mixup_plan (csrc/mixplan.hip) through ops.mixup_plan and TargetTables.load_mixed against tests/mixup_plan_ref.py - which
tests/test_mixup_plan_cpu.py pins to the host plan - and, where the host route takes the batch, against the host plan itself.
Everything is exact: offsets, split words, labels, job records and status equal; boxes and ratios bit-equal; only live entries written.

Shapes (tests/mixup_plan_ref.py designed_cases, random_case): B = 1 with mix_num = 0; B = 2; B = 5 with ns = 3, n_lab = 4; B = 65 and
B = 130 (past one wave, past one pass of 16 waves over the mixed clips) and the envelope's end, B = 1024; B_src > B.  Events: n1 + n2 == max_events and max_events + 1;
boxes that touch exactly and that miss by one ulp; an overlap inside clip i alone; an empty partner on either side, both empty, a weak
and an unlabelled partner; 63 boxes in one candidate.  Index: index[i] == i; two clips sent to one partner.  Capacity: max_targets_out
reached exactly and exceeded by one (status 1); two launches into the same buffers.  Status 2 is reached through the host-side refusal
only (tests/test_mixup_plan_cpu.py): no out-of-range index is fed to the kernel."""
import os

import numpy as np
import pytest
import torch

import mixup_plan_ref as R

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _buffers(B, M_out):
    return (torch.full((8 * B + 16 + 20 * B * M_out,), POISON, dtype=torch.uint8, device='cuda'),
            torch.full((16 * B,), POISON, dtype=torch.uint8, device='cuda'), torch.full((B,), -1, dtype=torch.int32, device='cuda'))


def _launch(c, bufs=None):
    from sound_event_detection_transformer_amd import ops
    B, Mo = c['B'], c['M_out']
    assert c['index'].min() >= 0 and c['index'].max() < B             # never an out-of-range index on the GPU
    out, jobs, status = _buffers(B, Mo) if bufs is None else bufs
    src = torch.from_numpy(R.source_blob(c['clips'], c['M_src'])).cuda()
    index = torch.from_numpy(c['index'].astype(np.int32)).cuda()
    lam = torch.from_numpy(R.lam_pair(c['lam'])).cuda()
    ops.mixup_plan(src, len(c['clips']), c['M_src'], B, c['ns'], c['n_lab'], index, lam, c['mix_num'], c['max_events'], Mo, out, jobs, status)
    return out.cpu().numpy(), jobs.cpu().numpy(), status.cpu().numpy()


def _check(c, got, host=True, fresh=True):
    raw, jobs, status = got
    B, Mo = c['B'], c['M_out']
    ref = R.reference(c)
    tables = R.read_tables(raw, B, Mo)
    R.assert_same_tables(tables, {k: ref[k] for k in ('off', 'lab', 'box', 'ratio')})
    R.assert_same_jobs(jobs, ref['jobs'])
    assert status.tolist() == ref['status'].tolist()
    if host:                                                         # the oracle itself, where it takes the batch
        want, want_jobs = R.oracle(c, torch)
        R.assert_same_tables(tables, want)
        R.assert_same_jobs(jobs, want_jobs)
    if fresh:                                                        # only live entries are written
        cap, o_lab = B * Mo, 8 * B + 16
        nl, nb = len(ref['lab']), len(ref['box'])
        assert (raw[o_lab + 8 * nl:o_lab + 8 * cap] == POISON).all() and (raw[o_lab + 8 * cap + 8 * nb:o_lab + 16 * cap] == POISON).all()
        assert (raw[o_lab + 16 * cap + 4 * nl:] == POISON).all() and (raw[4 * (2 * B + 4):o_lab] == POISON).all()
    return ref


@pytest.mark.parametrize('name', list(R.designed_cases()))
def test_designed_cases(name):
    c = R.designed_cases()[name]
    ref = _check(c, _launch(c), host=name != 'capacity + 1')
    if name == 'capacity + 1':
        assert ref['status'].tolist() == [1, 0, 1, 0]
    if name == '63 events merge':
        assert ref['off'][:3].tolist() == [0, 63, 126] and ref['outcomes'] == [R.STRONG] * 2
    if name == '64 events do not':
        assert ref['outcomes'] == [R.KEEP1_EVENTS] * 2


@pytest.mark.parametrize('B,B_src,ns,n_lab,mix_num', [(65, 65, 40, 60, 33), (130, 130, 130, 130, 130), (130, 141, 100, 120, 100),
                                                      (1024, 1024, 700, 900, 700)])
def test_random_batches_past_one_wave_and_one_pass(B, B_src, ns, n_lab, mix_num):
    rng = np.random.default_rng(B + B_src)
    c = R.random_case(rng, B=B, B_src=B_src, ns=ns, n_lab=n_lab, mix_num=mix_num)
    ref = _check(c, _launch(c))
    seen = set(ref['outcomes'])
    assert {R.KEEP1_EMPTY, R.KEEP2, R.WEAK, R.KEEP1_EVENTS, R.KEEP1_OVERLAP, R.STRONG} <= seen, seen
    assert ref['off'][2 * B + 2] < ns                                 # weak merges moved the split


def test_two_launches_into_the_same_buffers():
    """the second batch has fewer events and another split: every offset and the split words are rewritten, nothing of the first
    launch is read"""
    rng = np.random.default_rng(5)
    first = R.random_case(rng, B=65, ns=50, n_lab=60, mix_num=50, p_empty=0.1)
    second = R.random_case(rng, B=65, ns=30, n_lab=40, mix_num=12, p_empty=0.7)
    bufs = _buffers(65, 8)
    a = _check(first, _launch(first, bufs))
    b = _check(second, _launch(second, bufs), fresh=False)
    assert len(b['lab']) < len(a['lab']) and b['off'][-2:].tolist() != a['off'][-2:].tolist()
    again = _launch(second, bufs)                                     # deterministic: the same bytes
    _check(second, again, fresh=False)


def test_g13_recorded_draw(golden_dir):
    """fixture G13's recorded mixup_data draw (the reference's own lam and shuffled index) planned on the device from a blob built out
    of its inputs, as tests/test_input_gpu.py::test_g13_mixup_matches_reference does for the host plan.  The fixture was recorded with
    mix_up_ratio 0.67 on 3 strong + 3 weak clips: mix_num = 4 > ns = 3, outside the kernel's envelope (the fourth mixed clip is a weak
    one), so the draw is planned with mix_num = 3 - the largest the envelope takes.  Clips 0, 1, 2 (mixed) and 4, 5 (unchanged) then
    are exactly the fixture's rows; row 3 (unchanged here, a weak merge with itself there) and the whole result are held against the
    host plan of the same draw."""
    from oracle.criterion_oracle import synthetic_targets
    g = np.load(os.path.join(golden_dir, 'g13_transforms_mixup.npz'))
    rows = lambda a: [r[r >= 0] for r in a]
    tg = synthetic_targets(6, 133, 10)
    clips = [(t['labels'].numpy(), t['boxes'].numpy().reshape(-1, 2)) for t in tg]
    c = R.case(clips, 3, 6, g['mix_index'], 3, 20, M_src=20, lam=float(g['mix_lam']))
    assert int(6 * 0.67) == 4 and g['mix_masks'].tolist() == [3, 3, 6]
    raw, jobs, status = got = _launch(c)
    _check(c, got)
    t = R.read_tables(raw, 6, 20)
    off = t['off']
    assert off[-2:].tolist() == [3, 6] and not status.any()
    for b in (0, 1, 2, 4, 5):
        lab = t['lab'][off[b]:off[b + 1]]
        assert lab.tolist() == rows(g['mix_labels'])[b].astype(np.int64).tolist() and len(lab) == g['mix_nlabels'][b]
        ratio, want = t['ratio'][off[b]:off[b + 1]], rows(g['mix_ratio'])[b]
        if len(want):
            assert np.array_equal(ratio.view(np.int32), want.astype(np.float32).view(np.int32))
        else:
            assert (ratio == 1.0).all()
        if b < 3:
            assert off[7 + b + 1] - off[7 + b] == g['mix_nboxes'][b]
    # (in this draw the three strong clips are all kept - partner weak, or a same-class overlap; its only merge is the fixture's row 3)
    assert [len(r) for r in rows(g['mix_ratio'])] == [0, 0, 0, 12, 0, 0]


def test_load_mixed_fills_the_tables_and_the_job_buffer():
    """TargetTables.load_mixed: one pinned-ring upload of index and lam, one launch straight into the tables' blob and the job buffer;
    a source of more clips than the tables hold (the mean-teacher batch: the unlabelled clips follow)"""
    from sound_event_detection_transformer_amd import lib
    from sound_event_detection_transformer_amd.sedt import TargetTables
    from sound_event_detection_transformer_amd.utilities.recording_clips import DeviceTargets
    c = R.designed_cases()['B5 of a source of 7']
    ref = R.reference(c)
    dev = torch.device('cuda')
    dt = DeviceTargets(torch.from_numpy(R.source_blob(c['clips'], 8)).cuda(), torch.zeros(7, dtype=torch.int32, device=dev), 7, 8,
                       [f'r{b}' for b in range(7)], 10.0, ns=3, n_lab=4)
    tab = TargetTables(5, 3, 4, dev, max_targets=8, dynamic_split=True, with_ratio=True)
    jobs = torch.zeros(16 * 5, dtype=torch.uint8, device=dev)
    slot = tab._slot
    with lib.launch_log() as log:
        for _ in range(6):                                           # more calls than the ring has slots
            tab.load_mixed(dt, c['lam'], c['index'], c['mix_num'], c['max_events'], jobs)
    assert log['mixup_plan'] == 6 and tab._slot == slot
    R.assert_same_tables(R.read_tables(tab._blob.cpu().numpy(), 5, 8), {k: ref[k] for k in ('off', 'lab', 'box', 'ratio')})
    R.assert_same_jobs(jobs.cpu().numpy(), ref['jobs'])
    assert tab.split.tolist() == [2, 4] and not tab.plan_status.any()
    status = torch.full((5,), 7, dtype=torch.int32, device=dev)
    tab.load_mixed(dt, c['lam'], c['index'], c['mix_num'], c['max_events'], jobs, status=status)
    assert not status.any()
    # the static-split prefix load of the same source on the device
    want = TargetTables(5, 3, 4, dev, max_targets=8).load(dt.to_list()[:5])
    got = TargetTables(5, 3, 4, dev, max_targets=8).load(dt)
    nl, nb = int(want.off[5]), int(want.off[9])
    assert got.off[:10].tolist() == want.off[:10].tolist() and got.lab_cat[:nl].tolist() == want.lab_cat[:nl].tolist()
    assert torch.equal(got.box_cat[:nb], want.box_cat[:nb]) and nl > 0 and nb > 0
