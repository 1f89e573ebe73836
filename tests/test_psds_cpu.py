"""CPU: the host finish of the device PSDS (utilities/psds.py: psds_from_counts) on a hand-worked case and against the from-scratch
restatement (tests/psds_ref.py), the restatement's own counts on the rows behind that case, and the refusals."""
import numpy as np
import pytest

import psds_ref as R
from sound_event_detection_transformer_amd.utilities.psds import psds_from_counts

# two classes a, b; two 10 s clips (T = 20); clip 0: a [1, 3] and b [5, 9], clip 1: a [2, 4]: n = (2, 1), T_c = (4, 4)
LABELS = ['a', 'b']
REFERENCE = [[('a', 1.0, 3.0), ('b', 5.0, 9.0)], [('a', 2.0, 4.0)]]
DURATIONS = [10.0, 10.0]
# operating point 0: one detection on clip 0's a; operating point 1: b [5, 7] covers exactly half of b [5, 9] (GTC 0.5) and a [0, 4]
# lies exactly half inside a [2, 4] (DTC 0.5): both must pass; a [6, 8] misses every a, lies inside b [5, 9] and inside the clip
ROWS = [[(0, 0, 1.0, 3.0)],
        [(0, 0, 1.0, 3.0), (0, 1, 5.0, 7.0), (0, 0, 6.0, 8.0), (1, 0, 0.0, 4.0)]]
COUNTS = [[[1, 0, 0], [0, 0, 0]],
          [[2, 1, 1], [0, 1, 0]]]                           # [k][c][a, b, world]


@pytest.mark.parametrize('setting,want', [((0, 0, 100), 0.75), ((1, 0, 100), 0.75), ((0, 1, 100), 0.5), ((0, 0, 200), 0.775),
                                          ((1, 0, 200), 0.75)])
def test_hand_worked_case(setting, want):
    """point 0: tpr (0.5, 0) at efpr 0; point 1: tpr (1, 1), fpr_a = 1 / 20 * 3600 = 180 /h, ctr[a][b] = 1 / 4 * 3600 = 900 /h.  Class b
    reaches 1 at x = 0; class a holds 0.5 up to x = 180 (1080 with alpha_ct = 1): mean 0.75, std 0.25 on [0, 100]; up to 200 the last
    20 /h are at 1: (0.75 * 180 + 20) / 200 = 0.775"""
    got = psds_from_counts(np.array(COUNTS), [2, 1], [4.0, 4.0], 20.0, *setting)
    assert abs(got - want) <= 1e-12, (setting, got, want)
    assert abs(R.score(COUNTS, [2, 1], [4.0, 4.0], 20.0, *setting) - want) <= 1e-12


def test_restated_counts_of_the_hand_worked_rows():
    assert R.counts(ROWS, REFERENCE, DURATIONS, LABELS) == COUNTS
    assert R.constants(REFERENCE, DURATIONS, LABELS) == ([2, 1], [4.0, 4.0], 20.0)
    # just below the two thresholds the same rows fail: b [5, 7] no longer makes b a true positive, a [0, 4] becomes a false positive
    assert R.counts(ROWS[1:], REFERENCE, DURATIONS, LABELS, gtc=0.5000001)[0] == [[2, 1, 1], [0, 0, 0]]
    assert R.counts(ROWS[1:], REFERENCE, DURATIONS, LABELS, dtc=0.5000001)[0] == [[1, 1, 2], [0, 1, 0]]
    # a clip outside the reference and a zero-length detection add nothing; a present clip without events only false positives
    rows = [[(0, 0, 1.0, 3.0), (1, 0, 1.0, 3.0), (2, 1, 1.0, 3.0), (5, 0, 1.0, 3.0), (-1, 0, 1.0, 3.0), (0, 1, 6.0, 6.0)]]
    assert R.counts(rows, [REFERENCE[0], None, []], [10.0] * 3, LABELS) == [[[1, 0, 0], [0, 0, 1]]]


def _random_case(rng, C, K):
    n_gt = rng.integers(1, 7, C)
    if C > 1 and rng.random() < 0.6:
        n_gt[rng.integers(0, C)] = 0                        # a class without reference events
    gt_dur = np.where(n_gt > 0, rng.uniform(1.0, 40.0, C), 0.0)
    counts = rng.integers(0, 3, (K, C, C + 1))              # small integers: equal efpr values at several operating points
    counts[:, np.arange(C), np.arange(C)] = rng.integers(0, n_gt + 1, (K, C))      # tpr in [0, 1], in no order over k
    return counts, n_gt, gt_dur, float(rng.uniform(50.0, 500.0))


def test_finish_against_the_restatement_on_random_counts():
    """20 seeded count tensors over C in {1, 3, 10} and K in {1, 2, 9}; among them duplicated efpr values, a class with n_c = 0 and
    tpr that is not monotone over k (each asserted to occur); five settings each, to 1e-12"""
    rng = np.random.default_rng(2020)
    shapes = [(C, K) for C in (1, 3, 10) for K in (1, 2, 9)]
    seen = {'duplicate': 0, 'empty class': 0, 'non-monotone': 0}
    for i in range(20):
        C, K = shapes[i % len(shapes)]
        counts, n_gt, gt_dur, total = _random_case(rng, C, K)
        live = n_gt > 0
        seen['empty class'] += int((~live).any())
        seen['duplicate'] += int(any(len(set(counts[:, c, C].tolist())) < K for c in np.nonzero(live)[0]))
        diag = counts[:, np.arange(C), np.arange(C)]
        seen['non-monotone'] += int(K > 2 and any((np.diff(diag[:, c]) > 0).any() and (np.diff(diag[:, c]) < 0).any() for c in np.nonzero(live)[0]))
        for setting in ((0, 0, 100), (1, 0, 100), (0, 1, 100), (1, 1, 50), (0.5, 0.5, 1000)):
            got = psds_from_counts(counts, n_gt, gt_dur, total, *setting)
            want = R.score(counts.tolist(), n_gt.tolist(), gt_dur.tolist(), total, *setting)
            assert 0.0 <= got <= 1.0 and abs(got - want) <= 1e-12, (i, C, K, setting, got, want)
    assert all(v > 0 for v in seen.values()), seen


def test_refusals():
    counts = np.array(COUNTS)
    with pytest.raises(ValueError, match='no class has a reference event'):
        psds_from_counts(counts, [0, 0], [0.0, 0.0], 20.0, 0, 0, 100)
    for bad in (0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_efpr'):
            psds_from_counts(counts, [2, 1], [4.0, 4.0], 20.0, 0, 0, bad)
    with pytest.raises(ValueError, match='counts'):
        psds_from_counts(counts[:, :, :2], [2, 1], [4.0, 4.0], 20.0, 0, 0, 100)
    with pytest.raises(ValueError, match='total duration'):
        psds_from_counts(counts, [2, 1], [4.0, 4.0], 0.0, 0, 0, 100)
    with pytest.raises(ValueError, match='T_c'):
        psds_from_counts(counts, [2, 1], [4.0, 0.0], 20.0, 0, 0, 100)
