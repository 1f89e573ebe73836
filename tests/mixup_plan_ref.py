"""NumPy restatement of sedt_mixup_plan (csrc/mixplan.hip; DESIGN.md section 4, "Mix-up and mean-teacher training on recordings"),
written from the definition, at the level of the tables: a source of all-strong clips read under a static split goes in, the
dynamic-split tables with ratio, the job records and the status come out.  Its own oracle is the host plan
(utilities.mixup.plan_mixup_data followed by TargetTables.load): tests/test_mixup_plan_cpu.py compares the two.

A batch is a list of (labels int64 [n], boxes float32 [m, 2]) per clip, m <= n."""
import numpy as np

JOB = np.dtype([('src1', np.int32), ('src2', np.int32), ('mode', np.int32), ('lam', np.float32)])
KEEP1_EMPTY, KEEP2, WEAK, KEEP1_EVENTS, KEEP1_OVERLAP, STRONG = 'keep-1 (empty partner)', 'keep-2', 'weak merge', \
    'keep-1 (max_events)', 'keep-1 (overlap)', 'strong merge'


def lam_pair(lam):
    return np.asarray([lam, 1 - lam], np.float32)


def source_blob(clips, max_targets):
    """the blob sedt_cut_clips writes for these clips (every clip strong), as uint8; a clip with fewer boxes than labels (a weak clip
    of a hand-made batch) gets its own box offsets"""
    B = len(clips)
    nl = [len(c[0]) for c in clips]
    nb = [len(np.asarray(c[1]).reshape(-1, 2)) for c in clips]
    assert max(nl + [0]) <= max_targets and all(b <= l for b, l in zip(nb, nl))
    off = np.concatenate([[0], np.cumsum(nl), [0], np.cumsum(nb), [B, B]]).astype(np.int32)
    o_lab = 8 * B + 16
    o_box = o_lab + 8 * B * max_targets
    raw = np.zeros(o_box + 8 * B * max_targets, np.uint8)
    raw[:off.nbytes] = off.view(np.uint8)
    lab = np.concatenate([np.asarray(c[0], np.int64) for c in clips]) if B else np.zeros(0, np.int64)
    box = np.concatenate([np.asarray(c[1], np.float32).reshape(-1, 2) for c in clips]) if B else np.zeros((0, 2), np.float32)
    raw[o_lab:o_lab + lab.nbytes] = lab.view(np.uint8)
    raw[o_box:o_box + box.nbytes] = box.reshape(-1).view(np.uint8)
    return raw


def read_source(raw, B_src, max_targets):
    """(lab_off, box_off, lab_cat, box_cat) views of a source blob"""
    o_lab = 8 * B_src + 16
    o_box = o_lab + 8 * B_src * max_targets
    off = raw[:4 * (2 * B_src + 4)].view(np.int32)
    return (off[:B_src + 1], off[B_src + 1:2 * B_src + 2], raw[o_lab:o_box].view(np.int64),
            raw[o_box:o_box + 8 * B_src * max_targets].view(np.float32).reshape(-1, 2))


def clash(labels, boxes):
    """a same-class overlap anywhere: box k carries label k; s = c - l / 2, e = c + l / 2 in float32, pair-wise"""
    n = len(boxes)
    two = np.float32(2)
    for j in range(n):
        sj, ej = boxes[j, 0] - boxes[j, 1] / two, boxes[j, 0] + boxes[j, 1] / two
        for k in range(j):
            if labels[k] != labels[j]:
                continue
            sk, ek = boxes[k, 0] - boxes[k, 1] / two, boxes[k, 0] + boxes[k, 1] / two
            if not (ej < sk) and not (ek < sj):
                return True
    return False


def mixup_plan(raw, B_src, max_targets_src, B, ns, n_lab, index, lam, mix_num, max_events, max_targets_out):
    """-> dict(off int32 [2 B + 4], lab int64 [n], box float32 [m, 2], ratio float32 [n], jobs JOB [B], status int32 [B],
    outcomes [mix_num] (which row of the decision table applied))"""
    assert 1 <= B <= B_src <= 1024 and 0 <= ns <= n_lab <= B and 0 <= mix_num <= ns
    assert 1 <= max_events <= max_targets_out <= 63 and 1 <= max_targets_src <= 63
    lab_off, box_off, lab_cat, box_cat = read_source(np.asarray(raw), B_src, max_targets_src)
    lam2 = lam_pair(lam)
    labels = lambda b: lab_cat[lab_off[b]:lab_off[b + 1]] if b < n_lab else lab_cat[:0]
    boxes = lambda b: box_cat[box_off[b]:box_off[b + 1]] if b < ns else box_cat[:0]
    status = np.zeros(B, np.int32)
    one = lambda n: np.ones(n, np.float32)
    unchanged = lambda b: (b, labels(b), boxes(b), one(len(labels(b))), (b, 0, 1, 0.0))
    strong, weak, outcomes = [], [], []
    for i in range(mix_num):
        j = int(index[i])
        if not 0 <= j < B:
            status[i] = 2
            strong.append(unchanged(i))
            outcomes.append('bad index')
            continue
        n1, n2 = len(boxes(i)), len(boxes(j))
        merged_lab = np.concatenate([labels(i), labels(j)])
        merged_ratio = np.concatenate([np.full(len(labels(i)), lam2[0], np.float32), np.full(len(labels(j)), lam2[1], np.float32)])
        if n1 == 0 or n2 == 0:
            if n1 > 0:
                strong.append(unchanged(i)); outcomes.append(KEEP1_EMPTY)
            elif n2 > 0:
                strong.append((i, labels(j), boxes(j), one(len(labels(j))), (0, j, 2, 0.0))); outcomes.append(KEEP2)
            else:
                weak.append((i, merged_lab, box_cat[:0], merged_ratio, (i, j, 0, lam2[0]))); outcomes.append(WEAK)
        elif n1 + n2 > max_events:
            strong.append(unchanged(i)); outcomes.append(KEEP1_EVENTS)
        else:
            merged_box = np.concatenate([boxes(i), boxes(j)])
            if clash(merged_lab, merged_box):
                strong.append(unchanged(i)); outcomes.append(KEEP1_OVERLAP)
            else:
                strong.append((i, merged_lab, merged_box, merged_ratio, (i, j, 0, lam2[0]))); outcomes.append(STRONG)
    results = strong + [unchanged(b) for b in range(mix_num, ns)] + weak + [unchanged(b) for b in range(ns, B)]
    assert len(results) == B
    ns_out = ns - len(weak)
    M = max_targets_out
    nl, nb = [], []
    for src, l, bx, r, job in results:
        if len(l) > M:
            status[src] = 1
        nl.append(min(len(l), M))
        nb.append(min(len(bx), M))
    assert all(n == 0 for n in nb[ns_out:])
    off = np.concatenate([[0], np.cumsum(nl), [0], np.cumsum(nb), [ns_out, n_lab]]).astype(np.int32)
    return {'off': off,
            'lab': np.concatenate([r[1][:M] for r in results]).astype(np.int64),
            'box': np.concatenate([r[2][:M] for r in results]).astype(np.float32).reshape(-1, 2),
            'ratio': np.concatenate([r[3][:M] for r in results]).astype(np.float32),
            'jobs': np.asarray([r[4] for r in results], JOB), 'status': status, 'outcomes': outcomes}


def read_tables(raw, B, max_targets):
    """a dynamic-split TargetTables blob with ratio (uint8) -> dict(off, lab, box, ratio): the live entries only"""
    raw = np.asarray(raw)
    cap = B * max_targets
    o_lab = 8 * B + 16
    off = raw[:4 * (2 * B + 4)].view(np.int32).copy()
    nl, nb = int(off[B]), int(off[2 * B + 1])
    return {'off': off, 'lab': raw[o_lab:o_lab + 8 * nl].view(np.int64).copy(),
            'box': raw[o_lab + 8 * cap:o_lab + 8 * cap + 8 * nb].view(np.float32).reshape(-1, 2).copy(),
            'ratio': raw[o_lab + 16 * cap:o_lab + 16 * cap + 4 * nl].view(np.float32).copy()}


def assert_same_tables(got, want):
    """offsets, split words, live labels equal; live boxes and ratios bit-equal"""
    assert got['off'].tolist() == want['off'].tolist()
    assert got['lab'].tolist() == want['lab'].tolist()
    bits = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)
    assert np.array_equal(bits(got['box']), bits(want['box']))
    assert np.array_equal(bits(got['ratio']), bits(want['ratio']))


def assert_same_jobs(got, want):
    got, want = np.asarray(got).view(JOB).reshape(-1), np.asarray(want, JOB).reshape(-1)
    assert got.tobytes() == want.tobytes(), (got, want)


def to_list(clips, ns, n_lab, torch):
    """the list-of-dicts form of a batch under the split: empty boxes from clip ns on, empty labels from clip n_lab on"""
    out = []
    for b, (l, bx) in enumerate(clips):
        l = np.asarray(l, np.int64) if b < n_lab else np.zeros(0, np.int64)
        bx = np.asarray(bx, np.float32).reshape(-1, 2) if b < ns else np.zeros((0, 2), np.float32)
        out.append({'labels': torch.from_numpy(l.copy()), 'boxes': torch.from_numpy(bx.copy()), 'orig_size': torch.tensor(10.0)})
    return out


def host_route(clips, ns, n_lab, lam, index, mix_num, max_events, max_targets, torch):
    """the oracle: plan_mixup_data on the list form, then TargetTables.load(mixed, ns=, n_lab=) on CPU tables -> (tables dict, jobs)"""
    from sound_event_detection_transformer_amd.sedt import TargetTables
    from sound_event_detection_transformer_amd.utilities.mixup import plan_mixup_data
    B = len(clips)
    y = to_list(clips, ns, n_lab, torch)
    ratio = (mix_num + 0.5) / B                                   # int(B * ratio) == mix_num
    assert int(B * ratio) == mix_num
    jobs, mixed, n_strong, n_weak = plan_mixup_data(y, slice(ns), slice(ns, n_lab), lam, index, ratio, max_events)
    assert len(mixed) == B
    tab = TargetTables(B, ns, n_lab, torch.device('cpu'), max_targets=max_targets, with_ratio=True, dynamic_split=True)
    tab.load(mixed, ns=n_strong, n_lab=n_strong + n_weak)
    return read_tables(tab._blob.numpy(), B, max_targets), np.asarray(jobs, JOB)


# ---------------------------------------------------------------------------------------------------- cases
def case(clips, ns, n_lab, index, mix_num, max_events, M_src=8, M_out=None, lam=0.3, B=None):
    """one launch: ``clips`` is the source (B_src clips), of which the first B are the batch"""
    B = len(clips) if B is None else B
    clips = [(np.asarray(l, np.int64), np.asarray(b, np.float32).reshape(-1, 2)) for l, b in clips]
    return dict(clips=clips, B=B, ns=ns, n_lab=n_lab, index=np.asarray(index, np.int32), lam=lam, mix_num=mix_num, max_events=max_events,
                M_src=M_src, M_out=M_src if M_out is None else M_out)


def reference(c):
    return mixup_plan(source_blob(c['clips'], c['M_src']), len(c['clips']), c['M_src'], c['B'], c['ns'], c['n_lab'], c['index'], c['lam'],
                      c['mix_num'], c['max_events'], c['M_out'])


def oracle(c, torch):
    return host_route(c['clips'][:c['B']], c['ns'], c['n_lab'], c['lam'], c['index'], c['mix_num'], c['max_events'], c['M_out'], torch)


def host_outcomes(c, jobs):
    """which row of the decision table every mixed clip took, read off the HOST plan's job records (and the inputs for the reason of a
    keep-1): {outcome: count}"""
    import collections
    n = collections.Counter()
    nb = lambda b: len(c['clips'][b][1]) if b < c['ns'] else 0
    kept = [j for j in jobs if j['mode'] == 1 and j['src1'] < c['mix_num']]
    for j in jobs:
        if j['mode'] == 2:
            n[KEEP2] += 1
        elif j['mode'] == 0:
            i, p = int(j['src1']), int(j['src2'])
            n[WEAK if nb(i) == 0 and nb(p) == 0 else STRONG] += 1
    for j in kept:
        i = int(j['src1'])
        p = int(c['index'][i])
        if nb(p) == 0:
            n[KEEP1_EMPTY] += 1
        elif nb(i) + nb(p) > c['max_events']:
            n[KEEP1_EVENTS] += 1
        else:
            n[KEEP1_OVERLAP] += 1
    return n


def random_case(rng, B=None, B_src=None, classes=4, M=8, ns=None, n_lab=None, mix_num=None, p_empty=0.25):
    B = int(rng.integers(2, 11)) if B is None else B
    B_src = B if B_src is None else B_src
    ns = int(rng.integers(1, B + 1)) if ns is None else ns
    n_lab = int(rng.integers(ns, B + 1)) if n_lab is None else n_lab
    clips = []
    for b in range(B_src):
        n = 0 if rng.random() < p_empty else int(rng.integers(1, 4))
        lab = rng.integers(0, classes, n)
        length = rng.uniform(0.05, 0.3, n)
        centre = rng.uniform(length / 2, 1 - length / 2)
        clips.append((lab, np.stack([centre, length], 1) if n else np.zeros((0, 2))))
    mix_num = int(rng.integers(0, ns + 1)) if mix_num is None else mix_num
    index = rng.permutation(B) if rng.random() < 0.5 else rng.integers(0, B, B)
    return case(clips, ns, n_lab, index, mix_num, int(rng.integers(3, 6)), M_src=M, lam=float(rng.beta(1, 1)), B=B)


def designed_cases():
    """{name: case}: the shapes and events at which the plan can go wrong (tests/test_mixup_plan_gpu.py lists them)"""
    f = np.float32
    e = lambda *boxes: [list(b) for b in boxes]
    A, Bx, C = ([1], e((0.2, 0.1))), ([2], e((0.6, 0.2))), ([3, 1], e((0.8, 0.1), (0.5, 0.1)))
    empty = ([], [])
    d = {}
    d['B1'] = case([A], 1, 1, [0], 0, 4)
    d['B2 both merge'] = case([A, Bx], 2, 2, [1, 0], 2, 4)
    # 3 strong (the second one without events) | 1 weak with two tags | 1 unlabelled
    five = [C, empty, A, ([4, 5], e((0.5, 1.0), (0.5, 1.0))), empty]
    d['B5 partner weak, two clips one partner, self'] = case(five, 3, 4, [3, 3, 2, 0, 1], 3, 4)      # keep-1 | weak merge with tags | self overlap
    d['B5 empty partner either side, partner unlabelled'] = case(five, 3, 4, [1, 0, 4, 2, 3], 3, 4)  # keep-1 | keep-2 | keep-1
    d['B5 both empty'] = case([empty, empty, A, ([4], e((0.5, 1.0))), empty], 3, 4, [1, 4, 0, 3, 2], 2, 4)     # weak merges without labels
    d['B5 of a source of 7'] = case(five + [Bx, C], 3, 4, [2, 3, 0, 1, 4], 3, 4, B=5)
    three = ([0, 1, 2], e((0.1, 0.1), (0.3, 0.1), (0.5, 0.1)))
    two = ([3, 0], e((0.7, 0.1), (0.9, 0.1)))
    d['max_events reached'] = case([three, two], 2, 2, [1, 0], 2, 5)
    d['max_events + 1'] = case([three, two], 2, 2, [1, 0], 2, 4)
    left = ([1], e((0.25, 0.5)))                                      # [0, 0.5]
    d['boxes touch'] = case([left, ([1], e((0.75, 0.5)))], 2, 2, [1, 0], 1, 4)                      # [0.5, 1.0]: e == s is a clash
    d['boxes miss by one ulp'] = case([left, ([1], [[np.nextafter(f(0.75), f(1)), f(0.5)]])], 2, 2, [1, 0], 1, 4)
    d['overlap inside clip i'] = case([([1, 1], e((0.3, 0.2), (0.35, 0.2))), Bx], 2, 2, [1, 0], 1, 4)
    d['index[i] == i'] = case([A, empty, Bx], 3, 3, [0, 1, 2], 2, 4)                                  # self overlap | weak merge with itself
    tags = lambda n: (list(range(n)), e(*[(0.5, 1.0)] * n))
    d['capacity reached'] = case([empty, A, tags(3), tags(3)], 2, 4, [2, 3, 0, 1], 1, 3, M_src=4, M_out=3)
    d['capacity + 1'] = case([empty, A, tags(4), tags(3)], 2, 4, [2, 3, 0, 1], 1, 3, M_src=4, M_out=3)   # the weak merge and clip 2: 4 labels
    # one lane per box: 32 + 31 events of 63 classes merge under max_events = 63; 32 + 32 are one too many
    many = lambda lo, n: (list(range(lo, lo + n)), e(*[((k + 0.5) / 64, 0.01) for k in range(lo, lo + n)]))
    d['63 events merge'] = case([many(0, 32), many(32, 31)], 2, 2, [1, 0], 2, 63, M_src=63)
    d['64 events do not'] = case([many(0, 32), many(32, 32)], 2, 2, [1, 0], 2, 63, M_src=63)
    return d
