"""Rows for tests/test_target_envelope_gpu.py and tests/test_target_check_cpu.py: the kernels that decide what the model is trained
towards - csrc/criterion.hip (match_targets, set_criterion, set_criterion_bwd) and csrc/postproc.hip (postprocess, pseudo_labels,
feature_loss + its reduce, sum_f32, scale_layers).  A row is one launch (criterion rows: the forward launch and three backward
launches); every row is run whole, nothing is sampled.  Inputs are generated from the row by tests/target_check.py.

Work split of each kernel, and the edges the rows sit on:

match_targets     one 64-lane workgroup per (dense layer, strong clip) and one more for the bookkeeping (tgt_len, gt_weak: lane = clip,
                  stride 64 over B).  The class cost of a query row lives in registers when C + 1 <= 16 and takes a loop over global
                  memory above.  The assignment solver runs with one lane per COLUMN, columns 1..m in lanes 1..m: n <= Q targets are
                  the rows and the queries the columns (Q = 63: lane 63 is a live column and the result moves one lane down through a
                  shuffle); n > Q swaps the roles and scatters the result through an int view of the LDS tile.  LDS is
                  Q (C + 1 + 2 max_targets) floats.  Capacity: Q <= 63, C <= 63, n <= max_targets <= 63, L <= 8.
set_criterion     ONE workgroup of 1024 threads: thread = (dense layer, clip, query) row with stride 1024 over L B Q, the same two
                  row paths at C + 1 <= 16 / above; one wave per (layer, quantity) column adds B Q row values with stride 64; the
                  audio-tag terms run over Bat C (and Bp C) elements with stride 1024; the per-clip cardinality counters are
                  L B <= 8192 LDS words.
set_criterion_bwd 256-thread workgroups over the L B Qs head rows; rows outside [q0, q0 + Q) get zeros.
postprocess       one wave per clip, lane = query (Q <= 64; Q = 64: every lane is a query), a butterfly arg-max per class.
pseudo_labels     ONE workgroup of 16 waves, wave w takes clips w, w + 16, ...; lane = query; ranks by shuffles, the greedy pass by
                  ballots; LDS 2 B + 1 + 3 B Q + C words (above 64 KB the launch needs the raised dynamic-LDS attribute, above 150 KB
                  the entry point refuses); offsets clamp at cap and the tail is dropped.
feature_loss      one wave per (layer, clip, query) row, four rows per workgroup, lanes stride 64 over F / 4 float4 (F < 256: idle
                  lanes); the reduce adds ns Q row losses per layer with 256 threads.
sum_f32           one workgroup of 256 threads, stride 256.
scale_layers      grid (min(ceil(n4 / 256), 2048 / L + 1), L) of 256 threads over per_layer / 4 float4, grid-stride above the cap.
"""
import collections

Case = collections.namedtuple('Case', 'family name shape flags seed edge')


def _c(family, name, shape, seed, edge, **flags):
    return Case(family, name, shape, flags, seed, edge)


def _m(name, Q, n, seed, edge, C=10, L=3, B=None, ns=None, n_lab=None, Qs=None, q0=0, mt=None, split=None, **flags):
    """a matching shape: n = events per strong clip (cycled); B defaults to len(n), every clip strong"""
    B = len(n) if B is None else B
    ns = B if ns is None else ns
    n_lab = ns if n_lab is None else n_lab
    shape = dict(L=L, B=B, ns=ns, n_lab=n_lab, Q=Q, Qs=Q + q0 if Qs is None else Qs, q0=q0, C=C, n=tuple(n),
                 mt=max(max(n), 1) if mt is None else mt, split=split)
    return _c('match', name, shape, seed, edge, **flags)


MATCH = [
    _m('q63_n63_62_1', 63, (63, 62, 1), 1, 'Q = 63: lane 63 is a live column; n = Q, Q - 1 and 1'),
    _m('q20_n20_21_63', 20, (20, 21, 63), 2, 'n = Q, the first n > Q (roles swapped, LDS scatter) and the capacity'),
    _m('q4_n63', 4, (63, 63), 3, 'few queries, a full target table: scatter from lanes 1..63'),
    _m('q1_n1_5', 1, (1, 5), 4, 'one query: 1 x 1 and 1 x 5 problems'),
    _m('empty_next_to_full', 20, (0, 20, 0, 63), 5, 'an empty clip between full ones'),
    _m('c15', 10, (3, 12), 6, 'C + 1 = 16: the last register-path width', C=15),
    _m('c16', 10, (3, 12), 7, 'C + 1 = 17: the first looped width', C=16),
    _m('c63_q63_n63', 63, (63, 7), 8, 'C = 63 with the largest tile: 47.9 KB of LDS', C=63),
    _m('c1', 10, (3, 12), 9, 'C = 1', C=1),
    _m('focal_c17', 10, (3, 12), 10, 'focal cost on a looped row', C=17, fl=True),
    _m('focal_c10', 20, (5, 20, 30), 11, 'focal cost, register-sized row', fl=True),
    _m('l1', 10, (3, 12), 12, 'L = 1', L=1),
    _m('l8', 10, (3, 12), 13, 'L = 8', L=8),
    _m('q0_1_qs64', 63, (63, 5), 14, 'query window q0 = 1 of Qs = 64 head rows, Q = 63', q0=1),
    _m('ns_lt_b', 10, (4, 11), 15, 'ns < n_lab < B: weak clips carry labels only, the last clips nothing', B=6, ns=2, n_lab=4),
    _m('b65', 4, (2, 5), 16, 'bookkeeping block: B = 65, one clip past the first stride', B=65, ns=2, n_lab=65),
    _m('b130', 4, (2, 5), 17, 'bookkeeping block: B = 130, three strides', B=130, ns=2, n_lab=100),
    _m('split_0', 10, (4, 11, 3), 18, 'split words (0, n_lab): no strong clip at all', B=5, ns=3, n_lab=5, split=(0, 5)),
    _m('split_ns', 10, (4, 11, 3), 19, 'split words equal to the capacities', B=5, ns=3, n_lab=5, split=(3, 5)),
    _m('split_more', 10, (4, 11, 3), 20, 'split words above the capacities: clamped', B=5, ns=3, n_lab=5, split=(6, 8)),
    _m('split_less', 10, (4, 11, 3), 21, 'split words below the capacities: clips move to the weak side', B=5, ns=3, n_lab=5,
       split=(2, 4)),
    _m('ratio_mt63', 63, (63, 30, 1), 22, 'positional mix-up ratios, max_targets = 63', mt=63, ratio=True),
    _m('normalize_mt63', 20, (5, 20, 63), 23, 'normalize, max_targets = 63', mt=63, norm=True),
    _m('ft_eps3_mt63', 20, (3, 10, 20, 63), 24, 'fine-tune re-matching with injected uniforms, epsilon 3', mt=63, ft=True, eps=3.0),
    _m('ft_norm_ratio', 20, (3, 10, 20), 25, 'fine-tune + normalize with ratios', mt=63, ft=True, norm=True, ratio=True, eps=3.0),
    _m('ft_q63', 63, (63, 20), 26, 'fine-tune at Q = 63: the prefix mask of lane 62', mt=63, ft=True, eps=3.0, alpha=0.7),
    _m('tie', 6, (4, 4), 27, 'two identical queries and two identical targets: a tie', tie=True),
]

# criterion rows: a matching shape (the dense targets come from the float64 reference) plus what the loss kernel adds
_CR = []


def _cr(name, Q, n, seed, edge, Bat=None, Bp=None, wp_all=False, nb_given=False, **kw):
    fl = {k: kw.pop(k) for k in ('fl', 'ratio', 'norm', 'special') if k in kw}
    m = _m(name, Q, n, seed, edge, **kw)
    sh = dict(m.shape, Bat=Bat, Bp=Bp)
    _CR.append(_c('criterion', name, sh, seed, edge, wp_all=wp_all, nb_given=nb_given, **fl))


for _C in (15, 16, 63):
    _cr(f'c{_C}', 10, (3, 10, 0), 40 + _C, f'C + 1 = {_C + 1}', C=_C, Bat=3)
    _cr(f'c{_C}_focal', 10, (3, 10, 0), 140 + _C, f'C + 1 = {_C + 1}, focal', C=_C, Bat=3, fl=True)
_cr('q63_n63', 63, (63, 62, 1), 30, 'the widest matching shape', Bat=3)
_cr('q4_n63', 4, (63, 63), 31, 'every query matched, most targets unmatched')
_cr('lbq1023', 31, (3, 0, 31, 7), 32, 'L B Q = 1023: the last row of the first stride', B=11)
_cr('lbq1024', 32, (3, 0, 32, 7), 33, 'L B Q = 1024: the stride exactly', L=4, B=8)
_cr('lbq1025', 41, (3, 0, 41, 7), 34, 'L B Q = 1025: one row in the second pass', L=5, B=5)
_cr('bq63', 21, (3, 21, 5), 35, 'B Q = 63: one idle lane in the column sums')
_cr('bq64', 16, (3, 16, 5, 1), 36, 'B Q = 64')
_cr('bq65', 13, (3, 13, 5, 1, 0), 37, 'B Q = 65: one element in the second pass of the column sums')
_cr('l1', 10, (3, 12), 38, 'L = 1', L=1, Bat=2)
_cr('l8', 10, (3, 12), 39, 'L = 8', L=8, Bat=2)
_cr('lb8192_q1', 1, (1, 0, 2), 40, 'L B = 8192: every cardinality counter in use', L=8, B=1024)
_cr('bat16_c63', 4, (2, 5), 41, 'Bat C = 1008: the audio-tag loop below its stride', C=63, B=16, ns=2, n_lab=5, Bat=16)
_cr('bat17_c63', 4, (2, 5), 42, 'Bat C = 1071: the audio-tag loop past its stride', C=63, B=17, ns=2, n_lab=5, Bat=17)
_cr('atp_weak', 10, (3, 5), 43, 'pooled tags on the weak clips, Bp > n_lab', B=6, ns=2, n_lab=4, Bat=6, Bp=6)
_cr('atp_all', 10, (3, 5, 1, 2), 44, 'pooled tags with weak_mask None: every labelled clip', Bat=4, Bp=4, wp_all=True)
_cr('atp_empty', 10, (3, 5, 1), 45, 'pooled tags with an empty weak range: 0 / 0 like the mean over nothing', Bat=3, Bp=3)
_cr('atp_focal', 10, (3, 5), 46, 'focal audio-tag loss + pooled tags', B=6, ns=2, n_lab=4, Bat=6, Bp=6, fl=True)
_cr('nb_given', 10, (3, 12), 47, 'num_boxes handed in, not summed', nb_given=True, Bat=2)
_cr('q0_1', 10, (3, 10), 48, 'query window q0 = 1: the tag query rows of the gradients are zero', q0=1, Bat=2)
_cr('split_less', 10, (4, 10, 3), 49, 'split words below the capacities', B=5, ns=3, n_lab=5, split=(2, 4), Bat=5)
_cr('split_0', 10, (4, 10, 3), 53, 'split words (0, n_lab): no strong clip, only the audio-tag loss; the total stays finite', B=5, ns=3,
    n_lab=5, split=(0, 5), Bat=5)
_cr('ratio_norm', 20, (5, 20), 50, 'coefficients other than 1', ratio=True, Bat=2)
_cr('no_events', 10, (0, 0), 51, 'no event in any strong clip: num_boxes = 0, the reference divides by zero', Bat=2)
_cr('coincident', 4, (3,), 52, 'start == start, end == end and a touching pair: the sub-gradients of |x|, min, max, clamp', C=3, L=1,
    special='coincident')
CRITERION = _CR

# postprocess: B, Q, C, at_m (None: no tags), is_semi
POST = [_c('post', f'q{Q}_c{C}_b{B}_at{m}_{"semi" if s else "abs"}{"_lane63" if l63 else ""}', dict(B=B, Q=Q, C=C), seed, edge,
           at_m=m, semi=s, lane63=l63)
        for seed, (B, Q, C, m, s, l63, edge) in enumerate([
            (3, 64, 10, 2, False, False, 'Q = 64: every lane is a query'),
            (3, 64, 10, 3, True, True, 'a class whose best query is lane 63'),
            (3, 63, 10, 2, False, False, 'Q = 63: one idle lane in the butterfly'),
            (3, 1, 10, 2, False, False, 'Q = 1'),
            (2, 20, 63, 2, False, False, 'C = 63'),
            (2, 20, 63, 3, True, False, 'C = 63, at_m 3'),
            (2, 5, 1, 2, False, False, 'C = 1'),
            (3, 20, 10, 1, False, False, 'at_m 1'),
            (3, 20, 10, 1, True, False, 'at_m 1, semi'),
            (3, 20, 10, 3, False, False, 'at_m 3'),
            (3, 20, 10, None, False, False, 'no tags'),
            (3, 20, 10, None, True, False, 'no tags, semi'),
            (1, 64, 63, 2, True, True, 'B = 1, the widest clip'),
        ], 60)]

# pseudo labels: B, Q, C, nms, tags, cap ('big', 'total', 'minus1', 'mid', 'boundary')
PSEUDO = [_c('pseudo', f'b{B}_q{Q}_c{C}_{"nms" if nms else "order"}_{"at" if at else "noat"}_{cap}', dict(B=B, Q=Q, C=C), seed, edge,
             nms=nms, at=at, cap=cap)
          for seed, (B, Q, C, nms, at, cap, edge) in enumerate([
              (3, 64, 10, True, True, 'big', 'Q = 64: the prefix mask of lane 63'),
              (3, 64, 10, False, True, 'big', 'Q = 64, query order'),
              (3, 1, 10, True, True, 'big', 'Q = 1'),
              (3, 20, 63, True, True, 'big', 'C = 63'),
              (15, 20, 10, True, True, 'total', 'B = 15: one idle wave; cap == total'),
              (16, 20, 10, True, True, 'minus1', 'B = 16: one clip per wave; cap one below the total'),
              (17, 20, 10, True, True, 'mid', 'B = 17: wave 0 loops twice; cap in the middle of a clip'),
              (33, 20, 10, True, False, 'boundary', 'B = 33: three passes; no tag gate; cap at a clip boundary'),
              (33, 20, 10, False, True, 'mid', 'query order with a cap in the middle of a clip'),
              (100, 64, 10, True, True, 'big', 'B Q = 6400: 77 KB of LDS, above the 64 KB line'),
          ], 80)]

# feature loss: L, B, ns, Q, P, F
FEATURE = [_c('feature', name, dict(L=L, B=B, ns=ns, Q=Q, P=P, F=F), seed, edge, zero=zero, base=base)
           for seed, (name, L, B, ns, Q, P, F, zero, base, edge) in enumerate([
               ('f4_rows5', 1, 1, 1, 5, 3, 4, False, False, 'F = 4: one live lane; 5 rows: a partly filled workgroup'),
               ('f252_rows8', 2, 2, 2, 2, 3, 252, False, True, 'F = 252: lane 63 idle; 8 rows: two full workgroups'),
               ('f256', 3, 2, 2, 3, 4, 256, False, False, 'F = 256: every lane one float4'),
               ('f260', 3, 2, 2, 3, 4, 260, False, True, 'F = 260: lane 0 takes a second float4'),
               ('ns_lt_b', 3, 3, 2, 4, 4, 64, False, False, 'ns < B: the last clip has zero gradients and no row loss'),
               ('zero_pred', 2, 2, 2, 4, 4, 64, 'pred', False, 'a zero-norm prediction row: the clamped norm, gradients of 1e12'),
               ('zero_target', 2, 2, 2, 4, 4, 64, 'target', False, 'a zero-norm target row that a live row points at'),
               ('nsq255', 1, 5, 5, 51, 2, 8, False, False, 'ns Q = 255: the reduce one short of its stride'),
               ('nsq257', 1, 1, 1, 257, 2, 8, False, True, 'ns Q = 257: the reduce one past its stride'),
               ('l8', 8, 2, 2, 3, 4, 64, False, True, 'L = 8'),
           ], 100)]

SUM_N = (0, 1, 255, 256, 257)

# scale_layers: L, per_layer, idx (None: identity), which of g / gtot
SCALE = [_c('scale', name, dict(L=L, per=per), seed, edge, idx=idx, mode=mode)
         for seed, (name, L, per, idx, mode, edge) in enumerate([
             ('per4', 3, 4, None, 'both', 'per_layer = 4: one float4 per layer'),
             ('l1_above_cap', 1, 4 * (2049 * 256 + 5), None, 'g', 'L = 1, more float4 than 2049 workgroups hold: the grid-stride loop'),
             ('l8_perm', 8, 1028, (3, 0, 7, 1, 6, 2, 5, 4), 'gtot', 'L = 8 with a permutation'),
             ('l8_ident', 8, 8, None, 'both', 'L = 8, identity'),
             ('l3_perm', 3, 2052, (2, 0, 1), 'both', 'a permutation, two workgroups per layer'),
         ], 120)]

ALL = MATCH + CRITERION + POST + PSEUDO + FEATURE + SCALE
