"""The case table of tests/test_backbone_envelope_gpu.py: the fused backbone kernels at both sides of their strip / tile edges.

A row names the kernel family, the batch B and height H of the map the kernel reads, the input pattern and the path the dispatcher
must take there.  Families (the host entry point the row calls; its kernel):

  l1      ops.bneck_fwd / bneck_bwd, C 256 P 64 W 16     bneck_kernel<BG<256, 64, 16>, BWD, SKIP3>   layer1 identity block, H = 125
  l2      ops.bneck_fwd / bneck_bwd, C 512 P 128 W 8     bneck_kernel<BG<512, 128, 8>, BWD>          layer2 identity block, H = 63
  l3      ops.bneck_fwd / bneck_bwd, C 1024 P 256 W 4    bneck3_kernel<BWD>                          layer3 identity block, H = 32
  b0      ops.block_fwd('bneck0', ...)                   bneck0_fwd_kernel                           layer1 block 0, H = 125
  b2      ops.block_fwd('bneck2', ...)                   bneck2_fwd_kernel                           layer2 block 0, H = 125 -> 63
  stem    ops.stem_pool_fwd / stem_pool_wgrad            stem_pool_fwd_kernel, stem_pool_wgrad_kernel   H = 500 / 496 input frames
  c64     ops.conv_fwd / conv_dgrad (3x3, 64 -> 64, W 16)   conv3x3_c64_kernel                       layer1 conv2, H = 125

Work split (what the edges are edges of):
  bneck_kernel, bneck0:  strips of R = 8 rows, ceil(H / 8) per clip, nst = B * that; spw = ceil(nst / 256) consecutive strips per
                         workgroup, ceil(nst / spw) workgroups: a workgroup may cross clip boundaries, the last one may be short
  bneck2:                strips of 4 OUTPUT rows of H2 = (H - 1) // 2 + 1, same walk
  bneck3:                one 8-row strip per workgroup; the dispatcher (sedt_bneck3_ok) takes it while 192 <= nst <= 512
  stem forward:          tiles of 2 pooled rows, ceil(Hp / 2) per clip, <= 512 persistent workgroups (tile t, t + grid, ...)
  stem wgrad:            tiles of 4 un-pooled rows, min(B * ceil(Ho / 4), 512) workgroups = f32 slabs reduced afterwards
  conv3x3_c64:           tiles of 16 rows, ceil(H / 16) per clip, <= 256 persistent workgroups

Patterns: 'clip' - every clip its own magnitude (alternating x1/16 and x4 with an offset; tests/test_backbone_envelope_gpu.py: _clip_gain),
so a halo row or a strip taken from the neighbouring clip is off by a large factor, not by rounding; 'plain' - one magnitude.
"""
from collections import namedtuple

Case = namedtuple('Case', 'name fam B H pattern path')

R = 8
GRID = {'l1': 256, 'l2': 256, 'b0': 256, 'b2': 256, 'stem': 512, 'c64': 256}


def geometry(fam, H):
    """(rows per work item, work items per clip) of a family at map height H"""
    if fam in ('l1', 'l2', 'l3', 'b0'):
        return R, -(-H // R)
    if fam == 'b2':
        return 4, -(-((H - 1) // 2 + 1) // 4)
    if fam == 'stem':
        Hp = ((H - 1) // 2 + 1 - 1) // 2 + 1
        return 2, -(-Hp // 2)
    if fam == 'c64':
        return 16, -(-H // 16)
    raise KeyError(fam)


def walk(fam, B, H):
    """(work items, items per workgroup, workgroups) of a launch; for the persistent kernels 'items per workgroup' is the largest
    number of tiles one workgroup takes"""
    n = B * geometry(fam, H)[1]
    if fam == 'l3':
        return n, 1, n
    if fam in ('stem', 'c64'):
        g = min(n, GRID[fam])
        return n, -(-n // g), g
    spw = -(-n // 256)
    return n, spw, -(-n // spw)


def sample_clips(fam, B, H, limit=8):
    """clips whose float64 reference a case computes (clips are independent): first, last, middle, the clips on each side of the
    first, middle and last workgroup boundary and of the first clip boundary inside a workgroup; all of them when B is small"""
    if B <= limit:
        return list(range(B))
    per = geometry(fam, H)[1]
    n, spw, wgs = walk(fam, B, H)
    pick = {0, B - 1, B // 2}
    if fam in ('stem', 'c64'):
        bounds = [wgs, n - 1]                                  # tile `grid` is the first workgroup's second tile; the last tile
    else:
        bounds = [spw, (wgs // 2) * spw, (wgs - 1) * spw]     # first strip of workgroups 1, middle, last
    for s in bounds:
        if 0 < s < n:
            pick.update((max(s - 1, 0) // per, s // per))
    if fam not in ('stem', 'c64', 'l3'):
        for k in range(1, B):                                  # the first clip boundary inside a workgroup
            if (k * per) % spw:
                pick.update((k - 1, k))
                break
    return sorted(pick)


C = Case
CASES = [
    # ---- layer1 identity block (C 256, W 16): rows R +- 1, 2R + 1, single row, SP-SEDT patch, production; spw 1 / 2 / 3 / 4 / 5
    C('l1_h1', 'l1', 2, 1, 'clip', 'bneck'),
    C('l1_h7', 'l1', 3, 7, 'clip', 'bneck'),
    C('l1_h8', 'l1', 2, 8, 'clip', 'bneck'),
    C('l1_h9', 'l1', 3, 9, 'clip', 'bneck'),
    C('l1_h17', 'l1', 3, 17, 'clip', 'bneck'),
    C('l1_h13_patch', 'l1', 5, 13, 'clip', 'bneck'),
    C('l1_prod_b2', 'l1', 2, 125, 'plain', 'bneck'),
    C('l1_256_strips', 'l1', 16, 125, 'clip', 'bneck'),             # exactly 256 strips: spw 1, every workgroup one strip
    C('l1_257_strips', 'l1', 257, 8, 'clip', 'bneck'),              # 257: spw 2, the last workgroup one strip
    C('l1_spw3_partial', 'l1', 41, 125, 'clip', 'bneck'),           # 656 strips, spw 3, 219 workgroups, the last two strips
    C('l1_spw2_h13', 'l1', 200, 13, 'clip', 'bneck'),               # 2 strips per clip, the second 5 rows: spw 2
    C('l1_spw5_h17', 'l1', 411, 17, 'clip', 'bneck'),               # 1233 strips of 3 per clip, spw 5, the last workgroup 3
    C('l1_prod_b64', 'l1', 64, 125, 'clip', 'bneck'),               # C2: spw 4, 16 strips per clip
    # ---- layer2 identity block (C 512, W 8)
    C('l2_h1', 'l2', 2, 1, 'clip', 'bneck'),
    C('l2_h7', 'l2', 3, 7, 'clip', 'bneck'),
    C('l2_h9', 'l2', 3, 9, 'clip', 'bneck'),
    C('l2_h17', 'l2', 2, 17, 'clip', 'bneck'),
    C('l2_257_strips', 'l2', 257, 8, 'clip', 'bneck'),
    C('l2_spw3_partial', 'l2', 70, 63, 'clip', 'bneck'),            # 560 strips, spw 3, the last workgroup two
    C('l2_prod_b64', 'l2', 64, 63, 'clip', 'bneck'),                # spw 2
    # ---- layer3 identity block (C 1024, W 4): one strip per workgroup; the dispatch window 192 <= strips <= 512
    C('l3_h1_out', 'l3', 2, 1, 'clip', 'per-op'),
    C('l3_h9_out', 'l3', 3, 9, 'clip', 'per-op'),
    C('l3_h17_out', 'l3', 2, 17, 'clip', 'per-op'),
    C('l3_191', 'l3', 191, 8, 'clip', 'per-op'),
    C('l3_192', 'l3', 192, 8, 'clip', 'bneck3'),
    C('l3_prod_188', 'l3', 47, 32, 'clip', 'per-op'),
    C('l3_prod_192', 'l3', 48, 32, 'clip', 'bneck3'),
    C('l3_512', 'l3', 512, 8, 'clip', 'bneck3'),
    C('l3_513', 'l3', 513, 8, 'clip', 'per-op'),
    C('l3_prod_b64', 'l3', 64, 32, 'clip', 'bneck3'),
    # ---- layer1 block 0 (projection skip)
    C('b0_h1', 'b0', 2, 1, 'clip', 'bneck0'),
    C('b0_h7', 'b0', 3, 7, 'clip', 'bneck0'),
    C('b0_h9', 'b0', 3, 9, 'clip', 'bneck0'),
    C('b0_h17', 'b0', 2, 17, 'clip', 'bneck0'),
    C('b0_257_strips', 'b0', 257, 8, 'clip', 'bneck0'),
    C('b0_spw3_partial', 'b0', 41, 125, 'clip', 'bneck0'),
    C('b0_prod_b64', 'b0', 64, 125, 'clip', 'bneck0'),
    # ---- layer2 block 0 (3x3 stride 2): odd and even H, H2 = (H - 1) // 2 + 1 output rows in strips of 4
    C('b2_h1', 'b2', 2, 1, 'clip', 'bneck2'),
    C('b2_h7', 'b2', 3, 7, 'clip', 'bneck2'),
    C('b2_h8', 'b2', 3, 8, 'clip', 'bneck2'),
    C('b2_h9', 'b2', 3, 9, 'clip', 'bneck2'),
    C('b2_h13_patch', 'b2', 3, 13, 'clip', 'bneck2'),
    C('b2_h17', 'b2', 2, 17, 'clip', 'bneck2'),
    C('b2_h124', 'b2', 2, 124, 'clip', 'bneck2'),
    C('b2_257_strips', 'b2', 257, 8, 'clip', 'bneck2'),             # H2 = 4: one strip per clip, spw 2
    C('b2_spw3_partial', 'b2', 41, 125, 'clip', 'bneck2'),          # 656 strips, spw 3
    C('b2_prod_b64', 'b2', 64, 125, 'clip', 'bneck2'),
    # ---- stem (64 mel bands): odd / even frame counts, tiles of two pooled rows, 512 persistent workgroups
    C('stem_h1', 'stem', 2, 1, 'clip', 'stem'),
    C('stem_h9', 'stem', 3, 9, 'clip', 'stem'),
    C('stem_h13', 'stem', 3, 13, 'clip', 'stem'),
    C('stem_h37', 'stem', 2, 37, 'clip', 'stem'),
    C('stem_500', 'stem', 2, 500, 'plain', 'stem'),
    C('stem_496', 'stem', 3, 496, 'clip', 'stem'),
    C('stem_b20_500', 'stem', 20, 500, 'clip', 'stem'),             # 1260 tiles: 3 per workgroup, the last round partial
    C('stem_prod_b64', 'stem', 64, 500, 'clip', 'stem'),
    # ---- conv3x3_c64: tiles of 16 rows, 256 persistent workgroups
    C('c64_h1', 'c64', 2, 1, 'clip', 'conv3x3_c64'),
    C('c64_h7', 'c64', 3, 7, 'clip', 'conv3x3_c64'),
    C('c64_h9', 'c64', 3, 9, 'clip', 'conv3x3_c64'),
    C('c64_h17', 'c64', 2, 17, 'clip', 'conv3x3_c64'),
    C('c64_256_tiles', 'c64', 32, 125, 'clip', 'conv3x3_c64'),      # 8 tiles per clip: exactly 256 tiles
    C('c64_257_tiles', 'c64', 257, 16, 'clip', 'conv3x3_c64'),      # the first workgroup takes a second tile
    C('c64_3_rounds', 'c64', 300, 32, 'clip', 'conv3x3_c64'),       # 600 tiles: 3 rounds, the last partial
    C('c64_prod_b64', 'c64', 64, 125, 'clip', 'conv3x3_c64'),
]
BY_FAM = {}
for _c in CASES:
    BY_FAM.setdefault(_c.fam, []).append(_c)
