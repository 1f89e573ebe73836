"""CPU: the float64 restatement behind tests/test_backbone_envelope_gpu.py (tests/conv_check.py) against torch.nn modules in float64, in
the geometries of the fused Bottleneck kernels; the bound of tests/gemm_check.py against the tensor-maximum tolerance of the older
tests; and the case table (tests/backbone_cases.py) against the edges it has to cover."""
import pytest
import torch
import torch.nn as nn

import backbone_cases as BC
import conv_check as CC
from gemm_check import U_BF16

# (name, in channels, planes, stride, projection skip, map width)
GEOMS = [('layer1_identity', 256, 64, 1, False, 16), ('layer1_block0', 64, 64, 1, True, 16), ('layer2_identity', 512, 128, 1, False, 8),
         ('layer2_block0', 256, 128, 2, True, 16), ('layer3_identity', 1024, 256, 1, False, 4)]


class TorchBottleneck(nn.Module):
    """torchvision v1.5 Bottleneck (stride on the 3x3) with eval-mode BatchNorm2d"""

    def __init__(self, cin, planes, stride, proj, gen):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm2d(planes), nn.BatchNorm2d(planes), nn.BatchNorm2d(4 * planes)
        self.down = nn.Sequential(nn.Conv2d(cin, 4 * planes, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * planes)) if proj else None
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / m.weight[0].numel() ** 0.5)
                elif isinstance(m, nn.BatchNorm2d):
                    n = m.num_features
                    m.weight.copy_(1 + 0.3 * torch.randn(n, generator=gen))
                    m.bias.copy_(0.2 * torch.randn(n, generator=gen))
                    m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
                    m.running_var.copy_(1 + 0.5 * torch.rand(n, generator=gen))
        self.double().eval()

    def forward(self, x):
        a = torch.relu(self.bn1(self.conv1(x)))
        b = torch.relu(self.bn2(self.conv2(a)))
        skip = x if self.down is None else self.down(x)
        return a, b, torch.relu(self.bn3(self.conv3(b)) + skip)


def _sb(bn):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return s.detach(), (bn.bias - bn.running_mean * s).detach()


@pytest.mark.parametrize('name,cin,planes,stride,proj,W', GEOMS, ids=[g[0] for g in GEOMS])
def test_restatement_matches_torch_nn(name, cin, planes, stride, proj, W):
    gen = torch.Generator().manual_seed(len(name))
    m = TorchBottleneck(cin, planes, stride, proj, gen)
    H = 9                                                   # odd: the stride-2 form's last output row reads the zero row below
    x = torch.randn(2, cin, H, W, generator=gen, dtype=torch.float64).relu()
    with torch.no_grad():
        a, b, y = m(x)
    sb = [_sb(m.bn1), _sb(m.bn2), _sb(m.bn3)] + ([_sb(m.down[1])] if proj else [])
    ref = CC.bottleneck(x, m.conv1.weight.detach(), m.conv2.weight.detach(), m.conv3.weight.detach(), sb, stride=stride,
                        skip=m.down[0].weight.detach() if proj else None, rnd=lambda t: t)
    assert ref['y'][0].shape == y.shape == (2, 4 * planes, (H - 1) // stride + 1, (W - 1) // stride + 1)
    for st, want in (('a', a), ('b', b), ('y', y)):
        v, ab = ref[st]
        assert torch.allclose(v, want, rtol=1e-12, atol=1e-12), (name, st, (v - want).abs().max().item())
        assert (ab >= v.abs() * (1 - 1e-12)).all(), (name, st)          # |s| |W||X| + |bias| (+ |skip|) bounds the value
    # stage-conditioned: feeding the stage its own input back reproduces it
    ref2 = CC.bottleneck(x, m.conv1.weight.detach(), m.conv2.weight.detach(), m.conv3.weight.detach(), sb, stride=stride,
                         skip=m.down[0].weight.detach() if proj else None, A=a, Bt=b, rnd=lambda t: t)
    assert torch.allclose(ref2['y'][0], y, rtol=1e-12, atol=1e-12)
    # the input-gradient restatement of a stride-1 3x3 against autograd
    if stride == 1:
        g = torch.randn(2, planes, H, W, generator=gen, dtype=torch.float64)
        xa = a.detach().clone().requires_grad_(True)
        torch.nn.functional.conv2d(xa, m.conv2.weight.detach(), padding=1).backward(g)
        v, ab = CC.conv_t(g, m.conv2.weight.detach(), pad=1)
        assert torch.allclose(v, xa.grad, rtol=1e-12, atol=1e-12) and (ab >= v.abs() * (1 - 1e-12)).all()


def test_check_flags_a_wrong_border_element_that_close_accepts():
    """one element of the first (zero-padded) row of a small-valued clip off by 1 % of the tensor's maximum: the 2e-2-of-the-maximum
    tolerance (tests/test_bneck_gpu.py: rel, tests/test_ops_gpu.py: close) lets it through, the element-wise bound does not; an
    unwritten (NaN) element fails as such"""
    gen = torch.Generator().manual_seed(3)
    m = TorchBottleneck(256, 64, 1, False, gen)
    B, H, W = 2, 9, 16
    x = torch.randn(B, 256, H, W, generator=gen, dtype=torch.float64).relu()
    x[0] /= 64                                              # clip 0 small, clip 1 large: neighbouring clips of a strip walk
    x = CC.q(x)
    sb = [_sb(m.bn1), _sb(m.bn2), _sb(m.bn3)]
    ref = CC.bottleneck(x, CC.q(m.conv1.weight.detach()), CC.q(m.conv2.weight.detach()), CC.q(m.conv3.weight.detach()), sb)
    v, ab = (CC.tok(t) for t in ref['y'])
    got = CC.q(v).clone()
    assert CC.bound_check(got, v, ab, 64) <= 0.5                                 # bf16 rounding alone: half the budget
    row, col = 3, int(v[3].argmax())                        # clip 0, image row 0 (a border row), column 3
    bad = got.clone()
    bad[row, col] += 0.01 * v.abs().max()
    rel = ((bad - v).abs().max() / v.abs().max()).item()
    assert rel < 2e-2                                       # what rel() / close() accept
    with pytest.raises(AssertionError, match='over the bound'):
        CC.bound_check(bad, v, ab, 64, what='border row')
    bad = got.clone()
    bad[row, col] = float('nan')
    with pytest.raises(AssertionError, match='non-finite'):
        CC.bound_check(bad, v, ab, 64, what='unwritten')
    assert U_BF16 == 2.0 ** -8


def test_pool_reference_takes_the_first_maximal_in_bounds_tap():
    s1 = torch.zeros(1, 3, 4, 1, dtype=torch.float64)
    s1[0, 0, 0, 0] = s1[0, 0, 1, 0] = 2.0                  # a tie in the first window: kh 1, kw 1 (top-left in bounds) wins
    m, code = CC.pool3s2(s1)
    assert m.shape == (1, 2, 2, 1) and m[0, 0, 0, 0] == 2 and code[0, 0, 0, 0] == 4
    assert m[0, 1, 1, 0] == 0 and code[0, 1, 1, 0] == 0    # all zero: the first in-bounds tap (kh 0, kw 0)
    assert code[0, 0, 1, 0] == 3                           # window (0, 1): row -1 is out of bounds, pixel (0, 1) = tap kh 1, kw 0


def test_case_table_covers_the_strip_edges():
    fams = {c.fam for c in BC.CASES}
    assert fams == {'l1', 'l2', 'l3', 'b0', 'b2', 'stem', 'c64'}
    names = [c.name for c in BC.CASES]
    assert len(set(names)) == len(names)
    for fam in ('l1', 'l2', 'b0', 'b2'):
        walks = [BC.walk(c.fam, c.B, c.H) for c in BC.BY_FAM[fam]]
        assert any(spw == 1 for _, spw, _ in walks), fam
        assert any(n == 257 for n, _, _ in walks), fam                          # the last workgroup gets one strip
        assert any(n % spw and spw >= 2 for n, spw, _ in walks), fam            # a short last workgroup
        assert any(c.B == 64 for c in BC.BY_FAM[fam]), fam
        hs = {c.H for c in BC.BY_FAM[fam]}
        assert {1, 7, 9, 17} <= hs, fam
    for fam in ('l1', 'b0', 'b2'):
        assert any(spw >= 3 and n % spw for n, spw, _ in (BC.walk(c.fam, c.B, c.H) for c in BC.BY_FAM[fam])), fam
    for fam, h in (('l1', 125), ('l2', 63), ('l3', 32), ('b0', 125), ('b2', 125), ('c64', 125)):     # production heights at 500 frames
        assert any(c.H == h for c in BC.BY_FAM[fam]), fam
    assert {c.H % 2 for c in BC.BY_FAM['b2']} == {0, 1} and {c.H % 2 for c in BC.BY_FAM['stem']} == {0, 1}
    assert {500, 496} <= {c.H for c in BC.BY_FAM['stem']} and any(c.H == 13 for c in BC.BY_FAM['l1'])
    assert any(BC.walk('stem', c.B, c.H)[1] >= 3 for c in BC.BY_FAM['stem'])
    assert any(BC.walk('c64', c.B, c.H)[1] >= 3 for c in BC.BY_FAM['c64'])
    # layer3: both sides of both ends of the dispatch window, and the decision each row expects
    n3 = {BC.walk('l3', c.B, c.H)[0]: c.path for c in BC.BY_FAM['l3']}
    assert {191, 192, 512, 513} <= set(n3)
    for n, path in n3.items():
        assert path == ('bneck3' if 192 <= n <= 512 else 'per-op'), (n, path)
    # the sampled clips include both sides of a clip boundary inside a workgroup where there is one
    cl = BC.sample_clips('l1', 41, 125)
    assert {0, 1, 40} <= set(cl)
