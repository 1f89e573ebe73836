"""Float64 restatements of the backbone's fused operations and their element-wise bound (a helper of
tests/test_backbone_envelope_gpu.py and tests/test_backbone_ref_cpu.py, not a conftest).

Every convolution is an unfold + matmul in float64 on whatever device the operands live on, and comes with the same contraction over
absolute values, so that check() (tests/gemm_check.py) can bound each element:

    |got - ref| <= c (sqrt(K) 2^-24 absprod + u_out |ref| + extra),    absprod = |s| (|W| |X|) + |bias| + |residual|

K is the contraction length of the stage (C for a 1x1 over C channels, 9 P for a 3x3 over P, 128 for the stem's packed taps), u_out
2^-8 for a bf16 output.  `extra` carries an operand that the kernel itself rounds to bf16 inside an epilogue (the projection skip of
layer1 / layer2 block 0: bf16(sd acc + bd) is added before the final ReLU): 2^-8 |that operand|.

A ReLU is 1-Lipschitz, so the bound of a pre-activation holds after it; a stage reads the kernel's OWN bf16 output of the stage before
(stage-conditioned), so a ReLU decision that lands on the neighbouring bf16 value moves nothing downstream.
"""
import math

import torch
import torch.nn.functional as F

from gemm_check import U_ACC, U_BF16, check  # noqa: F401  (U_BF16: re-exported for the tests)

def q(t):
    """bf16-rounded, as float64"""
    return t.to(torch.bfloat16).double()


def nchw(t, B, H, W):
    """[B*H*W, C] tokens -> float64 [B, C, H, W]"""
    return t.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)


def tok(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv(x, w, stride=1, pad=0):
    """float64 conv2d (no bias) of x [B, Ci, H, W] with w [Co, Ci, k, k] by unfold + matmul, and the same over |x|, |w|"""
    x, w = x.double(), w.double().to(x.device)
    B, Ci, H, W_ = x.shape
    Co, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W_ + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)                     # [B, Ci*k*k, Ho*Wo]
    wm = w.reshape(Co, -1)
    out = torch.matmul(wm, cols).view(B, Co, Ho, Wo)
    ab = torch.matmul(wm.abs(), cols.abs()).view(B, Co, Ho, Wo)
    return out, ab


def conv_t(g, w, pad=0):
    """the input gradient of a stride-1 conv with weight w [Co, Ci, k, k] (pad `pad`): a conv of g [B, Co, H, W] with the taps
    mirrored and the channels swapped"""
    return conv(g, w.transpose(0, 1).flip(2, 3), 1, pad)


def affine(acc, s, b=None):
    """(s acc + b, |s| |acc-operands| + |b|) for acc = (value, absprod) of conv(); s, b per output channel"""
    v, ab = acc
    s = s.double().to(v.device).view(1, -1, 1, 1)
    v, ab = v * s, ab * s.abs()
    if b is not None:
        b = b.double().to(v.device).view(1, -1, 1, 1)
        v, ab = v + b, ab + b.abs()
    return v, ab


def relu(t):
    return t.clamp_min(0)


def bits_of(t):
    """the kernels' sign-bit bytes of t [M, C]: bit c % 8 of byte c / 8 is [t > 0]"""
    b = (t.float() > 0).view(t.shape[0], -1, 8).to(torch.uint8)
    return (b << torch.arange(8, device=t.device, dtype=torch.uint8)).sum(-1).to(torch.uint8)


def unbits(bits, C):
    """[M, C / 8] sign-bit bytes -> bool [M, C]"""
    sh = torch.arange(8, device=bits.device, dtype=torch.uint8)
    return ((bits.unsqueeze(-1) >> sh) & 1).bool().reshape(bits.shape[0], C)


def pool3s2(s1):
    """max-pool 3x3 stride 2 pad 1 of s1 [B, H, W, C] (values >= 0): (pooled, argmax code kh * 3 + kw of the FIRST maximal in-bounds tap)"""
    B, H, W, C = s1.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = torch.full((B, H + 3, W + 3, C), -1.0, dtype=torch.float64, device=s1.device)
    pad[:, 1:H + 1, 1:W + 1] = s1.double()
    taps = torch.stack([pad[:, kh:kh + 2 * Hp:2, kw:kw + 2 * Wp:2] for kh in range(3) for kw in range(3)])     # [9, B, Hp, Wp, C]
    m = taps.max(0).values
    code = (taps == m).to(torch.uint8).argmax(0)                      # first maximal tap (torch.argmax: the first of equal maxima)
    return m, code.to(torch.uint8)


def bound_check(got, ref, absprod, K, u_out=U_BF16, extra=None, rows=None, what=''):
    """check() of tests/gemm_check.py on [M, C] tensors (got: the whole output, every element must be finite; ref / absprod: the rows
    `rows` of it), with an optional per-element extra term (see the header)"""
    if extra is not None:
        absprod = absprod + extra / (math.sqrt(K) * U_ACC)
    return check(got, ref, absprod, K, u_out, rows=rows, what=what)


def bottleneck(X, w1, w2, w3, sb, stride=1, skip=None, A=None, Bt=None, rnd=q):
    """float64 restatement of a torchvision v1.5 Bottleneck over NCHW X: conv1 1x1 -> affine -> ReLU -> conv2 3x3 (stride, pad 1) ->
    affine -> ReLU -> conv3 1x1 -> affine -> + skip -> ReLU.  sb = ((s1, b1), (s2, b2), (s3, b3)[, (sd, bd)]); skip None = identity,
    else the projection 1x1 (weight `skip`, stride `stride`) with affine sb[3], NOT rounded (the kernels add bf16 of it: the caller
    budgets that rounding as `extra` = 2^-8 |i|).
    A / Bt: the stage inputs to use for stage 2 / 3 (the kernel's own intermediates); default: this restatement's, rounded by `rnd`.
    Returns {name: (value, absprod)} for 'a', 'b', 'y' (pre-ReLU absprod, ReLU applied to the value) and 'i' (the projection)."""
    (s1, b1), (s2, b2), (s3, b3) = sb[:3]
    a_v, a_ab = affine(conv(X, w1), s1, b1)
    out = {'a': (relu(a_v), a_ab)}
    A = rnd(relu(a_v)) if A is None else A
    b_v, b_ab = affine(conv(A, w2, stride, 1), s2, b2)
    out['b'] = (relu(b_v), b_ab)
    Bt = rnd(relu(b_v)) if Bt is None else Bt
    y_v, y_ab = affine(conv(Bt, w3), s3, b3)
    if skip is None:
        I, I_ab = X, X.abs()
    else:
        I, I_ab = affine(conv(X, skip, stride), *sb[3])
    out['i'] = (I, I_ab)
    out['y'] = (relu(y_v + I), y_ab + I_ab)
    return out
