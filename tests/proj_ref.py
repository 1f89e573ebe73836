"""Float64 references for the input gradient of a strided 1x1 projection and for the residual map that carries it (SedtIgemm.rmap,
include/sedt_hip.h) - a helper of tests/test_proj_compact_cpu.py and tests/test_proj_compact_gpu.py, not a conftest.

Tokens are NHWC: a map is a matrix [B * H * W, C].  The dense reference is torch.nn.grad.conv2d_input in float64; coarse_rows() is the
header's index formula written out, checked against it on the CPU."""
import numpy as np
import torch
from torch.nn.grad import conv2d_input


def nchw(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def out_hw(Hi, Wi, sh, sw):
    return (Hi - 1) // sh + 1, (Wi - 1) // sw + 1


def dense_proj_dgrad(gy, w, B, Hi, Wi, s):
    """gy [B * Ho * Wo, Co], w [Co, Ci] (float64) -> the input gradient [B * Hi * Wi, Ci] of the 1x1 stride-s convolution, pad 0"""
    Ho, Wo = out_hw(Hi, Wi, s, s)
    Co, Ci = w.shape
    return nhwc(conv2d_input((B, Ci, Hi, Wi), w.view(Co, Ci, 1, 1), nchw(gy, B, Ho, Wo), stride=s))


def scatter_dense(side_c, B, Hi, Wi, s):
    """side_c [B * Ho * Wo, C] on the coarse grid -> [B * Hi * Wi, C], zeros off the grid: conv2d_input with the identity as its weight,
    so that it does not depend on coarse_rows()"""
    C = side_c.shape[1]
    return dense_proj_dgrad(side_c.double(), torch.eye(C, dtype=torch.float64), B, Hi, Wi, s)


def coarse_rows(B, Hi, Wi, sh, sw):
    """(fine, coarse): the rows of the [B * Hi * Wi] map that take a residual, and the row of the coarse map each one reads - the
    formula of SedtIgemm.rmap"""
    rH, rW = out_hw(Hi, Wi, sh, sw)
    row = torch.arange(B * Hi * Wi)
    n, rem = row // (Hi * Wi), row % (Hi * Wi)
    h, w = rem // Wi, rem % Wi
    on = (h % sh == 0) & (w % sw == 0)
    coarse = (n * rH + h // sh) * rW + w // sw
    return row[on], coarse[on]


def divmod_f32(a, b):
    """the kernels' division (csrc/igemm3.hip, res_row): float32 reciprocal estimate, one integer correction each way.  a: int64
    array of values in [0, 2^24), b: positive int"""
    a = np.asarray(a, dtype=np.int64)
    q = (a.astype(np.float32) * (np.float32(1.0) / np.float32(b))).astype(np.int64)
    r = a - q * b
    lo = r < 0
    q, r = q - lo, r + lo * b
    hi = r >= b
    return q + hi, r - hi * b
