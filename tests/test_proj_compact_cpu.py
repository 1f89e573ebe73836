"""CPU: the identities the compact projection gradient rests on (ops.proj_dgrad, SedtIgemm.rmap), in float64 - so that the reference
tests/test_proj_compact_gpu.py trusts is itself checked without a GPU.

  * the input gradient of a 1x1 stride-s convolution (pad 0) is the plain GEMM gy W on the OUTPUT grid, scattered to the pixels with
    row % s == 0 and column % s == 0, and zero elsewhere - odd map heights included (125 -> 63, 7 -> 4: the last coarse row maps to the
    last fine row);
  * the row formula of SedtIgemm.rmap is that scatter;
  * the kernels' float-reciprocal division is exact below 2^24."""
import numpy as np
import pytest
import torch

import proj_ref as R

# (B, Hi, Wi, Ci, Co): layer2's and layer3's block 0 at two clips, then small maps with odd / even heights and both widths
SHAPES = [(2, 125, 16, 256, 512), (2, 63, 8, 512, 1024), (1, 7, 4, 24, 40), (3, 8, 6, 16, 8), (2, 7, 16, 8, 16), (2, 8, 8, 8, 16)]


@pytest.mark.parametrize('B,Hi,Wi,Ci,Co', SHAPES)
def test_strided_projection_gradient_is_a_plain_gemm_on_the_coarse_grid(B, Hi, Wi, Ci, Co):
    g = torch.Generator().manual_seed(Hi * 100 + Wi)
    Ho, Wo = R.out_hw(Hi, Wi, 2, 2)
    gy = torch.randn(B * Ho * Wo, Co, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, generator=g, dtype=torch.float64) / Co ** 0.5
    dense = R.dense_proj_dgrad(gy, w, B, Hi, Wi, 2)
    side_c = gy @ w                                             # [B Ho Wo, Ci]: no geometry at all
    fine, coarse = R.coarse_rows(B, Hi, Wi, 2, 2)
    assert len(fine) == B * Ho * Wo and torch.equal(coarse, torch.arange(B * Ho * Wo))      # each coarse pixel is read exactly once, in order
    scat = torch.zeros_like(dense)
    scat[fine] = side_c[coarse]
    scale = float(dense.abs().max())
    assert float((scat - dense).abs().max()) <= 1e-12 * scale
    off = torch.ones(B * Hi * Wi, dtype=torch.bool)
    off[fine] = False
    assert float(dense[off].abs().max()) == 0.0                 # off the grid the gradient is exactly zero
    # (what the dense form wastes: at C2's maps one pixel in four carries a value)
    share = len(fine) / (B * Hi * Wi)
    assert abs(share - Ho * Wo / (Hi * Wi)) < 1e-15 and 0.25 <= share <= 0.33
    # the identity-weight scatter the GPU test uses is the same map
    assert torch.equal(R.scatter_dense(side_c, B, Hi, Wi, 2), scat)


@pytest.mark.parametrize('sh,sw', [(2, 2), (1, 2), (3, 2), (2, 1)])
def test_coarse_rows_follow_the_convolution_for_other_strides(sh, sw):
    from torch.nn.grad import conv2d_input
    B, Hi, Wi, C = 2, 11, 9, 4
    rH, rW = R.out_hw(Hi, Wi, sh, sw)
    side_c = torch.randn(B * rH * rW, C, dtype=torch.float64, generator=torch.Generator().manual_seed(sh * 10 + sw))
    dense = R.nhwc(conv2d_input((B, C, Hi, Wi), torch.eye(C, dtype=torch.float64).view(C, C, 1, 1), R.nchw(side_c, B, rH, rW), stride=(sh, sw)))
    fine, coarse = R.coarse_rows(B, Hi, Wi, sh, sw)
    scat = torch.zeros_like(dense)
    scat[fine] = side_c[coarse]
    assert torch.equal(scat, dense)


def test_reciprocal_division_is_exact_below_2_pow_24():
    """divisors the residual map meets (pixels per image, map width, strides) and awkward ones; numerators: every value near a
    multiple of the divisor, the top of the range, and a seeded sample"""
    rng = np.random.default_rng(7)
    for b in (1, 2, 3, 4, 5, 7, 8, 15, 16, 63 * 8, 125 * 16, 2000, 4095, 4095 * 4095 // 7, 4095 * 4095):
        top = 1 << 24
        mult = np.arange(0, top, b, dtype=np.int64)
        if len(mult) > 200000:
            mult = mult[rng.integers(0, len(mult), 200000)]
        a = np.concatenate([mult, mult - 1, mult + 1, mult + b - 1, np.arange(top - 70000, top), rng.integers(0, top, 200000)])
        a = a[(a >= 0) & (a < top)]
        q, r = R.divmod_f32(a, b)
        assert np.array_equal(q, a // b) and np.array_equal(r, a % b), b
