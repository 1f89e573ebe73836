"""Float64 references and element-wise error bounds for the GEMM kernels (a helper of tests/test_gemm_envelope_gpu.py, not a conftest).

Bound.  Element (i, j) of a GEMM result may differ from the float64 result of the same (dtype-rounded) operands by

    |got - ref| <= c * (sqrt(K) * u_acc * (|A| |B|)_ij + u_x3 * (|A| |B|)_ij + u_out * |ref_ij|) + tiny

where |A| |B| is the same contraction over absolute values (float64), u_acc = 2^-24 (f32 accumulation), u_x3 = 2^-16 in the bf16x3
mode (the dropped lo * lo term and the rounding of lo) and 0 otherwise, u_out = 2^-8 for a bf16 output and 0 for an f32 one, and
c = 2 (a bf16 output's own rounding alone reaches 2^-8 |ref|).  The accumulation term grows with sqrt(K), the growth the kernels
show, not with the worst case K: measured on MI355X the K * u_acc form was ~500x looser than every f32-output result and let a
split-K reduction that dropped its last slice (4 of 516 K blocks at K = 33,000) pass.  The inputs are seeded, so the ratios a run
reports are reproducible; tests/test_gemm_envelope_gpu.py records the largest ones.

The budget is per element: a wrong row, tile or K slice fails however small its values are, where a bound relative to the largest
output (tests/test_ops_gpu.py: close()) lets it through.  check() reports the failing rows and columns as ranges, so a wrong 64-row
tile shows as "rows 128-191".

Unwritten elements.  poison() fills the caching allocator's free memory with NaN before a kernel call, so the next torch.empty
(split-K slabs, column-sum scratch, outputs) starts as NaN; outputs passed as out= are NaN-filled too.  A non-finite element in a
result is an element no kernel wrote.
"""
import math

import numpy as np
import torch

U_ACC = 2.0 ** -24
U_BF16 = 2.0 ** -8
U_X3 = 2.0 ** -16
TINY = 1e-30


def poison(mb=256):
    """release the allocator's cached blocks, then hand it back NaN-filled ones: large blocks (one mb MiB segment) and the small
    pool (2 MiB segments of <= 1 MiB blocks)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    big = torch.full((mb << 18,), float('nan'), device='cuda', dtype=torch.float32)
    small = [torch.full((1 << 18,), float('nan'), device='cuda', dtype=torch.float32) for _ in range(16)]
    torch.cuda.synchronize()
    del big, small


def nan_buffer(n, dtype):
    return torch.full((n,), float('nan'), device='cuda', dtype=dtype)


def sample_index(n, tile, extra=64, seed=0):
    """indices 0..n-1 to check: both edges of every tile boundary (and the last index) plus `extra` seeded random ones; all of them
    when n is small"""
    if n <= 4 * tile:
        return torch.arange(n)
    edges = set([0, n - 1])
    for b in range(tile, n, tile):
        edges.update((b - 1, b))
    g = torch.Generator().manual_seed(seed)
    edges.update(torch.randint(0, n, (extra,), generator=g).tolist())
    return torch.tensor(sorted(edges))


def _ranges(idx):
    idx = sorted(set(int(i) for i in idx))
    out, start, prev = [], None, None
    for i in idx:
        if start is None:
            start = prev = i
        elif i == prev + 1:
            prev = i
        else:
            out.append((start, prev))
            start = prev = i
    if start is not None:
        out.append((start, prev))
    s = ', '.join(f'{a}' if a == b else f'{a}-{b}' for a, b in out[:8])
    return s + (f', ... ({len(out)} ranges)' if len(out) > 8 else '')


def check(got, ref, absprod, K, u_out, x3=False, c=2.0, rows=None, cols=None, what=''):
    """element-wise bound of the header on got (any device / dtype) against the float64 ref and |A||B| (same shape as got, or as
    got[rows][:, cols] when rows / cols - index tensors - are given; every element of got must be finite either way).  Returns the
    largest error / bound ratio."""
    got = got.detach().double().cpu()
    if got.dim() == 1:
        got, ref, absprod = got[:, None], ref[:, None], absprod[:, None]
    bad = ~torch.isfinite(got)                      # (every element, sampled rows or not)
    if bad.any():
        rr, cc = bad.nonzero(as_tuple=True)
        raise AssertionError(f'{what}: {int(bad.sum())} non-finite (unwritten?) elements, rows {_ranges(rr.tolist())}, '
                             f'cols {_ranges(cc.tolist())}')
    if rows is not None:
        got = got[rows]
    if cols is not None:
        got = got[:, cols]
    ref, absprod = ref.double(), absprod.double()
    assert got.shape == ref.shape == absprod.shape, (what, got.shape, ref.shape, absprod.shape)
    r_idx = rows if rows is not None else torch.arange(got.shape[0])
    c_idx = cols if cols is not None else torch.arange(got.shape[1])
    bound = c * ((math.sqrt(K) * U_ACC + (U_X3 if x3 else 0.0)) * absprod + u_out * ref.abs()) + TINY
    ratio = (got - ref).abs() / bound
    worst = float(ratio.max())
    if worst > 1.0:
        bad = ratio > 1.0
        rr, cc = bad.nonzero(as_tuple=True)
        i, j = np.unravel_index(int(ratio.argmax()), tuple(ratio.shape))
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements over the bound (worst ratio {worst:.3g} at row '
                             f'{int(r_idx[i])} col {int(c_idx[j])}: got {float(got[i, j]):.6g} ref {float(ref[i, j]):.6g}); '
                             f'rows {_ranges(r_idx[rr].tolist())}; cols {_ranges(c_idx[cc].tolist())}')
    return worst
