"""the bf16 attention backward alone, at the three shapes a C2 step runs it (B = 64, H = 8), with and without dropout: a captured graph of
20 launches replayed 20 times, so the figure is the kernel plus the gap to the next launch and not the host's issue rate.  Inputs stay
in the caches between launches; inside a step they do not (profiles/r10_ab_attn_bwd.txt has both).
usage: python tools/time_attn_bwd.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sound_event_detection_transformer_amd import ops      # noqa: E402

B, H, N = 64, 8, 20
for Lq, Lk in ((128, 128), (11, 128), (11, 11)):
    for p in (0.0, 0.1):
        q = torch.randn(B * Lq, 256, device='cuda').bfloat16()
        k = torch.randn(B * Lk, 256, device='cuda').bfloat16()
        v, do = torch.randn_like(k), torch.randn_like(q)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(k)
        o, lse = ops.attention_fwd(1, q, k, v, B, H, Lq, Lk, drop_p=p, seed=1)

        def fn():
            ops.attention_bwd(1, q, k, v, o, do, lse, B, H, Lq, Lk, dq, dk, dv, drop_p=p, seed=1)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                for _ in range(N):
                    fn()
        g.replay()
        torch.cuda.synchronize()
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            g.replay()
        b_.record()
        torch.cuda.synchronize()
        print(f'{Lq:4d} {Lk:4d} p {p}: bwd {a.elapsed_time(b_) / (20 * N) * 1e3:6.2f} us per launch (graph of {N})', flush=True)
