#!/usr/bin/env python3
"""What one eager C2 train step launches, for comparing two checkouts of the project (a refactor of the Python-side dispatch must not move
a launch): the lib.launch_log() counter of one step in bf16 and in f32 with GEMM_X3 (bf16x3), and of one recorded step (ops.PROFILE = [])
the (dtype code, shape tuple, hint) of every entry plus the fused-Bottleneck records.  Model and inputs as bench.py's C2.

The peak of torch's allocator over the logged step goes into the file too: an intermediate kept or dropped by mistake moves it.

usage:  python tools/launch_probe.py <checkout root> <output .json> [batch size, default 64] [frozen]
        (run it once per checkout, compare the two files; `frozen` builds the model with lr_backbone = 0)
"""
import json
import os
import sys

root, dst = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import torch
from sound_event_detection_transformer_amd import runtime, ops, lib as L
from sound_event_detection_transformer_amd.sedt import build_model, default_args
from sound_event_detection_transformer_amd.engine import build_optimizer, train_step
from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict, synthetic_batch
assert os.path.abspath(ops.__file__).startswith(root), ops.__file__
dev = torch.device('cuda', 0)
B, T = (int(sys.argv[3]) if len(sys.argv) > 3 else 64), 500
frozen = 'frozen' in sys.argv[4:]
out = {'root': root, 'B': B, 'frozen': frozen, 'has_conv_form': hasattr(ops, 'conv_form'), 'has_block_plan': hasattr(ops, 'block_form')}


def setup(mode):
    runtime.set_compute_dtype(mode)
    model, criterion, _ = build_model(default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.1, **(dict(lr_backbone=0.0) if frozen else {})))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.to(dev).train()
    criterion.to(dev)
    opt = build_optimizer(model)
    x, targets = synthetic_batch(B, T, 2020, torch.device('cpu'))
    return model, criterion, opt, x.to(dev), targets


for mode in ('bf16', 'bf16x3'):
    model, criterion, opt, x, targets = setup(mode)
    for _ in range(2):
        train_step(model, criterion, opt, x, targets, None, slice(B), max_norm=0.1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with L.launch_log() as log:
        loss, _ = train_step(model, criterion, opt, x, targets, None, slice(B), max_norm=0.1)
    torch.cuda.synchronize()
    out['max_memory_allocated_' + mode] = torch.cuda.max_memory_allocated()
    out['launches_' + mode] = dict(sorted(log.items()))
    out['loss_' + mode] = float(loss)
    ops.PROFILE = []
    del ops.PROFILE_FUSED[:]
    try:
        train_step(model, criterion, opt, x, targets, None, slice(B), max_norm=0.1)
        rec = ops.PROFILE
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    out['recorded_' + mode] = [[e[1], list(e[2]), (list(e[4]) if isinstance(e[4], tuple) else e[4])] for e in rec]
    out['fused_' + mode] = [list(f) for f in ops.PROFILE_FUSED]
    del model, criterion, opt
json.dump(out, open(dst, 'w'), indent=0)
print('probe', root, 'B', B, 'frozen', frozen,
      {k: (sum(v.values()) if k.startswith('launches') else len(v) if isinstance(v, list) else v) for k, v in out.items()
       if k.split('_')[0] in ('launches', 'recorded', 'fused', 'loss', 'max')})
