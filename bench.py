#!/usr/bin/env python3
"""Headline benchmark: SEDT training throughput (audio clips/s) on synthetic batches, one process per GPU.

    python bench.py --gpus N --steps K --warmup W [--config c2|c3|c4|c5] [--dtype bf16|f32] [--dump-outputs DIR] [--full]

N > 1 without a launcher: this script starts N ranks ITSELF (``python -m torch.distributed.run`` as a child process,
before the parent touches the GPU) and relays rank 0's JSON line.  Under a launcher (WORLD_SIZE set) it is one rank;
``--gpus`` must equal WORLD_SIZE.

A step = one full training step of the chosen BASELINE.json configuration, as HIP graphs, inputs resident in HBM:
  c2 (default, the metric's config): URBAN-SED SEDT E=3 dec_at Q=10 B=64/GPU bf16 - forward, on-device Hungarian matching +
      SetCriterion, backward, clip 0.1, AdamW, dropout 0.1
  c3: DCASE SEDT E=6 Q=20, B=32 = 16 strong + 16 weak clips
  c4: SP-SEDT pre-training E=6 Q=20, 10 patches per clip, B=200/GPU, backbone frozen, feature-reconstruction loss
  c5: mean-teacher step E=6 Q=20: 32 labelled (16+16) + 32 unlabelled clips through teacher (no grad) and student
Prints ONE JSON line (rank 0): clips/s over all ranks and `roofline` (whole-step MFMA roofline from HIP events on the launch
stream + PMC traffic from profiles/).  A plain run does nothing else: set-up, settle, warm-up, the timed steps, --dump-outputs.
--full adds, after the timed region, what takes runs of its own: `roofline.gemm_family` (the GEMM family replayed alone) and
`roofline.families` (per-kernel rooflines), `kernels` (per-kernel MFMA utilisation / HBM GB/s for the north-star kernels, timed
live with HIP events), `other_configs`, `cpu_baseline` (the CPU oracle on this box's host cores), `clocks_under_load`,
`host_launch_us_per_step` and, at N > 1, `exposed_comm`; the --no-* switches drop single legs of it.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic work per clip, fwd + bwd, 2*MAC, wgrad skipped for frozen tensors
FLOP_PER_CLIP = {'c2': 27.37e9, 'c3': 30.00e9, 'c4': 35.63e9, 'eval': 9.458e9}      # SURVEY.md 8(d); eval = C2 forward only
FLOP_C5_STEP_64 = (32 * 30.00 + 32 * 10.33 + 32 * 30.00) * 1e9      # labelled fwd+bwd, teacher fwd, student fwd+bwd
MFMA_PEAK = {'bf16': 2.5e15, 'f32': 157.3e12, 'bf16x3': 2.5e15}       # dense peaks, MI355X_MICROARCH.md (bf16x3 issues 3 bf16 MFMA flops per
                                                                       # algorithmic flop: its fraction of the bf16 peak is capped at 1/3)
HBM_PEAK = 8.0e12


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--settle', type=int, default=100,
                    help='captured steps only: un-timed replays right after the capture, before --warmup (the first replays run slow)')
    ap.add_argument('--config', default='c2', choices=['c2', 'c3', 'c4', 'c5', 'eval'],
                    help="BASELINE.json configuration (default c2 = the headline metric); 'eval' = the validation body of "
                         "engine.get_sedt_predictions at the C2 shape (an extra, not a BASELINE metric)")
    ap.add_argument('--batch', type=int, default=None, help='clips per GPU (default: the config\'s own)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32', 'bf16x3'],
                    help="bf16 = throughput mode (BASELINE configs[1]); f32 = exact-f32 parity mode; bf16x3 = parity-grade fast mode (f32 tensors, "
                         "split-bf16 products: meets the 1e-3 tolerance)")
    ap.add_argument('--full', action='store_true',
                    help='after the timed region, also run what the headline figure does not need: GEMM family and per-kernel rooflines, '
                         'the per-kernel report, the other configurations and precisions, the CPU baseline, clocks under load, host '
                         'issue time, exposed communication (the --no-* switches below drop single legs of it)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernels', action='store_true', help='skip the per-kernel report')
    ap.add_argument('--dump-igemm', default=None, help='write per-launch igemm timings (json) to this path')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after the timed steps, write what the last timed step returned (losses / predictions) and a fixed sample of '
                         'the parameters and gradients it left as DIR/<name>.npy (float32 / float64, at most 64 MB): two builds run '
                         'with the same arguments see the same inputs and can be compared output for output')
    ap.add_argument('--host-matching', action='store_true',
                    help='c2/c3: solve the Hungarian matching on the host between two HIP graphs (the reference split)')
    ap.add_argument('--no-graph', action='store_true', help='c2/c3: issue every kernel from Python instead of replaying HIP graphs')
    ap.add_argument('--model-only', action='store_true', help='c2: time fwd+bwd of the model with a fixed differentiable loss')
    ap.add_argument('--no-overlap', action='store_true', help='data parallel: one all-reduce after the backward (no cut)')
    ap.add_argument('--dp-cuts', default='coarse', choices=['none', 'coarse', 'fine'],
                    help='data parallel: where the backward is cut so that the all-reduce of one segment overlaps the backward of the '
                         'next (engine.dp_segment_plan); none = one all-reduce after the backward')
    ap.add_argument('--bf16-buckets', action='store_true', help='data parallel: bf16 flat gradient buffer (half the all-reduce bytes)')
    ap.add_argument('--async-wgrad', action='store_true', help='experiment: weight gradients as a parallel graph branch (second stream)')
    ap.add_argument('--no-other-configs', action='store_true',
                    help='default c2 line only: skip the bounded c3 / c4 / c5 measurements attached as "other_configs"')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'],
                    help="process-group backend; 'gloo' (flat gradient segments staged through the host) exists for the multi-GPU readiness "
                         "test on a one-GPU box (tests/test_dp_gpu.py): it exercises this file's rank path, not RCCL")
    ap.add_argument('--share-gpu', action='store_true', help='readiness test: every rank uses cuda:0')
    ap.add_argument('--force-graph-fallback', action='store_true',
                    help='readiness test: pretend the captured data-parallel stepper cannot be built (every rank then has to agree on the '
                         'eager fallback out of band)')
    ap.add_argument('--no-clocks', action='store_true', help='skip the rocm-smi clock reading under load')
    ap.add_argument('--no-gemm-family', action='store_true',
                    help='skip the eager recorded step + the back-to-back replay of every GEMM launch (roofline.gemm_family): use under rocprofv3 '
                         'so that the kernel statistics hold the captured step only')
    ap.add_argument('--no-families', action='store_true',
                    help='skip roofline.families (the in-process kernel trace of three extra steps; use under rocprofv3, which owns the tracer)')
    ap.add_argument('--loader', action='store_true',
                    help='c2: feed every step from HOST-resident raw mel batches (pinned double buffer -> H2D on a copy stream -> '
                         'sedt_box_transform -> graphed step) instead of replaying a device-resident batch')
    ap.add_argument('--mix-up-ratio', type=float, default=None,
                    help='mix-up inside the step (engine.py:50-53, 128-133, 150-153); default: 0.6 for c5 (its recipe), off for c2/c3')
    return ap.parse_args()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """N > 1 and no launcher: start the ranks as a CHILD process tree before this process makes any GPU call"""
    import torch
    have = torch.cuda.device_count()              # (does not initialise the GPU on this image)
    if have < args.gpus:
        print(f'bench.py: --gpus {args.gpus} but only {have} GPU(s) visible', file=sys.stderr)
        return 2
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def host_cores():
    """cores this process may really use: physical cores, capped by the affinity mask and the cgroup CPU quota"""
    n = os.cpu_count() or 1
    try:
        import psutil
        n = psutil.cpu_count(logical=False) or n
    except Exception:
        pass
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        q, p = open('/sys/fs/cgroup/cpu.max').read().split()
        if q != 'max':
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return max(1, n)


def cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except Exception:
        pass
    return 'unknown'


def cpu_baseline(budget_s=25.0):
    """the CPU oracle (pure-PyTorch restatement of the reference path, pinned to the reference by tests/golden) on this box's
    host cores: BASELINE.md section 3 - C1 (B=4) and B=64, threads = usable physical cores, full step and fwd+bwd only."""
    import torch
    from oracle import sedt_oracle as O
    from oracle.criterion_oracle import build_oracle_criterion
    from sound_event_detection_transformer_amd.utilities.synthetic import synthetic_batch
    cores = host_cores()
    torch.set_num_threads(cores)
    model = O.build_oracle_model(10, 10, 3, 3, True, True, True, dropout=0.1)
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), 2020))
    model.train()
    crit = build_oracle_criterion(10, 3, True, True)
    groups = [{"params": [p for n, p in model.named_parameters() if "backbone" not in n and p.requires_grad]},
              {"params": [p for n, p in model.named_parameters() if "backbone" in n and p.requires_grad], "lr": 1e-4}]
    opt = torch.optim.AdamW(groups, lr=1e-4, weight_decay=1e-4)

    def run(batch, max_steps, budget, full=True):
        x, targets = synthetic_batch(batch, 500, 2020, None)

        def step():
            ld, _ = crit(model(x), targets, None, slice(batch))
            loss = sum(ld[k] * crit.weight_dict[k] for k in ld if k in crit.weight_dict)
            loss.backward()
            if full:
                torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
                opt.step()
            opt.zero_grad()
        step()                                   # warm-up
        n, t0 = 0, time.perf_counter()
        while n < max_steps and (n == 0 or time.perf_counter() - t0 < budget):
            step()
            n += 1
        return batch * n / (time.perf_counter() - t0), n
    c1, n1 = run(4, 5, budget_s * 0.15)
    b64, n64 = run(64, 5, budget_s * 0.55)
    fb, nfb = run(64, 2, budget_s * 0.2, full=False)
    return {"value": round(b64, 3), "unit": "clips/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(),
            "c1_b4_clips_per_s": round(c1, 3), "b64_fwd_bwd_only_clips_per_s": round(fb, 3),
            "sample": f"CPU oracle, URBAN-SED SEDT E=3 Q=10 dec_at, f32, dropout on, torch.set_num_threads({cores}): "
                      f"1 warm-up + {n64} full train steps at B=64 (value), 1+{n1} at B=4 (BASELINE config C1), "
                      f"1+{nfb} fwd+bwd-only at B=64"}


def clocks_under_load(step, seconds=1.5):
    """{'sclk_mhz': ..., 'mclk_mhz': ...} read by `rocm-smi --showclocks` in a child process while this process keeps replaying the step
    (an idle GPU drops its clocks within milliseconds, so the reading has to be taken with the step running); None when the tool is
    missing or prints nothing parseable.  A diagnostic for 'why does this box read 3 % slower': never allowed to cost the result line"""
    import re
    import shutil
    import torch
    tool = shutil.which('rocm-smi') or '/opt/rocm/bin/rocm-smi'
    if not os.path.exists(tool):
        return None
    try:
        child = subprocess.Popen([tool, '--showclocks'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        t0 = time.perf_counter()
        while child.poll() is None and time.perf_counter() - t0 < 20.0:
            step()
        torch.cuda.synchronize()
        if child.poll() is None:
            child.kill()
            return None
        out = child.stdout.read()
        res = {}
        for key in ('sclk', 'mclk', 'fclk'):
            m = re.search(key + r' clock level[^(]*\((\d+)\s*Mhz\)', out, re.I)
            if m:
                res[key + '_mhz'] = int(m.group(1))
        return res or {"raw": out.strip()[:300]}
    except Exception as e:                           # noqa: BLE001
        return {"error": repr(e)[:120]}


def agree_out_of_band(ok, rank, world, tag, timeout_s=180.0):
    """all ranks learn whether EVERY rank built its captured data-parallel stepper - through the process group's TCP store, not
    through a collective: a rank whose constructor threw is no longer in step with ranks still inside the constructor's
    collectives, and one more all-reduce would pair up with the wrong call.  Returns True (all built), False (none built: every
    rank may take the same fallback), and exits the process with status 3 on a mixed outcome or when a rank never reports
    (the launcher then tears the job down instead of letting it hang)."""
    import datetime
    import torch.distributed as dist
    store = dist.distributed_c10d._get_default_store()
    store.set(f'{tag}/{rank}', '1' if ok else '0')
    try:
        store.wait([f'{tag}/{r}' for r in range(world)], datetime.timedelta(seconds=timeout_s))
    except Exception as e:                          # noqa: BLE001
        print(f'bench.py: rank {rank}: not every rank reported on "{tag}" within {timeout_s:.0f} s ({e!r})', file=sys.stderr)
        os._exit(3)
    votes = [store.get(f'{tag}/{r}') == b'1' for r in range(world)]
    if all(votes):
        return True
    if not any(votes):
        return False
    print(f'bench.py: rank {rank}: ranks disagree on "{tag}" ({votes}): aborting', file=sys.stderr)
    os._exit(3)


# ---------------------------------------------------------------------------------------------------------------------
def build_workload(args, dev, rank, world):
    """returns (step callable, clips per step per rank, flop per step per rank, description, graphed flag, extras)"""
    import torch
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    from sound_event_detection_transformer_amd.engine import build_optimizer, GraphedTrainStep, GraphedSemiStep, train_step
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict, synthetic_batch, synthetic_targets
    from sound_event_detection_transformer_amd.utilities.utils import EMA
    cfg = args.config
    seed = 2020 + rank

    def to_dev(ts):
        return [{k: v.to(dev) for k, v in t.items()} for t in ts]
    extras = {}
    if cfg in ('c2', 'c3'):
        E, Q, T = (3, 10, 500) if cfg == 'c2' else (6, 20, 496)
        B = args.batch or (64 if cfg == 'c2' else 32)
        ns = B if cfg == 'c2' else B // 2
        model, criterion, _ = build_model(default_args(enc_layers=E, num_queries=Q, dec_at=True, dropout=0.1))
        model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
        model.to(dev).train()
        criterion.to(dev)
        opt = build_optimizer(model)
        mix = args.mix_up_ratio or 0.0
        # the targets stay on the host, where a loader leaves them: TargetTables lays them out in pinned memory and sends ONE
        # host->device copy per step (device-resident targets cost two concatenation kernels and three copies)
        x, targets = synthetic_batch(B, T, seed, torch.device('cpu'))
        x = x.to(dev)
        for t in targets[ns:]:
            t['boxes'] = torch.zeros(0, 2, device=t['labels'].device)
        wm = slice(ns, B) if ns < B else None
        net = model
        if world > 1 and args.no_graph:
            from sound_event_detection_transformer_amd.engine import train_stream
            with torch.cuda.stream(train_stream(dev)):
                net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev.index], broadcast_buffers=False,
                                                                gradient_as_bucket_view=True)
        graphed = not (args.no_graph or args.model_only)
        if graphed:
            g, err = None, None
            try:
                if args.force_graph_fallback:
                    raise RuntimeError('--force-graph-fallback (readiness test)')
                g = GraphedTrainStep(net, criterion, opt, x, targets, wm, slice(ns), max_norm=0.1, device_matching=not args.host_matching,
                                     overlap_allreduce=not args.no_overlap, mix_up_ratio=mix, dp_cuts=args.dp_cuts,
                                     grad_dtype=torch.bfloat16 if args.bf16_buckets else None, async_wgrad=args.async_wgrad)
            except Exception as e:                      # noqa: BLE001
                if world == 1:
                    raise
                err = repr(e)[:300]
                print(f'bench.py: rank {rank}: graphed data-parallel step failed: {err}', file=sys.stderr)
            if world > 1:
                # every rank must take the same path, and must learn the others' outcome WITHOUT another collective (see
                # agree_out_of_band): all built -> captured schedule; none built (a deterministic failure of the capture - its first
                # execution on real multi-GPU hardware is the driver's scaling run) -> all ranks fall back to the eager step under
                # torch DDP rather than lose the measurement; mixed -> exit 3
                if not agree_out_of_band(g is not None, rank, world, 'graphed_dp_step'):
                    g = None
                    graphed = False
                    extras['graph_fallback'] = err or 'another rank failed to build the graphed data-parallel step'
                    from sound_event_detection_transformer_amd.engine import train_stream, broadcast_parameters
                    if torch.distributed.get_backend() == 'nccl':
                        with torch.cuda.stream(train_stream(dev)):
                            net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev.index], broadcast_buffers=False,
                                                                            gradient_as_bucket_view=True)
                    else:      # gloo moves no GPU tensors in this image: the eager step averages its flat gradient buffer itself
                        broadcast_parameters(model)
                        extras['eager_allreduce'] = True
        if graphed and args.loader:
            # input side in the loop: the batch is HOST-resident raw mel amplitudes per clip, as the reference's
            # DataLoader hands them over (data_utils/DataLoad.py:160-180 before its transform chain); per step: pinned staging + ONE
            # H2D copy on the prefetcher's copy stream (data_utils/DataLoad.py:304-336), the BoxTransforms chain of train_sedt.py:194-207
            # (ApplyLog, PadOrTrunc, TimeMask, FreqMask, FreqShift, Normalize) as sedt_box_transform on that stream, np.random draws in
            # the reference's order on the host, then the graphed step on what the prefetcher hands over
            import numpy as np
            from sound_event_detection_transformer_amd.utilities.prefetch import DevicePrefetcher
            from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
            from sound_event_detection_transformer_amd.utilities.synthetic import SEMI_SCALER
            rng = np.random.RandomState(seed)
            pool = [([np.power(10.0, 0.5 * rng.randn(T, 64)).astype(np.float32) for _ in range(B)],
                     synthetic_batch(B, T, seed + 10 * i, torch.device('cpu'))[1]) for i in range(4)]
            for _, tg in pool:
                for t in tg[ns:]:
                    t['boxes'] = torch.zeros(0, 2)

            def endless():
                i = 0
                while True:
                    yield pool[i % len(pool)]
                    i += 1
            tf = DeviceBoxTransform(T, np.full(64, SEMI_SCALER[0]), np.full(64, SEMI_SCALER[1]), time_mask=True, freq_mask=True,
                                    freq_shift=True, device=dev)
            pf = DevicePrefetcher(endless(), dev, transform=tf, targets_to_device=False)
            extras['stepper'] = g
            extras['loader'] = "host raw mel clips -> pinned staging -> H2D (copy stream) -> sedt_box_transform(time/freq mask, shift) -> step"

            def step():
                xb, tb = pf.next()
                return g(xb, tb)
        elif graphed:
            extras['stepper'] = g

            def step():
                return g(x, targets)
        elif args.model_only:
            def step():
                o = net(x)
                loss = o['pred_logits'].square().mean() + o['pred_boxes'].mean() + o['at'].mean() + \
                    sum(a['pred_logits'].square().mean() + a['pred_boxes'].mean() for a in o['aux_outputs'])
                loss.backward()
                opt.zero_grad(set_to_none=True)
                return o
        else:
            def step():
                return train_step(net, criterion, opt, x, targets, wm, slice(ns), max_norm=0.1, mix_up_ratio=mix,
                                  allreduce=bool(extras.get('eager_allreduce')))
        extras.update(model=model, criterion=criterion, opt=opt, x=x, targets=targets, wm=wm, ns=ns, net=net)
        if graphed:
            def local_step():                     # the same step without the data-parallel schedule (exposed_comm)
                loc = GraphedTrainStep(net, criterion, opt, x, targets, wm, slice(ns), max_norm=0.1, data_parallel=False, mix_up_ratio=mix)
                return lambda: loc(x, targets)
            extras['local_step'] = local_step
        what = (f"{'URBAN-SED' if cfg == 'c2' else 'DCASE2019'} SEDT enc_layers={E} dec_at num_queries={Q} B={B}/GPU"
                f"{'' if cfg == 'c2' else f' ({ns} strong + {B - ns} weak)'}, 10 s @ 64-mel (B,1,{T},64), full train step: fwd + "
                f"Hungarian matching ({'host' if (args.host_matching or not graphed) else 'device'}) + SetCriterion + bwd + clip 0.1 + "
                f"AdamW, dropout 0.1" + (f", mixup {mix} inside the step" if mix else "") + (" [model-only timing]" if args.model_only else "")
                + (" [INPUT SIDE IN THE LOOP: " + extras['loader'] + "]" if extras.get('loader') else ""))
        return step, B, FLOP_PER_CLIP[cfg] * B, what, graphed, extras
    if cfg == 'eval':
        from sound_event_detection_transformer_amd.engine import GraphedPredictStep
        B = args.batch or 64
        model, criterion, post = build_model(default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.1))
        model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
        model.to(dev).eval()
        criterion.to(dev)
        x, targets = synthetic_batch(B, 500, seed, dev)
        for t in targets:
            t['orig_size'] = torch.tensor(10.0, device=dev)
        g = GraphedPredictStep(model, criterion, post['bbox'], x, targets, fusion_strategy=(1,))
        extras.update(stepper=g, model=model)

        def step():
            return g(x, targets)
        what = (f"validation body of engine.get_sedt_predictions, URBAN-SED SEDT enc_layers=3 dec_at num_queries=10 B={B}/GPU: no-grad "
                f"forward + device matching + SetCriterion (logged losses) + audio tags + PostProcess (fusion strategy 1), one HIP graph")
        return step, B, FLOP_PER_CLIP['eval'] * B, what, True, extras
    if cfg == 'c4':
        B, P = args.batch or 200, 10
        model, criterion, _ = build_model(default_args(enc_layers=6, num_queries=20, dec_at=False, self_sup=True, lr_backbone=0.0,
                                                       dropout=0.1))
        model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
        model.to(dev).train()
        criterion.to(dev)
        opt = build_optimizer(model)
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(B, 1, 496, 64, generator=gen).to(dev)
        patches = torch.randn(B, P, 1, 128, 64, generator=gen).to(dev)
        targets = []
        for _ in range(B):                       # one box per patch, label 0 (DataLoad.py:57-77)
            l = (torch.randn(P, generator=gen) * 0.26 + 0.2).clamp(0.05, 0.799)
            c = l / 2 + torch.rand(P, generator=gen) * (1 - l)
            targets.append({'labels': torch.zeros(P, dtype=torch.int64), 'boxes': torch.stack([c, l], -1)})
        # (the targets stay on the host, where a loader leaves them - as for C2 / C3: TargetTables lays them out in pinned memory and sends
        #  ONE host->device copy per step; device-resident targets cost four concatenation kernels, two fills and three copies per step)
        g = GraphedTrainStep(model, criterion, opt, x, targets, slice(B), slice(B), max_norm=0.1, example_patches=patches,
                             overlap_allreduce=not args.no_overlap, dp_cuts=args.dp_cuts,
                             grad_dtype=torch.bfloat16 if args.bf16_buckets else None)
        if world > 1 and not agree_out_of_band(True, rank, world, 'graphed_dp_step'):
            os._exit(3)
        extras.update(stepper=g, model=model, targets=targets)

        def step():
            return g(x, targets, patches=patches)

        def local_step():
            loc = GraphedTrainStep(model, criterion, opt, x, targets, slice(B), slice(B), max_norm=0.1, example_patches=patches,
                                   data_parallel=False)
            return lambda: loc(x, targets, patches=patches)
        extras['local_step'] = local_step
        what = (f"SP-SEDT self-sup pre-training (feature_recon, num_patches=10) enc_layers=6 num_queries=20 B={B}/GPU + {B * P} patches "
                f"(1,128,64), backbone frozen, full step: clip + patch backbone fwd, transformer fwd/bwd, device matching, "
                f"CE/L1/GIoU/feature losses, clip 0.1 + AdamW, dropout 0.1")
        return step, B, FLOP_PER_CLIP['c4'] * B, what, True, extras
    # c5
    n_s = n_w = (args.batch // 4) if args.batch else 16
    n_u = 2 * n_s
    B = n_s + n_w + n_u
    model, criterion, _ = build_model(default_args(enc_layers=6, num_queries=20, dec_at=True, dropout=0.1))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 2020))
    model.to(dev).train()
    criterion.to(dev)
    ema = EMA(model, 0.9996)
    ema.register()
    opt = build_optimizer(model)
    # both views come from raw mel amplitudes through the reference's transform chain ON THE DEVICE, inside every timed step
    # (train_ss_sedt.py:87-90 --freq_mask --time_mask; utilities/BoxTransforms.py:363-427, 454-490): teacher = ApplyLog + PadOrTrunc
    # + FreqMask + Normalize, student = the noisy copy through ApplyLog + PadOrTrunc + TimeMask + FreqMask + Normalize, np.random
    # parameters drawn per clip on the host in the reference's order
    from sound_event_detection_transformer_amd.utilities.synthetic import synthetic_semi_raw, semi_view_transforms
    raw_t, raw_s = synthetic_semi_raw(n_s + n_w, n_u, 496, seed)
    raw_t, raw_s = raw_t.to(dev), raw_s.to(dev)
    tf_t, tf_s = semi_view_transforms(496, dev)
    x_t, x_s = tf_t(raw_t), tf_s(raw_s)
    targets = synthetic_targets(B, seed + 1, 10)
    for t in targets[n_s:]:
        t['boxes'] = torch.zeros(0, 2)
    for t in targets[n_s + n_w:]:
        t['labels'] = torch.zeros(0, dtype=torch.int64)
    mix = args.mix_up_ratio if args.mix_up_ratio is not None else 0.6        # train_ss_sedt.py's recipe (README.md:134)
    if not mix:
        targets = to_dev(targets)                     # (with mix-up the targets stay on the host: its label half is host work)
    thr = torch.full((10,), 0.1, device=dev)          # (random-init teacher: a low threshold keeps pseudo events alive)
    import numpy as np
    np.random.seed(seed)
    masks = (slice(n_s), slice(n_s, n_s + n_w), slice(n_s + n_w), slice(n_s + n_w, B))
    g = GraphedSemiStep(model, ema, criterion, opt, x_t, x_s, targets, *masks, thr, mix_up_ratio=mix,
                        overlap_allreduce=not args.no_overlap, dp_cuts=args.dp_cuts,
                        grad_dtype=torch.bfloat16 if args.bf16_buckets else None)
    if world > 1 and not agree_out_of_band(True, rank, world, 'graphed_dp_step'):
        os._exit(3)
    extras.update(stepper=g, model=model)

    def views():
        tf_t(raw_t, out=x_t)
        tf_s(raw_s, out=x_s)

    def step():
        views()
        return g(x_t, x_s, targets)

    def local_step():
        loc = GraphedSemiStep(model, ema, criterion, opt, x_t, x_s, targets, *masks, thr, mix_up_ratio=mix, data_parallel=False)

        def run():
            views()
            loc(x_t, x_s, targets)
        return run
    extras['local_step'] = local_step
    what = (f"semi-supervised mean-teacher step (train_ss_sedt.py) enc_layers=6 num_queries=20 per GPU: {n_s} synthetic + {n_w} weak "
            f"labelled clips fwd/bwd, {n_u} unlabelled clips through the EMA teacher (no grad) -> device pseudo labels -> student "
            f"fwd/bwd on the augmented view (both views produced per step from raw mel amplitudes by sedt_box_transform: ApplyLog, "
            f"PadOrTrunc, FreqMask(mean), Normalize; the student's also TimeMask), one backward, clip 0.1 + AdamW + EMA update, "
            f"dropout 0.1, " +
            (f"mixup {mix} inside the step (mixup_data on the labelled clips, mixup_label_unlabel of the student view with the "
             f"pseudo labels: np.random draws + label plan on the host per step, feature mixing + label merge in the graph)"
             if mix else "mixup off"))
    return step, B, FLOP_C5_STEP_64 * B / 64.0, what, True, extras



# ---------------------------------------------------------------------------------------------------------------------
def _short_kernel_name(name):
    """'void sedt::igemm3_kernel<64, 64, 2>(SedtIgemm, unsigned, unsigned)' -> 'igemm3_kernel<64, 64, 2>'"""
    n = name.strip()
    if n.startswith('_ZN4sedt'):                 # a mangled name the demangler could not take (DF16b = __bf16): the length-prefixed identifier
        import re
        m = re.match(r'_ZN4sedt(\d+)', n)
        if m:
            k = int(m.group(1))
            ident = n[len(m.group(0)):len(m.group(0)) + k]
            return ident + ('<bf16>' if 'DF16b' in n else '<float>' if 'IfL' in n or 'IfE' in n else '')
    if n.startswith('void '):
        n = n[5:]
    depth, cut = 0, len(n)
    for i, ch in enumerate(n):
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            cut = i
            break
    n = n[:cut].strip()
    return n.replace('sedt::', '').replace('(anonymous namespace)::', '')


def _demangle(names):
    mangled = [n for n in names if n.startswith('_Z')]
    if not mangled:
        return {}
    for tool in ('/opt/rocm/lib/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt', 'c++filt'):
        try:
            r = subprocess.run([tool], input='\n'.join(mangled), capture_output=True, text=True, timeout=30)
            out = r.stdout.split('\n')
            if r.returncode == 0 and len(out) >= len(mangled):
                return dict(zip(mangled, out))
        except Exception:                            # noqa: BLE001
            continue
    return {}


def kernel_times(step, reps=3):
    """{short kernel name: [us per step, launches per step]} of `reps` further steps, from the activity records the torch profiler
    collects in THIS process (every kernel dispatch of the replayed graphs, whoever launched it)"""
    import torch
    from torch.profiler import profile, ProfilerActivity
    from torch.autograd import DeviceType
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
    raw = {}
    for e in prof.events():
        if e.device_type != DeviceType.CUDA:
            continue
        dur = e.time_range.elapsed_us() if hasattr(e, 'time_range') else float(getattr(e, 'device_time', 0.0))
        r = raw.setdefault(e.name, [0.0, 0])
        r[0] += dur
        r[1] += 1
    dem = _demangle(list(raw))
    out = {}
    for name, (us, n) in raw.items():
        k = _short_kernel_name(dem.get(name, name))
        r = out.setdefault(k, [0.0, 0.0])
        r[0] += us / reps
        r[1] += n / reps
    return out


def gemm_algorithmic(rec_entry, es):
    """(flop, bytes) one recorded GEMM launch HAS to do / move: 2 M N K, and every operand once - gathered input pixels (not the im2col
    matrix), weights, output (+ residual / ReLU-mask operands the epilogue reads); a weight gradient reads dY and X once and leaves
    4 B per weight (its split-K slabs are overhead, not algorithm)"""
    a, _, (M, N, K, trans, conv), _, _ = rec_entry
    flop = 2.0 * M * N * K
    if trans:                      # dW[M = Cout][N = taps*Cin] over K pixels: A = dY [K][M], B = X (input pixels x Cin)
        rows_b = K if not conv else (K // max(a.Ho * a.Wo, 1)) * a.Hi * a.Wi
        nbytes = (K * M + rows_b * (a.Ci if conv else N)) * es + 4.0 * M * N
    else:
        rows_a = M if not conv else ((M + a.Ho * a.Wo - 1) // (a.Ho * a.Wo)) * a.Hi * a.Wi
        nbytes = (rows_a * (a.Ci if conv else K) + N * K) * es + M * N * (4 if a.out_f32 else es)
        if a.res:
            nbytes += M * N * es
        if a.mask:
            nbytes += M * N / 8.0 if a.mask_bits else M * N * es
        if a.bits_out:
            nbytes += M * N / 8.0
    return flop, nbytes


def family_report(step, rec, dtype, n_params, step_ms):
    """roofline.families: every kernel instance of the measured step with its time (in-process kernel trace of three further steps),
    and - for the GEMM families, whose shapes one recorded eager step gives - algorithmic flops and bytes, the roofline that bounds it
    (mfma when flops / peak > bytes / HBM peak) and the fraction of that roofline it reaches"""
    import ctypes
    from sound_event_detection_transformer_amd import lib as L_
    times = kernel_times(step)
    es = 2 if dtype == 'bf16' else 4
    peak = MFMA_PEAK[dtype]
    lib = L_.load()
    buf = ctypes.create_string_buffer(128)
    work, unmatched = {}, 0

    def match(label):
        if label in times:
            return label
        c = [k for k in times if k.startswith(label)]
        return c[0] if len(c) == 1 else None
    alg_gemm_bytes = 0.0
    for ent in rec or []:
        a, dt_, _, _, hint = ent
        flop, nb = gemm_algorithmic(ent, es)
        alg_gemm_bytes += nb
        label, share = None, 1.0
        if hint == 'conv3x3_c64_kernel':
            label = match('conv3x3_c64_kernel')
        elif isinstance(hint, tuple) and hint[0] == 'group':
            # the measured step runs this problem inside a grouped launch (sedt_igemm_group_describe gave its kernel instance at record
            # time), possibly in a form that executes a share of the recorded problem's flops: layer4's dilated 3x3 as two column
            # halves walks 6 of 9 taps, a stride-2 input gradient by output parity a quarter of the transposed walk
            label, share = (match(hint[1]) if hint[1] else None), hint[2]
        if label is None:
            if lib.sedt_igemm_describe(ctypes.byref(a), dt_, 1 if hint == 'wgrad_group' else 0, buf, 128) == 0:
                label = match(buf.value.decode())
        if label is None:
            unmatched += 1
            continue
        w = work.setdefault(label, [0.0, 0.0, 0.0])
        w[0] += flop * share             # flops the launch executes
        w[1] += nb
        w[2] += flop                     # flops of the convolution / linear it implements (SURVEY 8d counts these)
    # the fused Bottleneck launches of the recorded step (ops.PROFILE_FUSED: kernel-name prefix, flop, bytes)
    from sound_event_detection_transformer_amd import ops as ops_
    for name, flop, nb in ops_.PROFILE_FUSED:
        alg_gemm_bytes += nb
        label = match(name)
        if label is None:
            unmatched += 1
            continue
        w = work.setdefault(label, [0.0, 0.0, 0.0])
        w[0] += flop
        w[1] += nb
        w[2] += flop
    # the streaming kernels whose byte counts follow from the parameter count alone
    for k in times:
        if k.startswith('multi_adamw_kernel'):
            work[k] = [0.0, 28.0 * n_params, 0.0]
        elif k.startswith('multi_sumsq_kernel'):
            work[k] = [0.0, 4.0 * n_params, 0.0]
    fams = []
    for k, (us, n) in sorted(times.items(), key=lambda kv: -kv[1][0]):
        row = {"kernel": k, "launches": round(n, 1), "us": round(us, 1), "share": round(us / (step_ms * 1e3), 4)}
        if k in work:
            flop, nb, flop_alg = work[k]
            t = us * 1e-6
            t_m, t_h = flop / peak, nb / HBM_PEAK
            row.update(flop=flop, bytes=nb)
            if abs(flop_alg - flop) > 1e-6 * max(flop_alg, 1.0):
                row.update(flop_algorithmic=flop_alg)        # (the row's achieved / frac are over the flops it EXECUTES)
            if t_m >= t_h:
                row.update(bound="mfma", achieved=round(flop / t / 1e12, 1), unit="TFLOP/s", peak=peak / 1e12, frac=round(t_m / t, 4))
            else:
                row.update(bound="hbm", achieved=round(nb / t / 1e9, 1), unit="GB/s", peak=HBM_PEAK / 1e9, frac=round(t_h / t, 4))
        fams.append(row)
    # a GEMM kernel row with time but no flop record means the join above lost its problems: counted as unmatched, listed by name
    no_flops = [r["kernel"] for r in fams if "flop" not in r and rec is not None and
                any(r["kernel"].startswith(pfx) for pfx in ('igemm', 'wgrad3', 'wgrad4', 'conv3x3', 'bneck'))]
    unmatched += len(no_flops)
    small = [r for r in fams if r["share"] < 0.004 and "flop" not in r]
    keep = [r for r in fams if not (r["share"] < 0.004 and "flop" not in r)]
    if small:
        keep.append({"kernel": f"{len(small)} further kernels below 0.4 % of the step each", "launches": round(sum(r["launches"] for r in small), 1),
                     "us": round(sum(r["us"] for r in small), 1), "share": round(sum(r["share"] for r in small), 4)})
    total_us = sum(v[0] for v in times.values())
    # algorithmic bytes of one step AS IT IS LAUNCHED (no cross-launch fusion assumed): every GEMM operand once (above), the optimizer's
    # 28 B per trainable parameter + 4 B for the norm, the two packed bf16 weight layouts (4 B read + 2 x 2 B written per parameter)
    alg = alg_gemm_bytes + (28.0 + 4.0 + 8.0) * n_params
    return {"families": keep, "kernel_time_us": round(total_us, 1), "unmatched_gemm_records": unmatched, "gemm_rows_without_flops": no_flops,
            "algorithmic_bytes": round(alg), "algorithmic_bytes_gemm_operands": round(alg_gemm_bytes)}


def in_step_rows(prefixes):
    """what the named kernels do INSIDE the measured step, from the newest committed per-kernel PMC table (profiles/rNN_step_c2.csv:
    launches per step, summed microseconds, FETCH x2 + WRITE bytes): 'N launches, T us, X MB -> Y GB/s (file)'"""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_step_c2.csv')))
    if not files:
        return 'no per-kernel PMC table under profiles/'
    n = us = kb = 0.0
    with open(files[-1]) as f:
        for r in csv.DictReader(f):
            if any(pfx in r['kernel'] for pfx in prefixes):
                n += float(r['launches_per_step'])
                us += float(r['time_us'])
                kb += float(r['FETCH_KB_x2'] or 0) + float(r['WRITE_KB'] or 0)
    if not us:
        return 'not in ' + os.path.basename(files[-1])
    return '%d launches, %.0f us, %.0f MB moved = %.0f GB/s fabric-side (%s; the launches sit on the ~4.7 us launch floor)' % (
        n, us, kb * 1.024e-3, kb * 1024 / us / 1e3, os.path.basename(files[-1]))


def kernel_report(dtype, dev):
    """north_star's per-kernel figures, timed live with HIP events at the C2 shapes: MFMA utilisation of the attention core,
    the encoder self-attention block, the FFN GEMMs and the layer4 3x3 conv; HBM GB/s of LayerNorm and the fused AdamW."""
    import torch
    from sound_event_detection_transformer_amd import ops, lib as L
    from sound_event_detection_transformer_amd.optim import FusedAdamW
    dt = L.BF16 if dtype == 'bf16' else L.F32
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    es = 2 if dtype == 'bf16' else 4
    peak = MFMA_PEAK[dtype]
    B, S, E, H, FF = 64, 128, 256, 8, 2048
    M = B * S
    g = torch.Generator().manual_seed(1)

    def rnd(*shape, scale=1.0, dtype_=None):
        return (torch.randn(*shape, generator=g) * scale).to(device=dev, dtype=dtype_ or td)

    def timeit(fn, reps=20, post=None):
        """device time of fn's launches as they run inside the step: captured into a HIP graph (no host launch overhead
        between them), `reps` copies per replay, HIP events around the replays"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_):
            for _ in range(reps):
                fn()
        if post is not None:
            post()                                  # (e.g. FusedAdamW.flush_uploads: table uploads are not part of a capture)
        g_.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            g_.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (3 * reps) * 1e-3
    out = []
    x, pos = rnd(M, E), rnd(M, E, scale=0.5)
    gam, bet = rnd(E, dtype_=torch.float32), rnd(E, dtype_=torch.float32)
    w_in, b_in = rnd(3 * E, E, scale=0.06), rnd(3 * E, dtype_=torch.float32)
    w_o, b_o = rnd(E, E, scale=0.06), rnd(E, dtype_=torch.float32)
    w1, b1 = rnd(FF, E, scale=0.06), rnd(FF, dtype_=torch.float32)
    w2, b2 = rnd(E, FF, scale=0.02), rnd(E, dtype_=torch.float32)
    q, k, v = rnd(M, E), rnd(M, E), rnd(M, E)

    def mf(name, flop, t, note=''):
        out.append({"kernel": name, "us": round(t * 1e6, 2), "achieved": round(flop / t / 1e12, 1), "unit": "TFLOP/s",
                    "peak": peak / 1e12, "frac": round(flop / t / peak, 4), "bound": "mfma", "note": note})

    def hb(name, nbytes, t, note=''):
        out.append({"kernel": name, "us": round(t * 1e6, 2), "achieved": round(nbytes / t / 1e9, 1), "unit": "GB/s",
                    "peak": HBM_PEAK / 1e9, "frac": round(nbytes / t / HBM_PEAK, 4), "bound": "hbm", "note": note})
    t = timeit(lambda: ops.attention_fwd(dt, q, k, v, B, H, S, S, None, None, 0.1, 7, None))
    mf("attention core fwd (sedt_attention_fwd: 512 heads x 128x128x32, dropout 0.1)", 4.0 * S * S * 32 * B * H, t)

    def block():
        xn, xnp, _, _ = ops.layernorm_fwd(dt, x, gam, bet, add_t=pos)
        qk, vv = ops.linear_group(dt, [(xnp, w_in[:2 * E], dict(bias=b_in[:2 * E])), (xn, w_in[2 * E:], dict(bias=b_in[2 * E:]))])
        ctx, _ = ops.attention_fwd(dt, qk[:, :E], qk[:, E:], vv, B, H, S, S, None, None, 0.1, 7, None)
        return ops.linear(dt, ctx, w_o, bias=b_o, drop_p=0.1, seed=3, res=x, ldr=x.stride(0))
    t = timeit(block)
    mf("encoder self-attn block fwd (LN1 + pos -> QKV -> attention -> out-proj + dropout + residual)", 83.9e6 * B, t,
       "4 launches (LayerNorm, grouped QK|V projection, attention core, out-proj); north_star target >= 0.60")
    xn0, xnp0, _, _ = ops.layernorm_fwd(dt, x, gam, bet, add_t=pos)
    t = timeit(lambda: ops.linear_group(dt, [(xnp0, w_in[:2 * E], dict(bias=b_in[:2 * E])), (xn0, w_in[2 * E:], dict(bias=b_in[2 * E:]))]))
    mf("  QK | V projections (one grouped launch, 8192 x 256 x 768)", 2.0 * M * E * 3 * E, t)
    t = timeit(lambda: ops.linear(dt, q, w_o, bias=b_o, drop_p=0.1, seed=3, res=x, ldr=x.stride(0)))
    mf("  out-proj + dropout + residual (8192 x 256 x 256)", 2.0 * M * E * E, t)

    def ffn():
        h = ops.linear(dt, x, w1, bias=b1, act=L.ACT_RELU, drop_p=0.1, seed=5)
        return ops.linear(dt, h, w2, bias=b2, drop_p=0.1, seed=6, res=x, ldr=x.stride(0))
    t = timeit(ffn)
    mf("encoder FFN fwd (linear1 + ReLU + dropout, linear2 + dropout + residual)", 2.0 * 2 * M * E * FF, t)
    # the whole pre-norm encoder layer: the per-op chain (seven launches) against the x-stationary slab kernels (two launches)
    gam2, bet2 = rnd(E, dtype_=torch.float32), rnd(E, dtype_=torch.float32)

    def layer_chain():
        x1 = block()
        x1n, _, _, _ = ops.layernorm_fwd(dt, x1, gam2, bet2)
        h = ops.linear(dt, x1n, w1, bias=b1, act=L.ACT_RELU, drop_p=0.1, seed=5)
        return ops.linear(dt, h, w2, bias=b2, drop_p=0.1, seed=6, res=x1, ldr=x1.stride(0))
    layer_flop = 352.3e6 * B                                     # FFN 268.4 + QKV / out 67.1 + attention 16.8 MFLOP per clip
    t = timeit(layer_chain)
    mf("encoder layer fwd, per-op chain (LN1, QK|V, attention, out-proj, LN2, linear1, linear2: 7 launches)", layer_flop, t)
    if ops.encoder_slab_ok(dt, E, H, S, FF, None):
        from sound_event_detection_transformer_amd import packing
        masters = [torch.nn.Parameter(w.float()) for w in (w_in, w_o, w1, w2)]
        plan = packing.PackPlan(dt, dev, [], masters, (), masters)
        plan.run()
        torch.cuda.synchronize()
        fr = [plan.frag_table[m.data_ptr()][0] for m in masters]

        def slab_layer(train):
            qk_, v_, _ = ops.encoder_qkv_fwd(x, pos, gam, bet, fr[0], b_in, B, S, train=train)
            return ops.encoder_attn_ffn_fwd(x, qk_, v_, None, fr[1], b_o, gam2, bet2, fr[2], b1, fr[3], b2, B, S, FF, 0.1, (7, 3, 5, 6), None,
                                            train=train)
        t = timeit(lambda: slab_layer(True))
        mf("encoder layer fwd, slab kernels (sedt_encoder_qkv_fwd + sedt_encoder_attn_ffn_fwd: 2 launches), training form", layer_flop, t,
           "a workgroup owns 32 tokens, activations stay in LDS, only weights stream L2 -> registers (csrc/slab.h); by-products for the backward written")
        t = timeit(lambda: slab_layer(False))
        mf("encoder layer fwd, slab kernels, no-grad form (teacher / eval)", layer_flop, t)
        t = timeit(lambda: ops.encoder_qkv_fwd(x, pos, gam, bet, fr[0], b_in, B, S, train=True))
        mf("  sedt_encoder_qkv_fwd alone (LN1 + pos, Q|K|V projections; 393 KB of weights per 32-token slab)", 2.0 * M * E * 3 * E, t)
        qk0, v0, _ = ops.encoder_qkv_fwd(x, pos, gam, bet, fr[0], b_in, B, S, train=False)
        t = timeit(lambda: ops.encoder_attn_ffn_fwd(x, qk0, v0, None, fr[1], b_o, gam2, bet2, fr[2], b1, fr[3], b2, B, S, FF, 0.1, (7, 3, 5, 6),
                                                    None, train=True))
        mf("  sedt_encoder_attn_ffn_fwd alone (attention, out-proj, LN2, FFN pair; 2.23 MB of weights per slab)",
           layer_flop - 2.0 * M * E * 3 * E, t)
        t = timeit(lambda: plan.run())
        hb("weight packing of one encoder layer incl. the fragment-major forms (multi_pack + pack_frag)", 1.31e6 * (4 + 4 * 2), t)
    xin = rnd(B * 32 * 4, 512)
    wc = rnd(512, 9 * 512, scale=0.02)
    sc, bi = rnd(512, dtype_=torch.float32), rnd(512, dtype_=torch.float32)
    geo = ops.ConvGeom(32, 4, 512, 512, 3, 1, 2, 2)
    t = timeit(lambda: ops.conv_fwd(dt, xin, B, geo, wc, scale=sc, bias=bi, act=L.ACT_RELU))
    mf("layer4 3x3 dilated conv fwd (implicit GEMM 8192 x 512 x 4608, FrozenBN + ReLU epilogue)", 2.0 * M * 512 * 4608, t)
    # layer1 conv2: the direct 3x3 kernel (conv3x3_c64.hip) and its input gradient
    g1 = ops.ConvGeom(125, 16, 64, 64, 3, 1, 1, 1)
    x1 = rnd(B * 125 * 16, 64)
    w1c = rnd(64, 64, 3, 3, scale=0.04, dtype_=torch.float32)
    sc1, bi1 = rnd(64, dtype_=torch.float32).abs() + 0.5, rnd(64, dtype_=torch.float32)
    wf1, wb1 = ops.pack_conv(dt, w1c, sc1)
    y1 = torch.empty_like(x1)
    t = timeit(lambda: ops.conv_fwd(dt, x1, B, g1, wf1, out=y1, scale=sc1, bias=bi1, act=L.ACT_RELU))
    mf("layer1 3x3 conv fwd (direct kernel, 128000 x 64 x 576, FrozenBN + ReLU)", 2.0 * B * 125 * 16 * 64 * 576, t,
       "halo tile + all nine taps in LDS; the implicit GEMM it replaced: 25 us")
    t = timeit(lambda: ops.conv_dgrad(dt, x1, B, g1, wb1, out=y1, mask=x1, ldm=64))
    mf("layer1 3x3 conv input gradient (direct kernel, taps flipped, ReLU mask)", 2.0 * B * 125 * 16 * 64 * 576, t,
       "the implicit GEMM it replaced: 37 us")
    # the fused Bottlenecks (bneck.hip, bneck3.hip): an identity block of layer1 / layer2 / layer3 in one launch each way
    if dtype == 'bf16':
        from sound_event_detection_transformer_amd import packing
        from sound_event_detection_transformer_amd.sedt.backbone import ResNet50Body
        body = ResNet50Body(True).to(dev)
        for name, layer, Hm, Wm in (('layer1', body.layer1, 125, 16), ('layer2', body.layer2, 63, 8), ('layer3', body.layer3, 32, 4)):
            blk = layer[1]
            if not ops.bneck_ok(dt, blk.cfg, Wm, B, Hm):
                continue
            ws = (blk.conv1.weight, blk.conv2.weight, blk.conv3.weight)
            plan = packing.PackPlan(dt, dev, [(blk.conv1.weight, blk.bn1.tensors()), (blk.conv2.weight, blk.bn2.tensors()),
                                              (blk.conv3.weight, blk.bn3.tensors())], [], (), (), list(ws))
            plan.run()
            torch.cuda.synchronize()
            cf = [plan.conv_frag_table[w.data_ptr()] for w in ws]
            sb = [plan.table[w.data_ptr()][2:] for w in ws]
            Cb, Pb = blk.cfg.cin, blk.cfg.planes
            Mb = B * Hm * Wm
            xb_ = rnd(Mb, Cb).relu()
            gyb = rnd(Mb, Cb)
            trainable = name != 'layer1'                      # (layer1 is frozen in the reference: sign bits only; layer2 / 3 also keep a, b)
            _, _, _, bits_, ab_, bb_ = ops.bneck_fwd(xb_, B, Hm, Wm, [c[0] for c in cf], sb, want_ab=False)
            flop = 2.0 * Mb * (2 * Cb * Pb + 9 * Pb * Pb)
            by_f = Mb * (2 * Cb * 2 + Cb // 8 + 2 * (Pb // 8) + (2 * Pb * 2 if trainable else 0))
            by_b = Mb * (2 * Cb * 2 + Cb // 8 + 2 * (Pb // 8) + (2 * Pb * 2 if trainable else 0))
            wbytes = 2.0 * (2 * Cb * Pb + 9 * Pb * Pb)
            note = ("HBM-bound: x in, y out, sign bits%s; %d KB of weights stream from L2 per strip" % (' + a, b' if trainable else '', wbytes // 1024))
            t = timeit(lambda: ops.bneck_fwd(xb_, B, Hm, Wm, [c[0] for c in cf], sb, want_ab=trainable))
            hb("%s identity Bottleneck fwd, fused (1 launch; training form), %.1f GFLOP" % (name, flop / 1e9), by_f, t, note)
            t = timeit(lambda: ops.bneck_fwd(xb_, B, Hm, Wm, [c[0] for c in cf], sb, train=False))
            hb("%s identity Bottleneck fwd, fused, no-grad form (teacher / eval / frozen backbone)" % name, Mb * 2 * Cb * 2, t)
            t = timeit(lambda: ops.bneck_bwd(gyb, B, Hm, Wm, [c[1] for c in cf], ab_, bb_, bits_, want_g=trainable))
            hb("%s identity Bottleneck input-gradient chain, fused (1 launch)" % name, by_b, t,
               "masks = the sign bits the forward wrote" + ("; gb, ga out for the weight-gradient GEMMs" if trainable else ""))
            del plan
    # the stem in one launch each way (stem.hip): bytes = f32 input + pooled bf16 output + argmax bytes
    if ops.stem_pool_ok(dt, 64):
        xs = torch.randn(B, 1, 500, 64, device=dev)
        w0, b0 = torch.randn(3, 1, 1, 1, device=dev), torch.randn(3, device=dev)
        ws1 = torch.randn(64, 3, 7, 7, device=dev) / 12
        wcat = ops.stem_prep(dt, w0, b0, ws1)
        pool, idx, Hp, Wp = ops.stem_pool_fwd(xs, wcat, sc1, bi1, B, 500, 64)
        gpool = torch.randn_like(pool)
        t = timeit(lambda: ops.stem_pool_fwd(xs, wcat, sc1, bi1, B, 500, 64))
        hb("stem forward, one launch (conv0 o conv1 7x7/s2 o FrozenBN o ReLU o max-pool)", xs.numel() * 4.0 + pool.numel() * 3.0, t,
           "VALU-bound (epilogue + pooling), not HBM-bound; the im2col -> GEMM -> pool chain it replaced: 110 us")
        t = timeit(lambda: ops.stem_pool_wgrad(xs, gpool, idx, pool, sc1, B, 500, 64))
        hb("stem backward, one launch + reduce (conv0 gradients from the pooled gradient)", xs.numel() * 4.0 + pool.numel() * 5.0, t,
           "the max-pool backward -> weight-gradient GEMM chain it replaced: 122 us")
    # LayerNorm against the HBM roofline, honestly: the launches of one capture rotate over NBUF distinct input / output pairs
    # (>= 512 MB in total, twice the 256 MB Infinity Cache), so no launch finds its rows on the die; beside it the back-to-back replay on ONE
    # 8 MB pair (an L2 / Infinity-Cache figure, labelled so) and what the step's own LayerNorm launches reach (rocprofv3 PMC table)
    NBUF = max(2, int(math.ceil(512e6 / (2.0 * M * E * es))))
    xs_ln = [torch.randn(M, E, device=dev).to(td) for _ in range(NBUF)]
    ys_ln = [(torch.empty_like(xs_ln[0]), torch.empty(M, device=dev), torch.empty(M, device=dev)) for _ in range(NBUF)]

    def ln_rotate():
        for i in range(NBUF):
            ops.layernorm_fwd(dt, xs_ln[i], gam, bet, out=ys_ln[i])
    t = timeit(ln_rotate, reps=1) / NBUF
    in_step = in_step_rows(('ln_fwd_kernel', 'ln_bwd_kernel'))
    hb("LayerNorm fwd 8192 x 256 (sedt_layernorm_fwd), %d distinct buffer pairs = %.0f MB per pass: every row comes from HBM" % (NBUF, NBUF * 2.0 * M * E * es / 1e6),
       2.0 * M * E * es, t, "in the step: " + in_step)
    del xs_ln, ys_ln
    t = timeit(lambda: ops.layernorm_fwd(dt, x, gam, bet))
    hb("LayerNorm fwd 8192 x 256, back-to-back replays on ONE 8 MB buffer pair (an L2 / Infinity-Cache rate, not an HBM figure)", 2.0 * M * E * es, t)
    if dt == L.BF16:
        # ---- round 5: zero-tap elimination (the same problem with the plain nine-tap gather beside it) and the parity-grade bf16x3 pieces
        def ab(flag, fn):
            res = []
            for on in (True, False):
                keep = getattr(ops, flag)
                setattr(ops, flag, on)
                try:
                    res.append(timeit(fn))
                finally:
                    setattr(ops, flag, keep)
            return res
        C4_ = 512
        g4 = ops.ConvGeom(32, 4, C4_, C4_, 3, 1, 2, 2)
        x4, w4 = rnd(B * 128, C4_), torch.randn(C4_, C4_, 3, 3, device=dev) / 68
        sc4, bi4 = torch.ones(C4_, device=dev), torch.zeros(C4_, device=dev)
        wf4, wb4 = ops.pack_conv(dt, w4, bnscale=sc4)
        t1, t0 = ab('DIL_HALVES', lambda: ops.conv_fwd(dt, x4, B, g4, wf4, scale=sc4, bias=bi4, act=L.ACT_RELU))
        mf("layer4 dilated 3x3 fwd by column halves (2 x 6-tap problems, one grouped 128x128 launch; useful flops = 2/3 of the 9-tap walk)",
           2.0 * B * 128 * C4_ * 6 * C4_, t1, "the plain nine-tap gather: %.1f us" % (t0 * 1e6))
        g3 = ops.ConvGeom(63, 8, 256, 256, 3, 2, 1, 1)
        w3 = torch.randn(256, 256, 3, 3, device=dev) / 48
        _, wb3 = ops.pack_conv(dt, w3)
        dy3 = rnd(B * g3.Ho * g3.Wo, 256)
        t1, t0 = ab('S2_PARITY', lambda: ops.conv_dgrad(dt, dy3, B, g3, wb3))
        mf("layer3 block 0 stride-2 3x3 input gradient by output parity (4 grouped problems; useful flops = 1/4 of the transposed gather's)",
           2.0 * B * 63 * 8 * 256 * 9 * 256 / 4, t1, "the transposed nine-tap gather: %.1f us" % (t0 * 1e6))
        # bf16x3: f32 tensors, one bf16 GEMM over the tripled contraction; priced against a third of the bf16 peak (three MFMAs per product)
        xf, wf32 = torch.randn(M, FF, device=dev), torch.randn(E, FF, device=dev) / 45
        keep3 = L.GEMM_X3
        L.GEMM_X3 = True
        try:
            def x3lin():
                ops.x3_cache_clear()
                return ops.linear(L.F32, xf, wf32)
            t = timeit(x3lin)
            out.append({"kernel": "bf16x3 linear 8192 x 256 x 2048 (split pass + ONE bf16 GEMM over K' = 6144, f32 epilogue)", "us": round(t * 1e6, 2),
                        "achieved": round(2.0 * M * E * FF / t / 1e12, 1), "unit": "TFLOP/s (f32-grade products)", "peak": round(peak / 3e12, 1),
                        "frac": round(2.0 * M * E * FF / t / (peak / 3), 4), "bound": "mfma",
                        "note": "peak = a third of the dense bf16 peak: hi.hi + lo.hi + hi.lo"})
            qf, kf, vf = torch.randn(M, E, device=dev), torch.randn(M, E, device=dev), torch.randn(M, E, device=dev)
            t = timeit(lambda: ops.attention_fwd(L.F32, qf, kf, vf, B, H, S, S, None, None, 0.1, 7, None))
            out.append({"kernel": "f32 attention core fwd on v_mfma_f32_32x32x2_f32 (512 heads x 128x128x32, dropout 0.1)", "us": round(t * 1e6, 2),
                        "achieved": round(4.0 * S * S * 32 * B * H / t / 1e12, 1), "unit": "TFLOP/s", "peak": MFMA_PEAK['f32'] / 1e12,
                        "frac": round(4.0 * S * S * 32 * B * H / t / MFMA_PEAK['f32'], 4), "bound": "mfma", "note": "exact f32 matrix rate (157 TF)"})
            def split_only():
                ops.x3_cache_clear()
                return ops._split3([(xf, 0, M, FF, FF, 0)])
            t = timeit(split_only)
            hb("bf16x3 operand image 8192 x 2048 (sedt_split3: f32 -> [hi | lo])", 8.0 * M * FF, t, "4 B read + 4 B written per element")
        finally:
            L.GEMM_X3 = keep3
            ops.x3_cache_clear()
    n = 32579869
    p = torch.nn.Parameter(torch.zeros(n, device=dev))
    p.grad = torch.full((n,), 1e-3, device=dev)
    opt = FusedAdamW([p], lr=1e-4, weight_decay=1e-4)
    opt.step(max_norm=0.1)
    t = timeit(lambda: opt.step(max_norm=0.1), reps=5, post=opt.flush_uploads)
    hb("clip + AdamW over 32.58 M parameters (sedt_multi_sumsq + sedt_multi_adamw)", 32.0 * n, t,
       "sumsq reads g (4 B), adamw reads p,g,m,v and writes p,m,v (28 B) per parameter")
    return out


def other_configs(args, dev, keep_alive, replays=20, settle=30):
    """BASELINE.json's configs[2..4] (C3 DCASE weak+strong step, C4 SP-SEDT pre-training step, C5 mean-teacher step with its
    mix-up) and the headline config in the f32 parity mode on this GPU, each captured and timed for a bounded number of replays AFTER
    the headline's timed region, so that they appear in the driver's record too.  Per-rank figures on one GPU; never allowed to cost the headline (errors are reported in
    place)."""
    import copy
    import gc
    import torch
    from sound_event_detection_transformer_amd import runtime
    res = {}
    for name in ('c3', 'c4', 'c5', 'c2_f32', 'c2_bf16x3', 'c2_loader'):
        try:
            a = copy.copy(args)
            a.config, a.mix_up_ratio, a.loader = name, None, False
            if name == 'c2_loader':                  # the headline config fed from host-resident raw clips (H2D + transforms in the loop)
                a.config, a.loader = 'c2', True
            if name == 'c2_f32':                     # the f32 parity mode (the mode that meets north_star's 1e-3) on the headline config
                a.config, a.dtype = 'c2', 'f32'
                runtime.set_compute_dtype('f32')
            if name == 'c2_bf16x3':                  # the parity-grade FAST mode: f32 tensors, split-bf16 products (1e-3 met at MFMA rate)
                a.config, a.dtype = 'c2', 'bf16x3'
                runtime.set_compute_dtype('bf16x3')
            step, clips, flop, what, _, ex = build_workload(a, dev, 0, 1)
            for _ in range(settle):              # (the first replays after a capture run slow: the same settle policy as the headline)
                step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(replays):
                step()
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / replays
            ms = e0.elapsed_time(e1) / replays
            res[name] = {"ms_per_step": round(wall * 1e3, 3), "ms_per_step_hip_events": round(ms, 3), "clips_per_step": clips,
                         "clips_s": round(clips / wall, 1), "dtype": a.dtype, "frac": round(flop / wall / MFMA_PEAK[a.dtype], 4),
                         "peak_tflops": MFMA_PEAK[a.dtype] / 1e12, "replays": replays, "settle_replays": settle, "workload": what}
            if name == 'c2_bf16x3':
                # the parity-grade mode against ITS OWN ceiling: every product is three bf16 MFMAs (hi.hi + lo.hi + hi.lo), so a third of the
                # dense bf16 peak bounds it; and where its step goes, per kernel instance (in-process trace of three further replays)
                ceil_ = MFMA_PEAK['bf16'] / 3.0
                roof = {"bound": "mfma", "achieved": round(flop / (ms * 1e-3) / 1e12, 2), "unit": "TFLOP/s (f32-grade products)",
                        "peak": round(ceil_ / 1e12, 1), "frac_of_mode_ceiling": round(flop / (ms * 1e-3) / ceil_, 4),
                        "frac_of_bf16_peak": round(flop / (ms * 1e-3) / MFMA_PEAK['bf16'], 4),
                        "note": "peak = dense bf16 peak / 3; outputs and losses within 1e-3 of the oracle, gradients within 2e-2 (DESIGN.md section 2)"}
                try:
                    kt = kernel_times(step)
                    rows = sorted(kt.items(), key=lambda kv: -kv[1][0])
                    tot = sum(v[0] for v in kt.values())
                    gemm_us = sum(v[0] for k_, v in kt.items() if k_.startswith(('igemm', 'wgrad3', 'wgrad4', 'bneck', 'conv3x3', 'enc_')))
                    roof["families"] = [{"kernel": k_, "launches": round(v[1], 1), "us": round(v[0], 1), "share": round(v[0] / tot, 4)} for k_, v in rows[:14]]
                    roof["kernel_time_us"] = round(tot, 1)
                    roof["kernels_per_step"] = round(sum(v[1] for v in kt.values()), 1)
                    roof["gemm_family"] = {"us": round(gemm_us, 1), "frac_of_mode_ceiling": round(flop / (gemm_us * 1e-6) / ceil_, 4)}
                    roof["split3_launches"] = round(sum(v[1] for k_, v in kt.items() if k_.startswith('split3')), 1)
                except Exception as e:           # noqa: BLE001
                    roof["families_error"] = repr(e)[:200]
                res[name]["roofline"] = roof
            del step, ex
        except Exception as e:                   # noqa: BLE001
            res[name] = {"error": repr(e)[:200]}
        runtime.set_compute_dtype(args.dtype)
        gc.collect()
        torch.cuda.empty_cache()
    return res


DUMP_BUDGET = 64 << 20              # bytes, all arrays of one --dump-outputs together
DUMP_MAX_ELEMS = 1 << 20            # elements per array; a larger one is written as a fixed, seeded sample of its flat elements


def _dump_sample(t, cap, seed):
    """t flattened; above `cap` elements a sorted sample drawn by a fixed seed (the same indices for the same numel in every run)"""
    import numpy as np
    import torch
    flat = t.detach().reshape(-1)
    if flat.numel() > cap:
        idx = np.unique(np.random.default_rng(seed).integers(0, flat.numel(), cap))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat


def dump_outputs(out_dir, result, model, train):
    """--dump-outputs: `result` is what the last timed step returned (nested dicts / lists / tuples of tensors); for a training
    step also the parameters it updated and the gradients it computed, each as one flat sample over all trainable tensors (the
    same indices in both).  Floating arrays are written as float32 (float64 stays), integer / bool ones as float64.  Returns {name: shape}"""
    import re
    import numpy as np
    import torch
    arrays = []

    def walk(name, v):
        if isinstance(v, torch.Tensor):
            arrays.append((name, v.detach() if v.numel() <= DUMP_MAX_ELEMS else _dump_sample(v, DUMP_MAX_ELEMS, len(arrays))))
        elif isinstance(v, dict):
            for k in sorted(v, key=str):
                walk(f'{name}.{k}', v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f'{name}.{i}', x)
        elif isinstance(v, (bool, int, float)):
            arrays.append((name, torch.tensor(v)))
    walk('out', result)
    if train:
        ps = [p for p in model.parameters() if p.requires_grad]
        arrays.append(('params', _dump_sample(torch.cat([p.detach().float().reshape(-1) for p in ps]), 2 * DUMP_MAX_ELEMS, 0)))
        gs = [p.grad for p in ps if p.grad is not None]
        if gs:
            arrays.append(('grads', _dump_sample(torch.cat([g.detach().float().reshape(-1) for g in gs]), 2 * DUMP_MAX_ELEMS, 0)))
    host = []
    for name, t in arrays:
        a = t.cpu()
        a = a.numpy().astype(np.float64) if not a.is_floating_point() else \
            a.numpy() if a.dtype == torch.float64 else a.float().numpy()
        host.append((re.sub(r'[^A-Za-z0-9_.-]', '_', name), a))
    total = sum(a.nbytes for _, a in host)
    if total > DUMP_BUDGET:
        raise RuntimeError(f'--dump-outputs: {total} bytes, more than {DUMP_BUDGET >> 20} MB')
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host:
        np.save(os.path.join(out_dir, name + '.npy'), a)
    return {name: list(a.shape) for name, a in host}


def pmc_traffic(config, stamp, kernels_per_step):
    """(profile dict or None, reason or None): HBM-side bytes per step from the committed PMC profile of this config (newest
    profiles/rNN_pmc_<config>.json) - but only when that profile was taken ON THIS BUILD: its `build_stamp` must equal the running
    sources' stamp (_build.source_stamp) and, when the per-family trace of this run is available, its kernel count per step must
    equal the running step's.  A stale profile yields (None, why)"""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', f'r*_pmc_{config}.json')), reverse=True):      # newest round first
        try:
            with open(path) as f:
                prof = json.load(f)
        except Exception:
            continue
        name = os.path.relpath(path, ROOT)
        if prof.get('build_stamp') != stamp:
            return None, f"{name} was taken on build {prof.get('build_stamp', '(unstamped)')}, this is build {stamp}"
        if kernels_per_step is not None and abs(prof.get('kernels_per_step', -1) - kernels_per_step) > 4:     # (the in-process trace also counts a few copies)
            return None, f"{name} holds {prof.get('kernels_per_step')} kernels per step, this run launches {kernels_per_step:g}"
        return prof, None
    return None, 'no PMC profile of this configuration under profiles/'


def main():
    args = parse()
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))
    import torch
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        print(f'bench.py: --gpus {args.gpus} does not match WORLD_SIZE {world}', file=sys.stderr)
        sys.exit(2)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if args.share_gpu:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        dist.init_process_group(args.backend)
    dev = torch.device('cuda', local_rank)
    torch.cuda.set_device(dev)

    from sound_event_detection_transformer_amd import runtime, ops
    runtime.set_compute_dtype(args.dtype)
    torch.manual_seed(2020)
    step, clips, flop_step, what, graphed, ex = build_workload(args, dev, rank, world)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # the first replays after a capture run a few percent slow (clocks, caches, the allocator's first touches): a stated number of
    # un-timed settle replays BEFORE the --warmup / --steps the caller asked for, so that a short timed region (the driver's
    # --steps 20 --warmup 5) reads the same steady state as a long one
    settle = args.settle if graphed else 0
    settle_ev = {}
    for i in range(settle):
        if i < 5 or i >= settle - 5:             # the first and last five settle replays are timed one by one (HIP events): does the step
            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)      # still drift when the timed region starts?
            a_.record()
            step()
            b_.record()
            settle_ev[i] = (a_, b_)
        else:
            step()
    for _ in range(args.warmup):
        step()
    barrier()
    settle_ms = {i: round(a_.elapsed_time(b_), 3) for i, (a_, b_) in settle_ev.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    last = None
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        last = step()
    e1.record()
    barrier()
    elapsed = time.perf_counter() - t0
    # what the last timed step returned, before any further step overwrites the graphs' static outputs
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, last, ex['model'], train=args.config != 'eval')
    last = None
    # the host's own cost of ISSUING a step (table refresh, graph launches, RCCL enqueues): three steps queued onto an idle device - the
    # pinned upload rings have four slots, so the host does not block on the GPU inside this burst.  Every rank runs it (collectives match)
    host_issue = None
    if args.full:
        t1 = time.perf_counter()
        for _ in range(3):
            step()
        host_issue = (time.perf_counter() - t1) / 3.0
        barrier()
    dev_ms = e0.elapsed_time(e1) / args.steps           # HIP events on the stream the step's graphs are launched on
    per_rank = [elapsed]
    rccl_world = 1
    # clocks UNDER LOAD, after the timed region: rocm-smi runs in a child while this process keeps replaying the step
    clocks = None
    if args.full and rank == 0 and world == 1 and graphed and not args.no_clocks:   # (world > 1: a step contains collectives - no rank may run extra ones)
        clocks = clocks_under_load(step)
    if world > 1:
        dist = torch.distributed
        t = torch.tensor([elapsed], device=dev if dist.get_backend() == 'nccl' else 'cpu', dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [float(v) for v in allt]
        elapsed = max(per_rank)
        rccl_world = dist.get_world_size() if dist.get_backend() == 'nccl' else 0

    # ---- exposed communication: the same step without the data-parallel schedule (local gradients only), same process
    exposed = None
    if args.full and world > 1 and graphed and 'local_step' in ex:
        try:                                   # a diagnostic after the timed region: never allowed to cost the result line
            loc = ex['local_step']()
            for _ in range(3):
                loc()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                loc()
            torch.cuda.synchronize()
            local_ms = (time.perf_counter() - t1) / args.steps * 1e3
            st = ex.get('stepper')
            exposed = {"local_step_ms": round(local_ms, 3), "exposed_comm_ms": round(elapsed / args.steps * 1e3 - local_ms, 3),
                       "allreduce_segments_mb": [round(v.numel() * v.element_size() / 1e6, 2) for v in getattr(st, 'flat_parts', [])],
                       "dp_cuts": args.dp_cuts, "bucket_dtype": "bf16" if args.bf16_buckets else "f32"}
            del loc
        except Exception as e:                 # noqa: BLE001
            exposed = {"error": repr(e)[:200]}
        barrier()

    # ---- GEMM family alone (c2/c3, rank 0): ONE extra eager step records the argument block of every GEMM launch, which are
    #      then replayed back to back on the launch stream between two HIP events
    gemm = None
    gemm_rec = None
    if args.full and args.config in ('c2', 'c3') and not args.model_only and not args.no_gemm_family:
        if rank != 0 and world > 1 and not graphed:
            ops.PROFILE = []                      # eager DDP: the extra step contains collectives, every rank must take part
            from sound_event_detection_transformer_amd.engine import train_step
            train_step(ex['net'], ex['criterion'], ex['opt'], ex['x'], ex['targets'], ex['wm'], slice(ex['ns']), max_norm=0.1,
                         allreduce=bool(ex.get('eager_allreduce')))
            torch.cuda.synchronize()
            ops.PROFILE = None
        if rank == 0:
          try:                                    # a diagnostic after the timed region: never allowed to cost the result line
              import ctypes
              from sound_event_detection_transformer_amd import lib as L_
              from sound_event_detection_transformer_amd.engine import train_step
              ops.PROFILE = []
              del ops.PROFILE_FUSED[:]
              train_step(ex['net'], ex['criterion'], ex['opt'], ex['x'], ex['targets'], ex['wm'], slice(ex['ns']), max_norm=0.1,
                         allreduce=bool(ex.get('eager_allreduce')))
              torch.cuda.synchronize()
              rec = ops.PROFILE
              ops.PROFILE = None
              n = len(rec)
              lib = L_.load()

              def replay():
                  for a, dt_, *_ in rec:
                      L_.check(lib.sedt_igemm(ctypes.byref(a), dt_, L_.stream_ptr()), 'sedt_igemm')
              replay()
              torch.cuda.synchronize()
              reps = 3
              g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
              g0.record()
              for _ in range(reps):
                  replay()
              g1.record()
              torch.cuda.synchronize()
              tot_ms = g0.elapsed_time(g1) / reps
              if args.dump_igemm:
                  per = []
                  for a, dt_, sh, *_ in rec:
                      s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                      s0.record()
                      for _ in range(5):
                          L_.check(lib.sedt_igemm(ctypes.byref(a), dt_, L_.stream_ptr()), 'sedt_igemm')
                      s1.record()
                      torch.cuda.synchronize()
                      per.append({'ms': s0.elapsed_time(s1) / 5, 'shape': sh})
                  with open(args.dump_igemm, 'w') as f:
                      json.dump(per, f)
              gemm = {"launches_per_step": n, "ms_per_step_replayed_alone": round(tot_ms, 3),
                      "avg_launch_us": round(tot_ms * 1e3 / max(n, 1), 2),
                      "achieved_tflops": round(flop_step / (tot_ms * 1e-3) / 1e12, 1),
                      "frac": round(flop_step / (tot_ms * 1e-3) / MFMA_PEAK[args.dtype], 4),
                      "note": "every conv/linear fwd, dgrad and wgrad launch of one step issued back to back (eager, ungrouped); "
                              "the same family inside the step graph is ~15 % faster (profiles/)"}
              gemm_rec = rec
          except Exception as e:               # noqa: BLE001
            ops.PROFILE = None
            gemm = {"error": repr(e)[:200]}

    # ---- per-kernel-family roofline of the measured step (rank 0): in-process kernel trace of three further steps, joined with the
    #      shapes of the recorded GEMM launches
    fam = None
    if args.full and rank == 0 and world == 1 and graphed and not args.no_families and not args.model_only:
        try:
            n_params = sum(p.numel() for p in ex['model'].parameters() if p.requires_grad)
            fam = family_report(step, gemm_rec, args.dtype, n_params, dev_ms)
        except Exception as e:                 # noqa: BLE001  (a diagnostic: never allowed to cost the result line)
            fam = {"error": repr(e)[:300]}
    gemm_rec = None

    if rank == 0:
        peak = MFMA_PEAK[args.dtype]
        ach = flop_step / (dev_ms * 1e-3)
        from sound_event_detection_transformer_amd import _build
        stamp = _build.source_stamp()
        kps = None
        if fam and fam.get('families'):
            kps = round(sum(r['launches'] for r in fam['families']), 1)
        traffic, traffic_why = pmc_traffic(args.config, stamp, kps)
        dom = None
        if fam and fam.get('families'):
            dom = next((r for r in fam['families'] if 'frac' in r), None)
        roof = {"bound": "mfma",
                "kernel": "whole training-step graph (>= 99 % of its algorithmic flops are the MFMA implicit-GEMM family "
                          "sedt::igemm3* / wgrad3/4*)" + (f"; dominant kernel by time: {dom['kernel']} - see dominant / families" if dom else
                                                          "; see gemm_family and kernels" if args.full else "; per-kernel figures: --full"),
                "achieved": round(ach / 1e12, 2), "peak": peak / 1e12, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                "traffic": None if traffic is None else traffic.get('hbm_bytes_per_step'),
                "traffic_source": traffic_why if traffic is None else traffic.get('source'),
                "algorithmic_flop_per_launch": flop_step, "launch": "one step = one replay of the step's HIP graph(s)",
                "avg_launch_ms_hip_events": round(dev_ms, 4), "gemm_family": gemm}
        if fam is not None:
            if dom is not None:       # the dominant kernel instance against ITS roofline: algorithmic flops (bytes) of its launches in one
                roof["dominant"] = dict(dom, avg_launch_us=round(dom['us'] / max(dom['launches'], 1), 2))      # step / their summed duration
            roof.update({k: v for k, v in fam.items()})
            if roof.get("traffic") and fam.get("algorithmic_bytes"):
                roof["traffic_over_algorithmic"] = round(roof["traffic"] / fam["algorithmic_bytes"], 2)
        kernels = None
        if args.full and not args.no_kernels and args.config == 'c2':
            try:
                kernels = kernel_report(args.dtype, dev)
            except Exception as e:                                   # the report must never cost the headline number
                kernels = [{"error": repr(e)}]
        others = None
        if args.full and args.config == 'c2' and world == 1 and graphed and not args.no_other_configs and args.dtype == 'bf16' and not args.batch:
            others = other_configs(args, dev, (ex, step))
        cpu = None if (not args.full or args.no_cpu_baseline or world > 1) else cpu_baseline()
        value = world * clips * args.steps / elapsed
        kind = "inference (validation step)" if args.config == 'eval' else "training"
        out = {"metric": f"audio clips/sec {kind} throughput (B={clips}, 10s@64-mel)", "value": round(value, 2),
               "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": what, "name": args.config, "global_batch": world * clips, "parallelism": f"dp{world}"},
               "roofline": roof, "kernels": kernels, "cpu_baseline": cpu, "hip_graph": graphed,
               "rccl_world": rccl_world, "ms_per_step_per_rank": [round(v / args.steps * 1e3, 3) for v in per_rank],
               "exposed_comm": exposed, "settle_replays": settle, "build_stamp": stamp, "kernels_per_step": kps,
               "settle_replay_ms": {"first": [settle_ms[i] for i in sorted(settle_ms) if i < 5],
                                    "last": [settle_ms[i] for i in sorted(settle_ms) if i >= 5 or settle <= 5][-5:]},
               "clocks_under_load": clocks,
               # time the host spends ISSUING one step (table refresh, graph launches, RCCL enqueues; measured as a burst of three onto an idle device): while
               # this stays below ms_per_step the GPU never waits for the host; at N > 1 it tells exposed communication from host issue time
               "host_launch_us_per_step": None if host_issue is None else round(host_issue * 1e6, 1)}
        if dumped is not None:
            out["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if others is not None:
            out["other_configs"] = others
        if ex.get('graph_fallback'):
            out["graph_fallback"] = ex['graph_fallback']
        print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
