"""GPU: the graphed data-parallel steps with world_size 2 (two processes sharing the one test GPU, gloo transport, the
flat gradient buffer staged through the host by engine.allreduce_mean).  Checked for the supervised, the SP-SEDT and the
mean-teacher step: replicas stay bit-identical; the segmented / overlapped schedule equals the single all-reduce schedule;
bf16 buckets stay close to f32 buckets; and ONE data-parallel step equals a single-process optimizer
step fed the explicit MEAN of the two ranks' gradients (each computed eagerly on that rank's batch).  Equality with a
single-process step on the concatenated batch is NOT expected: num_boxes is normalised per rank (sedt.py:322-324)."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(kind, dev, B, rank=0):
    """(model, criterion, optimizer, extra constructor kwargs, batch function) of one of the three data-parallel workloads"""
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    from sound_event_detection_transformer_amd.engine import build_optimizer
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict, synthetic_batch
    args = dict(sedt=dict(dropout=0.0), spsedt=dict(enc_layers=3, num_queries=20, dec_at=False, self_sup=True, lr_backbone=0.0, dropout=0.0),
                semi=dict(dropout=0.0))[kind]
    model, crit, _ = build_model(default_args(**args))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 3))
    model.to(dev).train()
    if kind == 'spsedt':
        model.mask_ratio = -1.0                               # every query keeps its patch: no random mask between the runs
    crit.to(dev)
    opt = build_optimizer(model)

    def batch(seed):
        if kind == 'spsedt':
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(B, 1, 496, 64, generator=g).to(dev)
            patches = torch.randn(B, 10, 1, 128, 64, generator=g).to(dev)
            t = []
            for _ in range(B):
                l = torch.rand(10, generator=g) * 0.3 + 0.05
                c = l / 2 + torch.rand(10, generator=g) * (1 - l)
                t.append({'labels': torch.zeros(10, dtype=torch.int64, device=dev), 'boxes': torch.stack([c, l], -1).to(dev)})
            return x, t, patches
        x, t = synthetic_batch(B, 500, seed, dev)
        return x, t, None
    return model, crit, opt, batch


def _make_stepper(kind, model, crit, opt, batch, B, **kw):
    from sound_event_detection_transformer_amd.engine import GraphedTrainStep, GraphedSemiStep
    from sound_event_detection_transformer_amd.utilities.utils import EMA
    x, t, patches = batch(100)
    if kind == 'semi':                                        # labelled clips 0..B/2, unlabelled B/2..B (one view)
        ema = EMA(model, 0.9)
        ema.register()
        h = B // 2
        for tt in t[h:]:
            tt['labels'], tt['boxes'] = tt['labels'][:0], tt['boxes'][:0]
        thr = torch.full((10,), 0.03, device=x.device)           # (random-init teacher: a low threshold keeps pseudo events alive)
        st = GraphedSemiStep(model, ema, crit, opt, x, x, t, slice(h), None, slice(h), slice(h, B), thr, warmup=1, **kw)
        return st, (lambda b: st(b[0], b[0], [dict(q, labels=q['labels'][:0], boxes=q['boxes'][:0]) if i >= h else q
                                              for i, q in enumerate(b[1])]))
    if kind == 'spsedt':
        st = GraphedTrainStep(model, crit, opt, x, t, slice(B), slice(B), warmup=1, example_patches=patches, **kw)
        return st, (lambda b: st(b[0], b[1], patches=b[2]))
    st = GraphedTrainStep(model, crit, opt, x, t, None, slice(B), warmup=1, **kw)
    return st, (lambda b: st(b[0], b[1]))


def _worker(rank, world, port, out, overlap=True, nsteps=2, kind='sedt', cuts='coarse', bf16=False):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import dp_segment_plan
    dev = torch.device('cuda', 0)
    runtime.set_compute_dtype('bf16')
    B = 4 if kind == 'semi' else 2
    model, crit, opt, batch = _build(kind, dev, B)
    plan = dp_segment_plan(model, cuts)
    if not overlap:          # same flat parameter order as the overlapped schedule: identical summation order of the grad norm
        opt.set_segments([sg[0] for sg in plan])
    stepper, run = _make_stepper(kind, model, crit, opt, batch, B, overlap_allreduce=overlap, dp_cuts=cuts,
                                 grad_dtype=torch.bfloat16 if bf16 else None)
    assert len(stepper.g_seg) == (len(plan) - 1 if overlap else 0), (len(stepper.g_seg), len(plan))
    v0 = torch.cat([p.detach().flatten().float().cpu() for p in model.parameters() if p.requires_grad])
    for i in range(nsteps):
        run(batch(200 + 10 * i + rank))
    torch.cuda.synchronize()
    vec = torch.cat([p.detach().flatten().float().cpu() for p in model.parameters() if p.requires_grad])
    both = [torch.zeros_like(vec) for _ in range(world)]
    dist.all_gather(both, vec)
    if rank == 0:
        ok = bool(torch.isfinite(vec).all()) and int(stepper.nonfinite.item()) == 0 and bool((vec != v0).any())
        torch.save({'same': bool(torch.equal(both[0], both[1])), 'finite': ok,
                    'norm': float(vec.norm()), 'vec': vec, 'nseg': len(plan)}, out)
    dist.destroy_process_group()


@pytest.mark.parametrize('kind,cuts,nseg', [('sedt', 'coarse', 4), ('sedt', 'fine', 5), ('spsedt', 'coarse', 2), ('semi', 'coarse', 4)])
def test_graphed_dp_world2_replicas_stay_identical(tmp_path, kind, cuts, nseg):
    """world 2: the backward cut in nseg segments, each segment's all-reduce issued as soon as its graph is queued - for the
    supervised step (C2/C3), the SP-SEDT pre-training step (C4: the reference's DDP configuration, train_spsedt.py:157-158; frozen
    backbone, cut at the encoder output) and the mean-teacher step (C5).  Replicas stay bit-identical and the result equals the
    single all-reduce schedule on the same flat layout"""
    out = str(tmp_path / 'r.pt')
    mp.spawn(_worker, args=(2, _free_port(), out, True, 2, kind, cuts), nprocs=2, join=True)
    r = torch.load(out)
    assert r['same'] and r['finite'] and r['nseg'] == nseg, {k: v for k, v in r.items() if k != 'vec'}
    # the same two steps without the backward cuts / split all-reduce (same flat layout order): same parameters
    out2 = str(tmp_path / 'r2.pt')
    mp.spawn(_worker, args=(2, _free_port(), out2, False, 2, kind, cuts), nprocs=2, join=True)
    r2 = torch.load(out2)
    assert r2['same'] and r2['finite']
    d = (r['vec'] - r2['vec']).abs().max().item()
    assert d <= 1e-6 * max(1.0, r2['vec'].abs().max().item()), d


def test_bf16_gradient_buckets_stay_close_to_f32_buckets(tmp_path):
    """grad_dtype=bf16 (half the all-reduce bytes): replicas identical; ONE step lands within a few per cent of an AdamW step of
    the f32-bucket result (gradients rounded to 8 mantissa bits once, before the average)"""
    a, b = str(tmp_path / 'bf.pt'), str(tmp_path / 'f32.pt')
    mp.spawn(_worker, args=(2, _free_port(), a, True, 1, 'sedt', 'coarse', True), nprocs=2, join=True)
    mp.spawn(_worker, args=(2, _free_port(), b, True, 1, 'sedt', 'coarse', False), nprocs=2, join=True)
    ra, rb = torch.load(a), torch.load(b)
    assert ra['same'] and ra['finite'] and rb['same']
    v0 = _initial_vec()
    # (L2, not max: the first Adam step moves every element by ~ lr * sign(g), so an element whose tiny gradient changes sign
    # under the rounding differs by a whole step; what must hold is that such elements are rare)
    moved = (rb['vec'] - v0).norm().item()
    d = (ra['vec'] - rb['vec']).norm().item()
    assert moved > 0 and 0 < d <= 0.05 * moved, (d, moved)


def _mean_grad_worker(rank, out):
    """single process: eager gradients of rank 0's and rank 1's first batch from the same initial weights, their explicit
    mean, one fused clip + AdamW step"""
    sys.path.insert(0, ROOT)
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    from sound_event_detection_transformer_amd.engine import build_optimizer
    from sound_event_detection_transformer_amd.utilities.synthetic import synthetic_batch
    from oracle import sedt_oracle as O
    dev = torch.device('cuda', 0)
    runtime.set_compute_dtype('bf16')
    model, crit, _ = build_model(default_args(dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), 3))
    model.to(dev).train()
    crit.to(dev)
    opt = build_optimizer(model)
    from sound_event_detection_transformer_amd.engine import dp_segment_plan
    opt.set_segments([sg[0] for sg in dp_segment_plan(model, 'coarse')])
    B = 2
    grads = []
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for r in range(2):
            x, t = synthetic_batch(B, 500, 200 + r, dev)
            crit(model(x), t, None, slice(B))
            crit.last_total.backward()
            crit.last_total = None
            grads.append([p.grad.clone() for p in model.parameters() if p.requires_grad])
            opt.zero_grad(set_to_none=True)
        for p, g0, g1 in zip([p for p in model.parameters() if p.requires_grad], *grads):
            p.grad = (g0 + g1) / 2
        opt.step(max_norm=0.1)
    torch.cuda.synchronize()
    vec = torch.cat([p.detach().flatten().float().cpu() for p in model.parameters() if p.requires_grad])
    torch.save({'vec': vec}, out)


def test_one_dp_step_equals_step_on_mean_of_rank_gradients(tmp_path):
    out = str(tmp_path / 'dp1.pt')
    mp.spawn(_worker, args=(2, _free_port(), out, True, 1), nprocs=2, join=True)
    ref = str(tmp_path / 'mean.pt')
    mp.spawn(_mean_grad_worker, args=(ref,), nprocs=1, join=True)
    a, b = torch.load(out), torch.load(ref)
    assert a['same'] and a['finite']
    d = (a['vec'] - b['vec']).abs().max().item()
    moved = (a['vec'] - _initial_vec()).abs().max().item()
    assert moved > 0 and d <= 2e-2 * moved, (d, moved)            # graph vs eager bf16 kernels: a few % of one AdamW step


def _initial_vec_all(kind):
    """every parameter (trainable or not) of the freshly built model of _build(kind, ...), on the host"""
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict
    args = dict(sedt=dict(dropout=0.0), spsedt=dict(enc_layers=3, num_queries=20, dec_at=False, self_sup=True, lr_backbone=0.0, dropout=0.0),
                semi=dict(dropout=0.0))[kind]
    model, _, _ = build_model(default_args(**args))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 3))
    return torch.cat([p.detach().float().flatten() for p in model.parameters()])


def _initial_vec():
    sys.path.insert(0, ROOT)
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    from oracle import sedt_oracle as O
    model, _, _ = build_model(default_args(dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), 3))
    return torch.cat([p.detach().flatten().float() for p in model.parameters() if p.requires_grad])


def _nccl_worker(rank, port, out, dp, kind='sedt'):
    """one process, one GPU; dp=True: RCCL process group of size 1 with the multi-GPU schedule forced"""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.engine import dp_segment_plan
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    if dp:
        dist.init_process_group('nccl', rank=0, world_size=1)
    runtime.set_compute_dtype('bf16')
    B = 4 if kind == 'semi' else 2
    model, crit, opt, batch = _build(kind, dev, B)
    plan = dp_segment_plan(model, 'coarse')
    if not dp:
        # same flat parameter order as the data-parallel schedule picks, so that the global-norm summation order - and with
        # it every bit of the clipped AdamW update - is the same in both runs (bf16 training amplifies 1-ulp differences)
        opt.set_segments([sg[0] for sg in plan])
    stepper, run = _make_stepper(kind, model, crit, opt, batch, B, data_parallel=True if dp else None)
    assert len(stepper.g_seg) == (len(plan) - 1 if dp else 0)
    v0 = torch.cat([p.detach().flatten().float().cpu() for p in model.parameters() if p.requires_grad])
    for i in range(2):
        run(batch(200 + 10 * i))
    torch.cuda.synchronize()
    vec = torch.cat([p.detach().flatten().float().cpu() for p in model.parameters() if p.requires_grad])
    sunk = 0
    if dp:                  # parameters whose static gradient IS its slot of the flat buffer (ops.grad_sink): no packing copy for them
        flat = opt._flat_g
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size()
        sunk = sum(1 for p in model.parameters() if p.grad is not None and lo <= p.grad.data_ptr() < hi)
    torch.save({'vec': vec, 'sunk': sunk,
                'finite': bool(torch.isfinite(vec).all()) and int(stepper.nonfinite.item()) == 0 and bool((vec != v0).any())}, out)
    if dp:
        dist.destroy_process_group()


@pytest.mark.parametrize('kind', ['sedt', 'spsedt', 'semi'])
def test_rccl_schedule_on_one_gpu_matches_single_process_step(tmp_path, kind):
    """the multi-GPU schedule (segmented backward, one asynchronous RCCL AVG all-reduce per flat segment, optimizer graph) on a
    process group of size 1 - exercises the real RCCL calls between the graphs - equals the plain one-graph step"""
    a, b = str(tmp_path / 'dp.pt'), str(tmp_path / 'single.pt')
    mp.spawn(_nccl_worker, args=(_free_port(), a, True, kind), nprocs=1, join=True)
    mp.spawn(_nccl_worker, args=(_free_port(), b, False, kind), nprocs=1, join=True)
    ra, rb = torch.load(a), torch.load(b)
    assert ra['finite'] and rb['finite']
    # the convolution / FFN / attention-projection weights of the trainable part deliver their gradients in place
    assert ra['sunk'] >= {'sedt': 60, 'spsedt': 30, 'semi': 60}[kind], ra['sunk']
    diff = (ra['vec'] - rb['vec']).abs()
    d = diff.max().item()
    where = torch.nonzero(diff > 0).flatten()
    assert d <= 1e-6 * max(1.0, rb['vec'].abs().max().item()), \
        f'max |dp - single| = {d:.3e}; {where.numel()} of {diff.numel()} elements differ, first at flat index {where[:4].tolist()}'


def _ddp_worker(rank, port, out, ddp):
    """eager train_step with the model wrapped in torch DistributedDataParallel over RCCL (world size 1) - the path bench.py
    falls back to when the graphed data-parallel schedule cannot be built - against the same eager steps without the wrapper"""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    from sound_event_detection_transformer_amd import runtime
    from sound_event_detection_transformer_amd.sedt import build_model, default_args
    from sound_event_detection_transformer_amd.engine import build_optimizer, train_step, train_stream
    from sound_event_detection_transformer_amd.utilities.synthetic import seeded_state_dict, synthetic_batch
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    if ddp:
        dist.init_process_group('nccl', rank=0, world_size=1)
    runtime.set_compute_dtype('bf16')
    runtime.manual_seed(4)
    model, crit, _ = build_model(default_args(dropout=0.0))
    model.load_state_dict(seeded_state_dict(model.state_dict(), 3))
    model.to(dev).train()
    crit.to(dev)
    opt = build_optimizer(model)
    net = model
    if ddp:
        with torch.cuda.stream(train_stream(dev)):          # DDP's AccumulateGrad hooks belong to the stream the steps run on
            net = torch.nn.parallel.DistributedDataParallel(model, device_ids=[0], broadcast_buffers=False, gradient_as_bucket_view=True)
    B = 2
    losses = []
    for i in range(3):
        x, t = synthetic_batch(B, 500, 300 + 10 * i, dev)
        total, ld = train_step(net, crit, opt, x, t, None, slice(B), max_norm=0.1)
        losses.append(float(total))
    torch.cuda.synchronize()
    vec = torch.cat([p.detach().flatten().float().cpu() for p in model.parameters() if p.requires_grad])
    torch.save({'vec': vec, 'losses': losses}, out)
    if ddp:
        dist.destroy_process_group()


def test_eager_step_under_torch_ddp_matches_plain_eager_step(tmp_path):
    a, b = str(tmp_path / 'ddp.pt'), str(tmp_path / 'plain.pt')
    mp.spawn(_ddp_worker, args=(_free_port(), a, True), nprocs=1, join=True)
    mp.spawn(_ddp_worker, args=(_free_port(), b, False), nprocs=1, join=True)
    ra, rb = torch.load(a), torch.load(b)
    # the first step sees identical parameters: identical losses; later steps differ by what bf16 training makes of a different
    # f32 summation order in the global gradient norm (bucket views vs per-parameter gradients): bounded, not bit-equal
    assert abs(ra['losses'][0] - rb['losses'][0]) <= 1e-6 * abs(rb['losses'][0]), (ra['losses'], rb['losses'])
    assert all(abs(x - y) <= 1e-2 * abs(y) for x, y in zip(ra['losses'], rb['losses'])), (ra['losses'], rb['losses'])
    assert torch.isfinite(ra['vec']).all()
    v0 = _initial_vec()
    ua, ub = ra['vec'] - v0, rb['vec'] - v0
    assert ub.norm().item() > 0
    assert (ua - ub).norm().item() <= 0.1 * ub.norm().item(), ((ua - ub).norm().item(), ub.norm().item())


def _run_bench_world2(extra, transport=('--backend', 'gloo', '--share-gpu')):
    """bench.py's own rank path, launched exactly as the driver launches it (python -m torch.distributed.run, one process per rank),
    two ranks sharing the one test GPU over gloo - or, transport=('--backend', 'nccl'), one GPU per rank over RCCL.  --full: the tests read
    `exposed_comm`, which only a full run measures"""
    import json
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--settle', '2',
           '--batch', '4', *transport, '--full', '--no-cpu-baseline', '--no-kernels', '--no-other-configs'] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{') and '"metric"' in l]
    assert len(lines) == 1, r.stdout[-2000:]                      # rank 0 prints ONE line, the other ranks none
    return json.loads(lines[0]), r.stderr


def test_bench_rank_path_world2_gloo_graphed_schedule():
    """multi-GPU readiness without multi-GPU hardware: build -> agree_out_of_band -> timed loop -> exposed_comm
    -> line, through the captured data-parallel schedule.  The line must say what it is: 2 ranks, NOT RCCL (rccl_world 0)."""
    out, _ = _run_bench_world2([])
    assert out['n_gpus'] == 2 and out['rccl_world'] == 0 and out['hip_graph'] is True and 'graph_fallback' not in out
    assert out['config']['global_batch'] == 8 and out['config']['parallelism'] == 'dp2' and out['scaling'] == 'weak'
    assert len(out['ms_per_step_per_rank']) == 2 and out['value'] > 0
    ec = out['exposed_comm']
    assert ec and 'error' not in ec and ec['local_step_ms'] > 0 and len(ec['allreduce_segments_mb']) >= 2, ec
    assert abs(out['value'] - 8 * 3 / (out['ms_per_step'] * 3e-3)) < 1e-2 * out['value']       # value = all ranks' clips / max-rank time


def test_bench_rank_path_world2_gloo_forced_graph_fallback():
    """the branch the first real multi-GPU execution may take: no rank can build the captured stepper, the ranks agree on that through
    the TCP store (no collective) and ALL take the eager data-parallel step; the line reports it"""
    out, err = _run_bench_world2(['--force-graph-fallback'])
    assert out['n_gpus'] == 2 and out['rccl_world'] == 0 and out['hip_graph'] is False
    assert 'force-graph-fallback' in out['graph_fallback'] and 'graphed data-parallel step failed' in err
    assert out['exposed_comm'] is None and out['value'] > 0 and len(out['ms_per_step_per_rank']) == 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# Two real GPUs, RCCL.  The pool this repository is developed on gives ONE GPU per call, so these tests skip there; on any box with
# two visible devices (the driver's 8-GPU node) they run by themselves: the first N > 1 RCCL execution of the captured data-parallel
# schedule is then a TEST, not the round-end scaling bench.  torch.cuda.device_count() does not initialise the GPU (the children are
# launched before anything in this process does); reference: train_spsedt.py:110-115, 157-158 (DistributedSampler + DDP).
def _two_gpus():
    try:
        return torch.cuda.device_count() >= 2
    except Exception:
        return False


needs_two_gpus = pytest.mark.skipif(not _two_gpus(), reason='needs two visible GPUs (the development pool has one per call)')


@needs_two_gpus
def test_bench_rank_path_world2_rccl_one_gpu_per_rank():
    """bench.py --gpus 2 over RCCL, one process per GPU, launched as the driver launches it: the captured segment / all-reduce schedule
    on real xGMI, the line says rccl_world 2"""
    out, _ = _run_bench_world2([], transport=('--backend', 'nccl'))
    assert out['n_gpus'] == 2 and out['rccl_world'] == 2 and out['hip_graph'] is True and 'graph_fallback' not in out, out
    assert out['config']['global_batch'] == 8 and out['scaling'] == 'weak' and out['value'] > 0
    ec = out['exposed_comm']
    assert ec and 'error' not in ec and len(ec['allreduce_segments_mb']) >= 2, ec


def _rccl2_worker(rank, port, path, kind):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    dev = torch.device('cuda', rank)
    torch.cuda.set_device(dev)
    dist.init_process_group('nccl', rank=rank, world_size=2)
    from sound_event_detection_transformer_amd import runtime
    runtime.set_compute_dtype('bf16')
    B = 4 if kind == 'semi' else 2
    model, crit, opt, batch = _build(kind, dev, B)
    stepper, run = _make_stepper(kind, model, crit, opt, batch, B)
    assert stepper.dp and len(stepper.g_seg) >= 1
    for i in range(3):
        run(batch(200 + 10 * i + rank))                        # per-rank data
    torch.cuda.synchronize()
    vec = torch.cat([p.detach().float().flatten() for p in model.parameters()]).cpu()
    torch.save({'vec': vec, 'ok': int(stepper.nonfinite.item()) == 0}, path + f'.{rank}')
    dist.barrier()
    dist.destroy_process_group()


@needs_two_gpus
@pytest.mark.parametrize('kind', ['sedt', 'spsedt', 'semi'])
def test_replicas_stay_bit_identical_over_rccl_two_gpus(tmp_path, kind):
    """three captured data-parallel steps on per-rank data, one GPU per rank over RCCL, for the supervised, the SP-SEDT (the reference's
    DDP configuration) and the mean-teacher step: the replicas must end with bit-identical parameters (the averaged gradient is the same
    tensor on both ranks, the optimizer is deterministic) that moved and stayed finite"""
    path = str(tmp_path / 'vec')
    mp.spawn(_rccl2_worker, args=(_free_port(), path, kind), nprocs=2, join=True)
    a, b = torch.load(path + '.0'), torch.load(path + '.1')
    assert a['ok'] and b['ok'] and torch.isfinite(a['vec']).all() and torch.equal(a['vec'], b['vec'])
    assert (a['vec'] - _initial_vec_all(kind)).abs().max().item() > 0
