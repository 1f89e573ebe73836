"""TargetTables.load_mixed (one pinned-ring upload of index and lam, ONE sedt_mixup_plan launch into the tables and the job buffer) timed
against the host route for the same draws - targets.to_list() (a synchronising read-back), utilities.mixup.plan_mixup_data,
TargetTables.load of the merged list, the job table upload - at the batch sizes of the two recipes that mix, in ONE process:
  c3   32 clips: 16 strong + 16 weak, the first 16 mixed
  c5   the labelled 32 (16 strong + 16 weak) of a 64-clip mean-teacher batch whose 32 unlabelled clips follow in the same blob
Per case it prints
  call        host clock around N calls of a route, the device drained at the end of the window (what the host spends per step and what
              a step waits for); median of R windows + range; the two routes alternate inside every repetition
  device      device events around N back-to-back load_mixed calls: upload + launch as the stream sees them
  clocks      read while the launch keeps running (bench.clocks_under_load; read, never set)
    python tools/time_mixup_plan.py"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM, R = 50, 3, 7
MAX_TARGETS, MAX_EVENTS = 32, 20


def source(B, ns, n_lab, seed):
    """(blob uint8 of B all-strong clips in sedt_cut_clips' layout, list form): strong clips with 0 .. 6 events, weak ones with 1 .. 3 tags
    staged as whole-window events, unlabelled ones empty"""
    gen = np.random.default_rng(seed)
    labs, boxes = [], []
    for b in range(B):
        n = int(gen.integers(0, 7)) if b < ns else (int(gen.integers(1, 4)) if b < n_lab else 0)
        length = gen.uniform(0.03, 0.3, n) if b < ns else np.ones(n)
        centre = gen.uniform(length / 2, 1 - length / 2) if b < ns else np.full(n, 0.5)
        labs.append(gen.integers(0, 10, n).astype(np.int64))
        boxes.append(np.stack([centre, length], 1).astype(np.float32).reshape(-1, 2))
    off = np.concatenate([[0], np.cumsum([len(l) for l in labs])]).astype(np.int32)
    o_lab = 8 * B + 16
    o_box = o_lab + 8 * B * MAX_TARGETS
    raw = np.zeros(o_box + 8 * B * MAX_TARGETS, np.uint8)
    raw[:8 * (B + 1) + 8] = np.concatenate([off, off, [B, B]]).astype(np.int32).view(np.uint8)
    lab, box = np.concatenate(labs), np.concatenate(boxes)
    raw[o_lab:o_lab + lab.nbytes] = lab.view(np.uint8)
    raw[o_box:o_box + box.nbytes] = box.reshape(-1).view(np.uint8)
    return raw


def host_route(targets, tables, jobs, lam, index, B, ns, n_lab, mix_num):
    from sound_event_detection_transformer_amd.utilities.mixup import job_table, plan_mixup_data
    lst = targets.to_list()[:B]
    recs, mixed, n_strong, n_weak = plan_mixup_data(lst, slice(ns), slice(ns, n_lab), lam, index, mix_num / B, MAX_EVENTS)
    tables.load(mixed, ns=n_strong, n_lab=n_strong + n_weak)
    jobs.send(job_table(recs))


def case(name, B_src, B, ns, n_lab, mix_num, res):
    import bench
    from sound_event_detection_transformer_amd.engine import _Upload
    from sound_event_detection_transformer_amd.sedt import TargetTables
    from sound_event_detection_transformer_amd.utilities.mixup import draw_mixup_data
    from sound_event_detection_transformer_amd.utilities.recording_clips import DeviceTargets
    dev = torch.device('cuda')
    dt = DeviceTargets(torch.from_numpy(source(B_src, ns, n_lab, B_src)).to(dev), torch.zeros(B_src, dtype=torch.int32, device=dev), B_src,
                       MAX_TARGETS, [f'r{b}' for b in range(B_src)], 10.0, ns=ns, n_lab=n_lab)
    on_dev = TargetTables(B, ns, n_lab, dev, max_targets=MAX_TARGETS, dynamic_split=True, with_ratio=True)
    on_host = TargetTables(B, ns, n_lab, dev, max_targets=MAX_TARGETS, dynamic_split=True, with_ratio=True)
    jobs_dev, jobs_host = _Upload(16 * B, dev), _Upload(16 * B, dev)
    np.random.seed(2)
    draws = [draw_mixup_data(B, 1) for _ in range(N)]
    device_route = lambda k: on_dev.load_mixed(dt, draws[k][0], draws[k][1], mix_num, MAX_EVENTS, jobs_dev.dev_buf)
    host = lambda k: host_route(dt, on_host, jobs_host, draws[k][0], draws[k][1], B, ns, n_lab, mix_num)
    call = {'device': [], 'host': []}
    for i in range(WARM + R):
        for key, fn in (('device', device_route), ('host', host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(N):
                fn(k)
            torch.cuda.synchronize()
            if i >= WARM:
                call[key].append((time.perf_counter() - t0) * 1e6 / N)
    same = bool(torch.equal(on_dev.off, on_host.off)) and bool(torch.equal(jobs_dev.dev_buf, jobs_host.dev_buf))
    windows = []
    for _ in range(R):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(N):
            device_route(k)
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / N)
    clocks = bench.clocks_under_load(lambda: device_route(0))
    d, h = float(np.median(call['device'])), float(np.median(call['host']))
    res[name] = dict(B_src=B_src, B=B, ns=ns, n_lab=n_lab, mix_num=mix_num, load_mixed_call_us=round(d, 1), load_mixed_min_us=round(min(call['device']), 1),
                     load_mixed_max_us=round(max(call['device']), 1), host_route_call_us=round(h, 1), host_route_min_us=round(min(call['host']), 1),
                     host_route_max_us=round(max(call['host']), 1), host_over_device=round(h / d, 1),
                     device_events_us=round(float(np.median(windows)), 1), device_events_min_us=round(min(windows), 1),
                     device_events_max_us=round(max(windows), 1), same_tables_and_jobs=same, clocks=clocks)
    print(f'{name}: load_mixed {d:7.1f} us per call ({min(call["device"]):.1f} .. {max(call["device"]):.1f}), by device events '
          f'{np.median(windows):.1f} us ({min(windows):.1f} .. {max(windows):.1f}); host route {h:8.1f} us ({min(call["host"]):.1f} .. '
          f'{max(call["host"]):.1f}), x{h / d:.1f}; same offsets and jobs: {same}; clocks {clocks}', flush=True)


def main():
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    res = {}
    case('c3', 32, 32, 16, 32, 16, res)
    case('c5', 64, 32, 16, 32, 16, res)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
