"""The resampler's one launch (sedt_resample) timed at the sizes a user runs, in ONE process, inputs resident on the device:
  hour_mono    one hour, mono f32, 44.1 kHz -> 16 kHz kaiser_best       (158.76 M samples in, 57.6 M out, 354 taps)
  hour_stereo  one hour, stereo int16, 48 kHz -> 16 kHz kaiser_best     (172.8 M frames in, 57.6 M out, 386 taps)
  clips        64 x 10 s mono f32, 48 kHz -> 44.1 kHz kaiser_best       (64 x 480000 in, 64 x 441000 out, 140 taps)
Per case it prints
  the launch time: device events around N back-to-back launches (after WARM), median of R such windows with their range;
  the bytes the launch has to move (input read once + output written) and the HBM floor at 8 TB/s;
  the arithmetic it stands for: n_out * taps f32 FMA, and the rate;
  the clocks read while the launch keeps running (bench.clocks_under_load; read, never set).
Then the sanity condition: ONE ten-minute 44.1 kHz mono recording through RecordingDetector (DCASE front end, the seeded C2-size model
of the tests, bf16, windows of 10 s every 5 s, 8 per replay), with sample_rates=44100 and - the same recording resampled beforehand -
without; host clock around submit(...).result(), median of R calls after a warm-up call; and the resample launch of that recording
alone.  Resampling a recording has to cost less than detecting it.
    python tools/time_resample.py [--short]        (--short: a minute instead of an hour, for a rehearsal)
Kernel times (without launch gaps) come from a trace of the same run, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o resample -- python tools/time_resample.py"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM, R = 10, 3, 5
HBM_TBS = 8.0


def time_launch(run):
    for _ in range(WARM):
        run()
    torch.cuda.synchronize()
    windows = []
    for _ in range(R):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            run()
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / N)
    return float(np.median(windows)), min(windows), max(windows)


def launch_case(name, rs, clips, res):
    import bench
    ns = [rs.n_out(n) for _, n, _ in clips]
    stride = max(ns)
    out = torch.empty((len(clips), stride), device='cuda')
    run = rs.prepare(clips, out.view(-1), [i * stride for i in range(len(clips))], [stride] * len(clips))
    us, lo, hi = time_launch(run)
    mb = (sum(w.numel() * w.element_size() for w, _, _ in clips) + out.numel() * 4) / 1e6
    gfma = sum(ns) * rs.plan.taps / 1e9
    floor_us = mb / HBM_TBS
    clocks = bench.clocks_under_load(run)
    res[name] = dict(L=rs.plan.L, M=rs.plan.M, taps=rs.plan.taps, table_kb=round(rs.table.nbytes / 1e3, 1), outputs=sum(ns),
                     launch_us=round(us, 1), min_us=round(lo, 1), max_us=round(hi, 1), hbm_mb=round(mb, 1), hbm_floor_us=round(floor_us, 1),
                     times_floor=round(us / floor_us, 1), gfma=round(gfma, 2), tfma_per_s=round(gfma / us * 1e3, 2), clocks=clocks)
    print(f'{name:12s}: {us:9.1f} us per launch (windows {lo:.1f} .. {hi:.1f}), {mb:7.1f} MB -> HBM floor {floor_us:6.1f} us, x{us / floor_us:.1f}; '
          f'{gfma:.2f} G FMA = {gfma / us * 1e3:.2f} T FMA/s; clocks {clocks}', flush=True)
    return us


def detector_case(res, seconds=600):
    from oracle import sedt_oracle as O
    from sound_event_detection_transformer_amd import runtime, sedt
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    runtime.set_compute_dtype('bf16')
    runtime.manual_seed(5)
    model, _, post = sedt.build_model(sedt.default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), 2020))
    model.cuda().eval()
    mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
    dec = EventDecoder([f'c{i}' for i in range(10)], 10.0, thresholds=[0.5], fusion_strategy=(1,))
    det = RecordingDetector(model, post['bbox'], dec, mel, transform, 10.0, 5.0, batch_windows=8)
    raw = (0.1 * torch.randn(seconds * 44100, generator=torch.Generator().manual_seed(44))).cuda()
    rs = det.resampler(44100)
    pre, n = rs([raw])
    pre = pre[0].clone()

    def call(**kw):
        t0 = time.perf_counter()
        det.submit([kw.pop('wave')], ['rec.wav'], **kw).result()
        return (time.perf_counter() - t0) * 1e3

    times = {}
    for key, kw in (('with_sample_rates', dict(wave=raw, sample_rates=44100)), ('at_model_rate', dict(wave=pre))):
        call(**dict(kw))
        t = [call(**dict(kw)) for _ in range(R)]
        times[key] = (float(np.median(t)), min(t), max(t))
    out = torch.empty(n[0], device='cuda')
    us, lo, hi = time_launch(rs.prepare([(raw, raw.numel(), 1)], out, [0], [n[0]]))
    w, d = times['with_sample_rates'], times['at_model_rate']
    ok = us / 1e3 < d[0]
    res['detector'] = dict(seconds=seconds, windows=len(det.plan([n[0]])[1]), with_sample_rates_ms=round(w[0], 2), at_model_rate_ms=round(d[0], 2),
                           ranges_ms=[round(v, 2) for v in (w[1], w[2], d[1], d[2])], resample_launch_ms=round(us / 1e3, 3),
                           resample_cheaper_than_detection=bool(ok))
    print(f'detector    : {seconds} s at 44.1 kHz, {res["detector"]["windows"]} windows: {w[0]:.2f} ms with sample_rates ({w[1]:.2f} .. {w[2]:.2f}), '
          f'{d[0]:.2f} ms already at 16 kHz ({d[1]:.2f} .. {d[2]:.2f}); its resample launch alone {us / 1e3:.3f} ms ({lo / 1e3:.3f} .. {hi / 1e3:.3f}) '
          f'-> resampling costs {"less" if ok else "NOT less"} than detecting', flush=True)


def main():
    from sound_event_detection_transformer_amd.utilities.resample import DeviceResampler
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    hour = 60 if '--short' in sys.argv else 3600
    res = {}
    gen = torch.Generator(device='cuda').manual_seed(2200)
    x = torch.randn(hour * 44100, device='cuda', generator=gen) * 0.1
    launch_case('hour_mono', DeviceResampler(44100, 16000), [(x, x.numel(), 1)], res)
    del x
    x = (torch.randn(hour * 48000, 2, device='cuda', generator=gen) * 3276.8).clamp(-32768, 32767).to(torch.int16)
    launch_case('hour_stereo', DeviceResampler(48000, 16000), [(x, x.shape[0], 2)], res)
    del x
    x = torch.randn(64, 480000, device='cuda', generator=gen) * 0.1
    launch_case('clips', DeviceResampler(48000, 44100), [(c, c.numel(), 1) for c in x], res)
    del x
    detector_case(res, 60 if '--short' in sys.argv else 600)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
