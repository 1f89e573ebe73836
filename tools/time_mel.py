"""The mel front end's one launch (sedt_mel_spectrogram) timed at the sizes a user runs, in ONE process:
  urban  B = 64 ten-second URBAN-SED clips (441000 samples at 44.1 kHz, n_fft 2048, window 1764, hop 882 -> 501 frames x 64 bands)
  dcase  B = 32 ten-second DCASE clips    (160000 samples at 16 kHz,   n_fft 1024, window 1024, hop 323 -> 496 frames x 64 bands)
each from f32 samples and from 16-bit PCM, the batch resident on the device.
Per case it prints
  the launch time: device events around N back-to-back launches (after WARM), median of R such windows;
  the HBM floor: the waveform read once plus the mel written (urban f32: 112.9 + 8.2 = 121.1 MB) over 8 TB/s, and the time as a
    multiple of it - the kernel is bound by LDS traffic and barriers, not by HBM, so this says how far that leaves it;
  the arithmetic it stands for: 2.5 n_fft log2(n_fft/2) flops per frame's FFT (the n_fft/2-point complex transform);
  the clocks read while the launch keeps running (bench.clocks_under_load);
  as orientation, the same batch through the float32 CPU pipeline: scipy.fft.rfft on windowed frames and a dense filterbank
    product, clips spread over 16 worker threads (scipy releases the GIL inside the transform).
    python tools/time_mel.py [--no-cpu]
Kernel times (without launch gaps) come from a trace of the same run, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o mel -- python tools/time_mel.py --no-cpu"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
N, WARM, R = 50, 10, 7
HBM_TBS = 8.0
CASES = {'urban': (64, 441000), 'dcase': (32, 160000)}


def cpu_pipeline(waves, m, workers=16):
    """float32 on the host: reflect pad, frames, window, scipy.fft.rfft, magnitude, dense filterbank; seconds for the batch"""
    import concurrent.futures
    import scipy.fft
    from sound_event_detection_transformer_amd.utilities.mel import expand_filterbank
    W = expand_filterbank(m.tables, m.n_fft).T.copy()
    win, N_, hop = m.tables.window, m.n_fft, m.hop

    def one(y):
        yp = np.pad(y, N_ // 2, mode='reflect')
        idx = np.arange(1 + len(y) // hop)[:, None] * hop + np.arange(N_)[None, :]
        return np.abs(scipy.fft.rfft(yp[idx] * win, axis=1)) @ W

    with concurrent.futures.ThreadPoolExecutor(workers) as ex:
        list(ex.map(one, waves[:workers]))                     # warm
        t0 = time.perf_counter()
        out = list(ex.map(one, waves))
        return time.perf_counter() - t0, out


def main():
    import bench
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram, frames_of
    res = {}
    for name, (B, n) in CASES.items():
        m = DeviceMelSpectrogram.urbansed() if name == 'urban' else DeviceMelSpectrogram.dcase()
        gen = torch.Generator().manual_seed(2100)
        host = torch.randn(B, n, generator=gen) * 0.1
        T = frames_of(n, m.hop)
        out = torch.empty(B, T, 64, device='cuda')
        for dtype in ('f32', 'i16'):
            wave = host.cuda() if dtype == 'f32' else (host * 32768).clamp(-32768, 32767).to(torch.int16).cuda()
            for _ in range(WARM):
                m(wave, out=out)
            torch.cuda.synchronize()
            windows = []
            for _ in range(R):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(N):
                    m(wave, out=out)
                e1.record()
                e1.synchronize()
                windows.append(e0.elapsed_time(e1) * 1e3 / N)
            us = float(np.median(windows))
            mb = (wave.numel() * wave.element_size() + out.numel() * 4) / 1e6
            floor_us = mb / HBM_TBS
            gflop = B * T * 2.5 * m.n_fft * np.log2(m.n_fft / 2) / 1e9
            clocks = bench.clocks_under_load(lambda: m(wave, out=out))
            key = f'{name}_{dtype}'
            res[key] = dict(B=B, samples=n, frames=T, launch_us=round(us, 1), min_us=round(min(windows), 1), max_us=round(max(windows), 1),
                            hbm_mb=round(mb, 1), hbm_floor_us=round(floor_us, 1), times_floor=round(us / floor_us, 1),
                            fft_gflop=round(gflop, 2), fft_tflops=round(gflop / us * 1e3, 2), clips_per_s=round(B / us * 1e6),
                            clocks=clocks)
            print(f'{key:10s}: {us:8.1f} us per launch (windows {min(windows):.1f} .. {max(windows):.1f}), {mb:6.1f} MB -> HBM floor '
                  f'{floor_us:5.1f} us, x{us / floor_us:.1f}; FFT {gflop:.2f} GFLOP = {gflop / us * 1e3:.2f} TFLOP/s; '
                  f'{B / us * 1e6:,.0f} clips/s; clocks {clocks}', flush=True)
        if '--no-cpu' not in sys.argv:
            waves = list(host.numpy())
            sec, ref = cpu_pipeline(waves, m)
            got32, _ = m(host.cuda())
            err = max(float(np.abs(got32[i].cpu().numpy() - ref[i]).max() / ref[i].max()) for i in (0, B - 1))
            res[f'{name}_cpu'] = dict(workers=16, batch_ms=round(sec * 1e3, 1), per_clip_ms=round(sec * 1e3 / B, 2), max_diff_of_max=err)
            print(f'{name} CPU   : {sec * 1e3:8.1f} ms for the batch on 16 threads ({sec * 1e3 / B:.2f} ms per clip of wall time); device vs '
                  f'this f32 pipeline: {err:.1e} of the maximum', flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
