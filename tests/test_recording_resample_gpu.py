"""GPU: RecordingDetector with ``sample_rates`` - recordings at their own rates, stereo PCM among them, down-mixed and resampled on the
device straight into the detector's flat staged vector.  Two recordings in one call, a 48 kHz stereo int16 one of about 23 s and a
44.1 kHz mono f32 one shorter than a window, must give records, tags, plan, rows and RecordingPredictions equal, bit for bit, to those
of the same detector fed the DeviceResampler outputs as mono recordings at mel.sr.  A second call replays the cached resamplers and
the graph.  Without sample_rates a 2-D input still raises the error it raised before."""
import numpy as np
import pytest
import torch

from oracle import sedt_oracle as O

pytestmark = pytest.mark.gpu

C2_CLASSES = 10
WIN, HOP, SR = 160000, 80000, 16000


def _c2_model():
    from sound_event_detection_transformer_amd import runtime, sedt
    runtime.set_compute_dtype('f32')
    runtime.manual_seed(5)
    model, crit, post = sedt.build_model(sedt.default_args(enc_layers=3, num_queries=10, dec_at=True, dropout=0.0))
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), 2020))
    model.cuda().eval()
    crit.cuda()
    return model, crit, post['bbox']


def _same_predictions(a, b, fusion, K):
    for m in fusion:
        for k in range(K):
            ta, tb = a[m].at(k), b[m].at(k)
            assert a[m].to_rows(k) == b[m].to_rows(k), (m, k)
            assert set(ta) == set(tb) and all(np.array_equal(ta[c], tb[c]) for c in ta), (m, k)


def test_detector_resamples_on_the_device():
    from sound_event_detection_transformer_amd import lib, runtime
    from sound_event_detection_transformer_amd.engine import detect_step, detect_recordings
    from sound_event_detection_transformer_amd.utilities.mel import DeviceMelSpectrogram
    from sound_event_detection_transformer_amd.utilities.predictions import EventDecoder
    from sound_event_detection_transformer_amd.utilities.recording import RecordingDetector
    from sound_event_detection_transformer_amd.utilities.resample import DeviceResampler
    from sound_event_detection_transformer_amd.utilities.transforms import DeviceBoxTransform
    model, _, post = _c2_model()
    try:
        B, fusion, C = 4, (1, 2), C2_CLASSES
        labels = [f'c{i}' for i in range(C)]
        mel, transform = DeviceMelSpectrogram.dcase(), DeviceBoxTransform(500)
        gen = torch.Generator().manual_seed(48)
        stereo = (0.1 * torch.randn(23 * 48000 + 1234, 2, generator=gen) * 32768).clamp(-32768, 32767).to(torch.int16).numpy()
        mono = (0.1 * torch.randn(5 * 44100 + 77, generator=gen)).numpy()
        names = ['field.wav', 'clip.wav']
        # the yardstick's input: the resampler's own outputs as mono recordings at mel.sr
        ra, na = DeviceResampler(48000, SR)([stereo])
        rb, nb = DeviceResampler(44100, SR)([mono])
        assert na == [-(-len(stereo) // 3)] and nb == [-(-len(mono) * 160 // 441)] and nb[0] < WIN < na[0]
        plain = [ra[0].clone(), rb[0].clone()]
        amp, nframes = mel(torch.stack([plain[0][s:s + WIN] for s in (0, HOP, 2 * HOP, na[0] - WIN)]))
        sizes = torch.full((B,), 10.0).cuda()
        scores = detect_step(model, post, transform(amp, nframes=nframes), sizes, fusion)[1][1][0].cpu().numpy()
        grid = [float(np.quantile(scores, q)) for q in (0.5, 0.8)]
        dec = EventDecoder(labels, 10.0, thresholds=grid, fusion_strategy=fusion)
        det = RecordingDetector(model, post, dec, mel, transform, 10.0, 5.0, batch_windows=B, merge_gap=0.25)

        want_rec, want_tags, want_plan = det.records(plain)
        want_rec = {m: t.clone() for m, t in want_rec.items()}
        want_tags = want_tags.clone()
        want, want_wt = det(plain, names)
        with lib.launch_log() as log:
            rec, tags, plan = det.records([stereo, mono], sample_rates=[48000, 44100])
        assert log['resample'] == 2                                          # one launch per source rate
        assert plan[0].tolist() == want_plan[0].tolist() == [0, 4, 5] and all(np.array_equal(a, b) for a, b in zip(plan, want_plan))
        assert plan[3].tolist() == [na[0] / SR, nb[0] / SR]
        assert all(torch.equal(rec[m], want_rec[m]) for m in fusion) and torch.equal(tags, want_tags)
        assert sum(int(rec[m][:, :, 0].sum()) for m in fusion) > 10          # the records are not empty
        got, wt = det([stereo, mono], names, sample_rates=[48000, 44100])
        _same_predictions(got, want, fusion, len(grid))
        assert np.array_equal(wt.tags, want_wt.tags) and wt.start.tolist() == want_wt.start.tolist() and wt.recording.tolist() == [0] * 4 + [1]
        assert len(got[1].to_rows(0)) > 3
        # a second call: the cached resamplers, the captured graph; device tensors as input; two calls in flight
        cached = dict(det._resamplers)
        assert sorted(cached) == [44100, 48000]
        first = det.submit([torch.from_numpy(stereo).cuda(), mono], names, sample_rates=[48000, 44100])
        second = det.submit([stereo, torch.from_numpy(mono).cuda()], names, sample_rates=[48000, 44100])
        for again in (first.result()[0], second.result()[0]):
            _same_predictions(again, want, fusion, len(grid))
        assert det._resamplers == cached and all(det._resamplers[r] is cached[r] for r in cached)
        # one rate for all: a recording already at mel.sr goes through the identity plan and gives the plain path's records
        same, _ = det(plain, names, sample_rates=SR)
        _same_predictions(same, want, fusion, len(grid))
        # the one-call form
        once, _ = detect_recordings(model, post, dec, mel, transform, [stereo, mono], names, 10.0, 5.0, batch_windows=B, merge_gap=0.25,
                                    graphed=False, sample_rates=[48000, 44100])
        _same_predictions(once, want, fusion, len(grid))
        # without sample_rates nothing changes: a 2-D input is refused as before
        with pytest.raises(ValueError, match='mono waveforms expected: every recording 1-D'):
            det([stereo], ['field.wav'])
        with pytest.raises(ValueError, match='one rate, or one per recording'):
            det([stereo, mono], names, sample_rates=[48000])
    finally:
        runtime.set_compute_dtype('bf16')
