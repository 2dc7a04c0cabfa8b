"""True peak, loudness range, the gain under a true-peak ceiling and the limiter on the MI355X.  Prints one JSON line.

One batch (default 32 utterances of 245 760 samples, 10.24 s at 24 kHz: the waveform of the benchmark batch of bench.py, here
seeded noise) through ``DeliveryMeter.measure``, through ``DeliveryMeter.normalize`` with the one gain and with the limiter - with
the allocation of the workspace and the upload of the spans that belong to a call - through ``LoudnessMeter.normalize`` as the
yardstick, and through the four entries one by one: device time from HIP events around --reps back-to-back calls, median (min, max)
of --rounds such windows after --warmup calls.  The target is one the batch cannot reach under the ceiling, so the gain is held by
the true peak and the limiter limits.  --step-ms takes the ms_per_step of bench.py measured in the same job and reports every
figure as a share of a step.

    python tools/bench_truepeak.py --step-ms 32.9 --out profiles/truepeak_bench.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import loudness, truepeak


def windows(fn, dev, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / args.reps)
    return {"us": round(float(np.median(out)), 2), "us_min": round(min(out), 2), "us_max": round(max(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=245760)
    ap.add_argument("--rate", type=int, default=24000)
    ap.add_argument("--target", type=float, default=-10.0, help="LUFS; past what 0.1 sigma noise reaches under -1 dBTP")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-ms", type=float, default=None, help="ms_per_step of bench.py in the same job")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_truepeak.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n, sr = args.batch, args.samples, args.rate
    S, F = loudness.segment_samples(sr), truepeak.oversampling(sr)
    m = truepeak.DeliveryMeter(dev)
    rng = np.random.default_rng(7)
    wave = torch.from_numpy(np.clip(0.1 * rng.standard_normal(B * n), -1, 1).astype(np.float32)).to(dev)
    spans = [(b * n, n) for b in range(B)]
    out = torch.empty_like(wave)
    rows = {"loudness_normalize": windows(lambda: m.loudness.normalize(wave, spans, sr, args.target, -1.0, out=out), dev, args),
            "measure": windows(lambda: m.measure(wave, spans, sr), dev, args),
            "normalize": windows(lambda: m.normalize(wave, spans, sr, args.target, -1.0, -1.0, out=out), dev, args)}
    steps = m.last_steps.cpu().numpy()
    rows["normalize_limiter"] = windows(lambda: m.normalize(wave, spans, sr, args.target, -1.0, -1.0, limiter=True, out=out), dev, args)
    lim = m.last_limiter.cpu().numpy()

    # the entries one by one, on buffers made once
    host, spans_d = m._rows(wave, spans)
    segs = -(-n // S)
    stats = m.loudness._measure(wave, host, spans_d, sr, args.target, -1.0)
    energy, peak = m.loudness.last_segments
    tp = torch.empty(B, dtype=torch.float32, device=dev)
    rng_rows = torch.empty((B, len(truepeak.RANGE_COLUMNS)), dtype=torch.float64, device=dev)
    lim_rows = torch.empty((B, len(truepeak.LIMITER_COLUMNS)), dtype=torch.float64, device=dev)
    taken, work = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((2, B), dtype=torch.int32, device=dev)
    mm, g = torch.empty_like(wave), torch.empty(wave.shape, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    tab = m.table(sr)

    def ok(rc):
        assert rc == 0, m.lib.tts_last_error()

    rows["tts_true_peak"] = windows(lambda: ok(m.lib.tts_true_peak(wave.data_ptr(), wave.numel(), spans_d.data_ptr(), host.ctypes.data, B, n, tab.data_ptr(),
                                                                    F, None, tp.data_ptr(), st)), dev, args)
    rows["tts_loudness_range"] = windows(lambda: ok(m.lib.tts_loudness_range(energy.data_ptr(), peak.data_ptr(), tp.data_ptr(), wave.numel(), spans_d.data_ptr(),
                                                                              B, S, segs, None, rng_rows.data_ptr(), st)), dev, args)
    fresh = stats.clone()

    def gain():
        stats.copy_(fresh)  # (the entry rewrites the gain it reads)
        ok(m.lib.tts_truepeak_gain(wave.data_ptr(), wave.numel(), spans_d.data_ptr(), host.ctypes.data, B, tab.data_ptr(), F, tp.data_ptr(), -1.0,
                                   stats.data_ptr(), taken.data_ptr(), work.data_ptr(), st))

    rows["tts_truepeak_gain"] = windows(gain, dev, args)
    stats.copy_(fresh)
    rows["tts_limit_true_peak"] = windows(lambda: ok(m.lib.tts_limit_true_peak(wave.data_ptr(), wave.numel(), spans_d.data_ptr(), host.ctypes.data, B, n, S,
                                                                                tab.data_ptr(), F, stats.data_ptr(), args.target, -1.0, -1.0, mm.data_ptr(),
                                                                                g.data_ptr(), tp.data_ptr(), lim_rows.data_ptr(), out.data_ptr(), st)), dev, args)
    r = rng_rows.cpu().numpy()
    res = {"metric": "truepeak_us_per_batch", "batch": B, "samples": n, "rate": sr, "factor": F, "target_lufs": args.target, "reps": args.reps,
           "rounds": args.rounds, "times": rows, "gain_steps": [int(steps.min()), int(steps.max())], "trim_db_worst": round(float(lim[:, 7].min()), 6),
           "over_db_worst": round(float(lim[:, 3].max()), 6), "true_peak_dbtp_mean": round(float(r[:, 1].mean()), 4),
           "gpu": torch.cuda.get_device_name(dev)}
    if args.step_ms:
        res["bench_ms_per_step"] = args.step_ms
        res["share_of_step"] = {k: round(v["us"] / 1e3 / args.step_ms, 5) for k, v in rows.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
