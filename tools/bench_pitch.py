"""Pitch tracking throughput on the MI355X: one batch (default 32 utterances of 10 s at 16 kHz = 621 frames each) through
pitch.PitchTracker.  Prints one JSON line: ms per batch for track() as a caller sees it (upload, three kernels, download; median of
--steps on a host clock that ends in the device-to-host copy), utterances per second from it, and the time of each kernel from HIP
events around --reps back-to-back launches.  The signals are seeded harmonic glides with noise, vibrato and a pause: voiced frames
with a few candidates and noise frames with many, as a recording has.

    python tools/bench_pitch.py --batch 32 --seconds 10 --steps 20 --warmup 3 --out profiles/pitch_bench_b32x10s.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import pitch


def recording(seed, n):
    """Six harmonics on an f0 gliding between two draws from 70 .. 400 Hz with a 3 Hz vibrato, a pause of 15 %, noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / pitch.SR
    fa, fb = rng.uniform(70.0, 400.0, 2)
    phase = 2.0 * np.pi * np.cumsum(fa + (fb - fa) * t / t[-1] + 8.0 * np.sin(2.0 * np.pi * 3.0 * t)) / pitch.SR
    x = sum(rng.uniform(0.3, 1.0) / h * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 7))
    x = 0.1 * x / np.abs(x).max()
    x[int(0.425 * n):int(0.575 * n)] = 0.0
    return (x + 0.002 * rng.standard_normal(n)).astype(np.float32)


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pitch.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n = args.batch, int(round(args.seconds * pitch.SR))
    waves = [recording(100 + u, n) for u in range(B)]
    tr = pitch.PitchTracker(dev)
    for _ in range(args.warmup):
        tracks = tr.track(waves)
    wall = []
    for _ in range(args.steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tr.track(waves)  # ends with the device-to-host copy of f0
        wall.append((time.perf_counter() - t0) * 1e3)
    lay = tr.layout(waves)
    freq, strength, n_cand, _ = tr.candidates(lay)
    ops, lib = tr.ops, tr.ops.lib
    stats = ops.empty(B, 2)
    ms_stats = event_ms(lambda: lib.tts_wave_stats(lay["wave"].data_ptr(), lay["wave_begin"].data_ptr(), lay["n_samples"].data_ptr(), B,
                                                   stats.data_ptr(), ops.stream()), args.reps)
    ms_cand = event_ms(lambda: lib.tts_pitch_candidates(lay["wave"].data_ptr(), lay["wave_begin"].data_ptr(), lay["n_samples"].data_ptr(),
                                                        stats.data_ptr(), lay["frame_begin_d"].data_ptr(), lay["n_frames"].data_ptr(), B,
                                                        max(lay["frames"]), tr.win.data_ptr(), tr.wr.data_ptr(), freq.data_ptr(),
                                                        strength.data_ptr(), n_cand.data_ptr(), None, ops.stream()), args.reps)
    ms_path = event_ms(lambda: tr.path(freq, strength, n_cand, lay["frames"]), args.reps)  # with its small uploads
    rows = lay["rows"]
    products = rows * 3 * 400 * pitch.N_LAGS  # the lag products the candidates kernel forms, zero tail included
    nc = n_cand.cpu().numpy()
    med = float(np.median(wall))
    out = {
        "metric": "pitch_ms_per_batch", "batch": B, "seconds": args.seconds, "frames_per_utterance": lay["frames"][0], "frames": rows,
        "steps": args.steps, "reps": args.reps,
        "ms_per_batch": round(med, 3), "ms_per_batch_min": round(float(np.min(wall)), 3), "ms_per_batch_max": round(float(np.max(wall)), 3),
        "utterances_per_s": round(1e3 * B / med, 1),
        "ms_wave_stats": round(ms_stats, 4), "ms_pitch_candidates": round(ms_cand, 4), "ms_pitch_path": round(ms_path, 4),
        "lag_products": products, "lag_gflops_over_candidates_kernel_time": round(2.0 * products / (ms_cand * 1e6), 1),
        "voiced_candidates_per_frame_mean": round(float(nc.mean() - 1), 2), "voiced_candidates_per_frame_max": int(nc.max() - 1),
        "voiced_frames": int(sum(int((t > 0).sum()) for t in tracks)),
        "gpu": torch.cuda.get_device_name(dev),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
