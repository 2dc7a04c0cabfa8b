"""Speech-activity measurement (ITU-T P.56) on the MI355X beside the loudness meter on the same batch.  Prints one JSON line.

One batch (default 32 utterances of 240 000 samples, 10 s at 24 kHz, seeded noise bursts with pauses) through
``SpeechActivity.measure`` (tts_activity_envelope: three launches, tts_activity_level, tts_activity_runs: two launches),
``SpeechActivity.normalize`` (the same, the gain, and the level of the output measured again) and ``LoudnessMeter.measure``, each
with the allocation of its workspace and the upload of the spans that belong to a call: device time from HIP events around --reps
back-to-back calls, median (min, max) of --rounds such windows after --warmup calls.  A record, not a gate.

    python tools/bench_activity.py --out profiles/activity_bench.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import activity, loudness


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
    ap.add_argument("--samples", type=int, default=240000)
    ap.add_argument("--rate", type=int, default=24000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_activity.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n, sr = args.batch, args.samples, args.rate
    rng = np.random.default_rng(7)
    # noise, one second on and half a second off
    gate = (np.arange(B * n) % (3 * sr // 2) < sr).astype(np.float32)
    wave = torch.from_numpy(np.clip(0.1 * rng.standard_normal(B * n), -1, 1).astype(np.float32) * gate).to(dev)
    spans = [(b * n, n) for b in range(B)]
    out = torch.empty_like(wave)
    act, loud = activity.SpeechActivity(dev), loudness.LoudnessMeter(dev)
    rows = {"activity_measure": windows(lambda: act.measure(wave, spans, sr), dev, args),
            "activity_normalize": windows(lambda: act.normalize(wave, spans, sr, -26.0, -1.0, out=out), dev, args),
            "loudness_measure": windows(lambda: loud.measure(wave, spans, sr), dev, args),
            "loudness_normalize": windows(lambda: loud.normalize(wave, spans, sr, -23.0, -1.0, out=out), dev, args)}
    s = act.measure(wave, spans, sr).cpu().numpy()
    res = {"metric": "activity_measure_us_per_batch", "batch": B, "samples": n, "rate": sr, "reps": args.reps, "rounds": args.rounds, "times": rows,
           "active_db_mean": round(float(s[:, 0].mean()), 4), "activity_mean": round(float(s[:, 2].mean()), 4),
           "runs_mean": round(float(act.last_counts[:, 15].double().mean()), 2), "gpu": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
