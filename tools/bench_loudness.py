"""Loudness measurement and normalisation on the MI355X.  Prints one JSON line.

One batch (default 32 utterances of 245 760 samples, 10.24 s at 24 kHz: the waveform of the benchmark batch of bench.py, here
seeded noise) through ``LoudnessMeter.normalize`` - tts_kweight_energy (three launches), tts_loudness_gate, tts_apply_gain, with
the allocation of the workspace and the upload of the spans that belong to a call - and through the three entries one by one:
device time from HIP events around --reps back-to-back calls, median (min, max) of --rounds such windows after --warmup calls.
--step-ms takes the ms_per_step of bench.py measured in the same job and reports the share of a step the normalisation is.

    python tools/bench_loudness.py --step-ms 36.5 --out profiles/loudness_bench.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import loudness


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--step-ms", type=float, default=None, help="ms_per_step of bench.py in the same job")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loudness.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n, sr = args.batch, args.samples, args.rate
    S = loudness.segment_samples(sr)
    m = loudness.LoudnessMeter(dev)
    rng = np.random.default_rng(7)
    wave = torch.from_numpy(np.clip(0.1 * rng.standard_normal(B * n), -1, 1).astype(np.float32)).to(dev)
    spans = [(b * n, n) for b in range(B)]
    out = torch.empty_like(wave)
    rows = {"normalize": windows(lambda: m.normalize(wave, spans, sr, -23.0, -1.0, out=out), dev, args)}

    # the entries one by one, on buffers made once
    host, spans_d = m._rows(wave, spans)
    segs = -(-n // S)
    state = torch.empty((B, segs, 4), dtype=torch.float64, device=dev)
    energy = torch.empty((B, segs), dtype=torch.float64, device=dev)
    peak = torch.empty((B, segs), dtype=torch.float32, device=dev)
    stats = torch.empty((B, 8), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    tab = m.table(sr)

    def ok(rc):
        assert rc == 0, m.lib.tts_last_error()

    rows["tts_kweight_energy"] = windows(lambda: ok(m.lib.tts_kweight_energy(wave.data_ptr(), wave.numel(), spans_d.data_ptr(), host.ctypes.data, B, S,
                                                                              tab.data_ptr(), segs, state.data_ptr(), energy.data_ptr(), peak.data_ptr(), st)), dev, args)
    rows["tts_loudness_gate"] = windows(lambda: ok(m.lib.tts_loudness_gate(energy.data_ptr(), peak.data_ptr(), wave.numel(), spans_d.data_ptr(), B, S, segs,
                                                                            -23.0, -1.0, stats.data_ptr(), st)), dev, args)
    rows["tts_apply_gain"] = windows(lambda: ok(m.lib.tts_apply_gain(wave.data_ptr(), wave.numel(), spans_d.data_ptr(), host.ctypes.data, B, n,
                                                                      stats.data_ptr(), out.data_ptr(), st)), dev, args)
    s = stats.cpu().numpy()
    res = {"metric": "loudness_normalize_us_per_batch", "batch": B, "samples": n, "rate": sr, "segments": B * segs, "reps": args.reps,
           "rounds": args.rounds, "times": rows, "lufs_mean": round(float(s[:, 0].mean()), 4), "gain_mean": round(float(s[:, 6].mean()), 6),
           "gpu": torch.cuda.get_device_name(dev)}
    if args.step_ms:
        res["bench_ms_per_step"] = args.step_ms
        res["normalize_share_of_step"] = round(rows["normalize"]["us"] / 1e3 / args.step_ms, 5)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
