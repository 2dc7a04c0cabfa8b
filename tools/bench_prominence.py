"""The prominence meter on the MI355X: its three kernels one by one, the track call and ``measure`` end to end, beside the front ends
it sits behind.  Prints one JSON line.

One batch (default 32 utterances of 160 000 samples, 10 s at 16 kHz: 626 frames each; five-word harmonic signals with a stressed
word, tests/test_gpu_prominence.py's generator repeated) through ``ProminenceMeter.measure`` with given durations - resampler check,
STFT, tts_frame_energy, the pitch tracker, the three launches, the rows to the host - and through its parts on buffers made once:
``tts_prominence_channels``, ``tts_prominence_cwt``, ``tts_prominence_units``, ``measure_tracks`` (uploads, three launches, rows to
the host), and for context the pitch tracker and the STFT with the frame energy alone.  Device time from HIP events around --reps
back-to-back calls, median (min, max) of --rounds such windows after --warmup calls.

    python tools/bench_prominence.py --out profiles/prominence_bench.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, capi, prominence, prosody
from tests import pitch_ref


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


def utterance(seed, frames):
    """Words of 25 frames with 6 quiet frames around them, one of them 30 % higher and 1.5 times louder, to `frames` frames."""
    rng = np.random.default_rng(seed)
    durations, k = [6], 0
    while sum(durations) + 31 <= frames:
        durations += [25, 6]
    durations[-1] += frames - sum(durations)
    words = (len(durations) - 1) // 2
    stressed = int(rng.integers(words))
    hz, level = [], []
    for k, d in enumerate(durations):
        word = (k - 1) // 2 if k % 2 == 1 else None
        hz += [120.0 * (1.3 if word == stressed else 1.0)] * (256 * d)
        level += [0.0 if word is None else (1.5 if word == stressed else 1.0)] * (256 * d)
    wave = pitch_ref.harmonic(np.asarray(hz), rng, noise=0.0) * np.asarray(level) + 0.0005 * rng.standard_normal(len(hz))
    feats = np.zeros((len(durations), 62), dtype=np.float32)
    feats[1::2, prosody.F_PHONEME] = 1.0
    return wave.astype(np.float32), feats, np.asarray(durations), stressed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=625)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prominence.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B = args.batch
    m = prominence.ProminenceMeter(dev)
    waves, feats, durations, stressed = zip(*[utterance(700 + u, args.frames) for u in range(B)])
    waves, feats, durations = list(waves), list(feats), list(durations)

    rows = {"measure": windows(lambda: m.measure(waves, 16000, feats, durations=durations), dev, args)}
    reports = m.measure(waves, 16000, feats, durations=durations)
    found = [int(np.argmax(r[:, 0])) for r in reports]
    tr = m.last
    rows["measure_tracks"] = windows(lambda: m.measure_tracks(tr["f0"], tr["energy"], tr["phoneme_frames"], tr["units"]), dev, args)
    frames, phones, units = prominence.check_tracks(tr["f0"], tr["energy"], tr["phoneme_frames"], tr["units"])
    utts, phones_h, units_h = m.layout(frames, phones, units)
    f0_d = torch.from_numpy(np.concatenate(tr["f0"])).to(dev)
    e_d = torch.cat([e.reshape(-1) for e in tr["energy"]]).contiguous()
    x = m.channels(f0_d, e_d, utts, phones_h)
    w = m.cwt(x, utts)
    rows["tts_prominence_channels"] = windows(lambda: m.channels(f0_d, e_d, utts, phones_h), dev, args)
    rows["tts_prominence_cwt"] = windows(lambda: m.cwt(x, utts), dev, args)
    rows["tts_prominence_units"] = windows(lambda: m.unit_rows(w, utts, units_h), dev, args)
    rows["pitch_tracker"] = windows(lambda: m._tracker.track(tr["waves16"]), dev, args)

    def stft_energy():
        spec, rag = align.batched_spectra(m.ops, m._logmel, tr["waves16"])
        energy = torch.empty(rag.total_rows, dtype=torch.float32, device=dev)
        capi.check(m.lib.tts_frame_energy(spec.data_ptr(), 2 * m._logmel.bins, m._logmel.bins, energy.data_ptr(), rag.total_rows, m.ops.stream()),
                   "tts_frame_energy")

    rows["stft_and_frame_energy"] = windows(stft_energy, dev, args)
    res = {"metric": "prominence_us_per_batch", "utterances": B, "frames": int(frames[0]), "words": int(len(units[0])), "reps": args.reps,
           "rounds": args.rounds, "times": rows, "stressed_word_found": int(sum(a == b for a, b in zip(found, stressed))),
           "gpu": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
