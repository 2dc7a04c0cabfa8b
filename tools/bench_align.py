"""Prosody extraction throughput on the MI355X: one batch of aligner work (default 32 utterances of 10 s = 625 frames, ~100 tokens
each) through align.AlignerEngine - conv stack and projections, the per-step LSTM recurrence, MAS with the duration repair - plus
the frame energy and token averages of align.ProsodyExtractor.  Prints one JSON line: ms per batch (median of --steps) and its split
into convs / LSTM / MAS / energy from HIP events, and the LSTM's time per step.

    python tools/bench_align.py --batch 32 --frames 625 --tokens 100 --steps 5 --warmup 2
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
from ims_toucan_prosody_variance_amd import align, fixture_weights as fw, phonemes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=625)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, L = args.batch, args.frames, args.tokens
    ex = align.ProsodyExtractor(fw.aligner_state_dict(), dev, timing=True)
    syms = sorted(s for s, v in phonemes.phone_table().items() if v[15] == 1 and v[21] == 0)
    feats = []
    for u in range(B):
        idx = (fw.uniform01("bench.syms%d" % u, L, 5) * len(syms)).astype(int)
        feats.append(phonemes.phones_to_features("".join(syms[i] for i in idx), handle_missing=False))
    waves = [fw.normal("bench.wave%d" % u, ((T - 1) * 256,), 6, 0.2) for u in range(B)]  # 1 + n // 256 = T frames
    mels = [fw.aligner_spectrogram(100 + u, T) for u in range(B)]
    f0 = [100.0 + 50.0 * fw.uniform01("bench.f0%d" % u, T, 7).astype(np.float32) for u in range(B)]
    for _ in range(args.warmup):
        ex.extract(feats, waves, f0=f0, mels=mels)
    wall, phases = [], []
    for _ in range(args.steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ex.extract(feats, waves, f0=f0, mels=mels)  # ends with a device-to-host copy of the results
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(dict(ex.aligner.last_phase_ms))
    med = lambda k: float(np.median([p.get(k, 0.0) for p in phases]))
    out = {
        "metric": "align_ms_per_batch", "batch": B, "frames": T, "tokens": L, "steps": args.steps,
        "ms_per_batch": round(float(np.median(wall)), 3),
        "ms_convs": round(med("convs"), 3), "ms_lstm": round(med("lstm"), 3), "ms_mas": round(med("mas"), 3),
        "ms_energy": round(med("energy"), 3),
        "lstm_us_per_step": round(1e3 * med("lstm") / T, 2),
        "utterances_per_s": round(1e3 * B / float(np.median(wall)), 1),
        "gpu": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
