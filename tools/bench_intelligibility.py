"""STOI and ESTOI on the MI355X: the whole call and its kernels one by one.  Prints one JSON line.

One batch (default 32 pairs of 102 400 samples, 10.24 s at 10 kHz: seeded modulated noise against itself plus noise at 5 dB SNR)
through ``Intelligibility.score_packed`` - with the allocations, the small uploads and the one copy of the counts and totals to the
host that belong to a call - and through its parts on buffers made once: ``tts_stoi_frame_energy`` + ``tts_stoi_select``,
``tts_stoi_gather``, the DFT (``tts_conv1d`` in fp32), ``tts_stoi_bands``, ``tts_stoi_segments`` + ``tts_stoi_reduce``.  Device time
from HIP events around --reps back-to-back calls, median (min, max) of --rounds such windows after --warmup calls.  For context, the
wall time of the float64 numpy restatement (tests/intelligibility_ref.py) on one pair on the host, times the batch.

    python tools/bench_intelligibility.py --out profiles/intelligibility_bench.json
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
from ims_toucan_prosody_variance_amd import capi, intelligibility
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import intelligibility_ref as ir


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
    ap.add_argument("--samples", type=int, default=102400)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_intelligibility.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n = args.batch, args.samples
    m = intelligibility.Intelligibility(dev)
    waves = []
    for p in range(B):
        x = ir.speech_like(n, 500 + p)
        waves += [x, ir.at_snr(x, 5.0, 600 + p)]
    packed = torch.from_numpy(np.concatenate(waves)).to(dev)  # [x0 y0 x1 y1 ...]
    pairs = np.asarray([(2 * p * n, (2 * p + 1) * n, n) for p in range(B)], dtype=np.int64)
    frames = [intelligibility.frame_count(n)] * B

    rows = {"score_packed": windows(lambda: m.score_packed(packed, pairs), dev, args)}
    first = m.score_packed(packed, pairs)[0]
    kept, counts, max_frames, pairs_d = m.select(packed, pairs)
    buf, row_begin = m.gather(packed, pairs, pairs_d, kept, counts, max_frames)
    lengths, begins = zip(*[(F, int(b)) for F, rb in zip(frames, row_begin) for b in rb])
    rag = Ragged(list(lengths), dev, begins=list(begins))
    spec = m.ops.empty(buf.shape[0], 2 * intelligibility.N_BINS)
    conv = lambda: m.ops.conv(m.basis, buf, spec, rag, compute=capi.COMPUTE_F32, split_k=False)
    conv()
    bands = torch.empty((buf.shape[0], intelligibility.N_BANDS), dtype=torch.float64, device=dev)
    band = lambda: capi.check(m.lib.tts_stoi_bands(spec.data_ptr(), int(spec.stride(0)), buf.shape[0], bands.data_ptr(), m.ops.stream()), "tts_stoi_bands")
    band()
    rows["frame_energy_and_select"] = windows(lambda: m.select(packed, pairs), dev, args)
    rows["tts_stoi_gather"] = windows(lambda: m.gather(packed, pairs, pairs_d, kept, counts, max_frames), dev, args)
    rows["dft_conv"] = windows(conv, dev, args)
    rows["tts_stoi_bands"] = windows(band, dev, args)
    rows["segments_and_reduce"] = windows(lambda: m.tail(bands, row_begin, frames, counts), dev, args)

    t0 = time.perf_counter()
    ref = ir.score(waves[0], waves[1])
    host_s = time.perf_counter() - t0
    res = {"metric": "intelligibility_us_per_batch", "pairs": B, "samples": n, "rate": intelligibility.SR, "frames": frames[0],
           "kept_frames": first["kept_frames"], "segments": first["segments"], "reps": args.reps, "rounds": args.rounds, "times": rows,
           "stoi": first["stoi"], "estoi": first["estoi"], "host_float64_stoi": ref["stoi"], "host_float64_estoi": ref["estoi"],
           "host_float64_restatement_ms_per_pair": round(1e3 * host_s, 2), "host_float64_restatement_ms_per_batch": round(1e3 * host_s * B, 1),
           "gpu": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
