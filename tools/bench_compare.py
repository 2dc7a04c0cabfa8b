"""Comparing renditions on the MI355X (compare.SpeechComparator): a batch (default 32 pairs of 10.2 s waves, about 640 x 640 frames)
and one pair at the cap (4096 x 4096 frames of seeded cepstra).  Prints one JSON line: ms per call of compare() as a caller sees
it (median of --steps on a host clock that ends in the device-to-host copies), the time of each stage from HIP events around
--reps back-to-back launches - log-mel front end, cepstra, warping, sums along the path, for the batch and for the pair at the
cap - and what the float64 restatement (tests/compare_ref.py, numpy by anti-diagonals) takes on the host for one pair of each size.

    python tools/bench_compare.py --steps 10 --warmup 2 --out profiles/compare_bench.json
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
from ims_toucan_prosody_variance_amd import align, compare
from tests import compare_ref as cr
from tools.bench_pitch import event_ms, recording


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_compare.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n = args.pairs, int(round(args.seconds * compare.SR))
    peak = lambda w: w / np.abs(w).max()
    # side a is another rendition of b's contour: its own seed, 3 % longer
    wb = [peak(recording(300 + u, n)) for u in range(B)]
    wa = [peak(recording(500 + u, int(1.03 * n))) for u in range(B)]
    cmp = compare.SpeechComparator(dev)
    for _ in range(args.warmup):
        res = cmp.compare(wa, wb, compare.SR)
    wall = {}
    for name, f0 in (("track", "track"), ("no_f0", None)):
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            cmp.compare(wa, wb, compare.SR, f0=f0)
            times.append((time.perf_counter() - t0) * 1e3)
        wall[name] = float(np.median(times))

    # the stages of the batch
    def front():
        spec, rag = align.batched_spectra(cmp.ops, cmp.logmel, wa + wb)
        return align.batched_log_mel(cmp.ops, cmp.logmel, spec, rag), rag
    ms_front = event_ms(front, args.reps)  # with its upload
    mel, rag = front()
    rows = torch.from_numpy(np.concatenate([np.arange(b, b + k, dtype=np.int32) for b, k in zip(rag.begins, rag.lengths)])).to(dev)
    ms_cep = event_ms(lambda: cmp.mel_cepstra(mel, rows), args.reps)
    cep, frames = cmp.cepstra(wa + wb)
    fa, fb = frames[:B], frames[B:]
    ca, cb = cep[:sum(fa)], cep[sum(fa):]
    stages = {}
    for name, force in (("lds_or_scratch", False), ("scratch", True)):
        stages["ms_dtw_" + name] = event_ms(lambda: cmp._dtw(ca, fa, cb, fb, force), args.reps)
    cost, path, path_len, _ = cmp._dtw(ca, fa, cb, fb)
    f0 = torch.full((max(sum(fa), sum(fb)),), 150.0, device=dev)
    stages["ms_path_sums"] = event_ms(lambda: cmp._path_sums(ca, fa, cb, fb, path, path_len, f0[:sum(fa)], f0[:sum(fb)]), args.reps)

    # one pair at the cap, seeded like the test cases
    T = compare.MAX_FRAMES
    rng = np.random.default_rng(1)
    big_a = rng.standard_normal((T, 13)).astype(np.float32)
    big_b = (big_a[np.clip(np.round(np.linspace(0, T - 1, T) + 40 * np.sin(np.arange(T) / 300.0)), 0, T - 1).astype(np.int64)]
             + 0.3 * rng.standard_normal((T, 13))).astype(np.float32)
    da, db = torch.from_numpy(big_a).to(dev), torch.from_numpy(big_b).to(dev)
    cmp._dtw(da, [T], db, [T])
    ms_big = event_ms(lambda: cmp._dtw(da, [T], db, [T]), max(1, args.reps // 2))
    big_cost, big_path = cmp.dtw(da, [T], db, [T])

    # the restatement on the host
    a0, b0 = ca[:fa[0]].cpu().numpy(), cb[:fb[0]].cpu().numpy()
    t0 = time.perf_counter()
    ref0 = cr.dtw(a0, b0)
    host_small = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref_big = cr.dtw(big_a, big_b)
    host_big = (time.perf_counter() - t0) * 1e3
    p0 = path.cpu().numpy()[:int(path_len[0])]
    out = {
        "metric": "compare_ms_per_batch", "pairs": B, "seconds": args.seconds, "frames_a": fa[0], "frames_b": fb[0], "steps": args.steps,
        "reps": args.reps, "launches": cmp.last_launches,
        "ms_compare_track": round(wall["track"], 3), "ms_compare_no_f0": round(wall["no_f0"], 3),
        "pairs_per_s_track": round(1e3 * B / wall["track"], 1),
        "ms_log_mel": round(ms_front, 4), "ms_mel_cepstra": round(ms_cep, 4), **{k: round(v, 4) for k, v in stages.items()},
        "cells": int(sum(x * y for x, y in zip(fa, fb))),
        "gcells_per_s_dtw": round(sum(x * y for x, y in zip(fa, fb)) / (stages["ms_dtw_lds_or_scratch"] * 1e6), 3),
        "ms_dtw_4096x4096": round(ms_big, 3), "gcells_per_s_dtw_4096x4096": round(T * T / (ms_big * 1e6), 3),
        "host_restatement_ms_pair0": round(host_small, 1), "host_restatement_ms_4096x4096": round(host_big, 1),
        "path_equals_restatement_pair0": bool(np.array_equal(p0, ref0["path"])),
        "path_equals_restatement_4096x4096": bool(np.array_equal(big_path[0], ref_big["path"])),
        "cost_rel_err_4096x4096": float(abs(big_cost[0] - ref_big["cost"]) / ref_big["cost"]),
        "restatement_gap_pair0": ref0["gap"], "restatement_gap_4096x4096": ref_big["gap"],
        "mcd_db_mean": round(float(np.mean([r["mcd_db"] for r in res])), 3),
        "gpu": torch.cuda.get_device_name(dev),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
