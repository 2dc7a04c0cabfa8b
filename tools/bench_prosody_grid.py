"""A prosody grid as ragged batches against one pass per setting, on the MI355X.  Prints one JSON line.

One sentence of 128 phonemes (seeded synthetic features, predicted durations, BigVGAN, fixture weights, --precision, default bf16)
at a 3 x 3 x 3 grid of duration / pitch-variance / energy-variance scales, 27 variants:

  grid     ONE ``synthesize_grid`` call: the variants as a ragged batch with per-utterance scales (tts_control_and_regulate_v);
  scalar   the same 27 variants as 27 scalar calls on the same commit, each the sentence alone with its four scalars
           (``synthesize_batch`` of the one feature tensor: the path ``forward`` takes behind its text front end).

Both in alternation, --steps times each after --warmup rounds, on a host clock that ends in a device synchronise with the waveforms
left on the device.  Reported: wall time per variant of both ways (median, min, max over the rounds) and their ratio.

    python tools/bench_prosody_grid.py --out profiles/prosody_grid_bench.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phonemes", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--durations", type=float, nargs="+", default=[0.9, 1.0, 1.1])
    ap.add_argument("--pitch", type=float, nargs="+", default=[0.7, 1.0, 1.3])
    ap.add_argument("--energy", type=float, nargs="+", default=[0.7, 1.0, 1.3])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prosody_grid.py measures on the MI355X"
    os.environ["TOUCAN_PRECISION"] = args.precision  # (read by the interface's constructor)
    import ims_toucan_prosody_variance_amd  # noqa: F401
    from ims_toucan_prosody_variance_amd import interface, prosody, synthetic as syn

    dev = torch.device("cuda:0")
    models_dir = interface.MODELS_DIR
    with tempfile.TemporaryDirectory() as tmp:  # the constructor reads the checkpoints; nothing is read from there afterwards
        interface.write_fixture_checkpoints(tmp, n_lang=20)
        interface.MODELS_DIR = tmp
        try:
            tts = interface.ToucanTTSInterface(device=str(dev), tts_model_path="Meta", faster_vocoder=False)
        finally:
            interface.MODELS_DIR = models_dir
    tts.set_language("en")
    feats = torch.from_numpy(syn.utterance_features(0, args.phonemes))
    variants = prosody.grid(args.durations, args.pitch, args.energy)

    def grid():
        out = tts.synthesize_grid(feats, args.durations, args.pitch, args.energy)
        torch.cuda.synchronize(dev)
        return out

    def scalar():
        out = [tts.synthesize_batch([feats], duration_scaling_factor=d, pitch_variance_scale=p, energy_variance_scale=e,
                                    pause_duration_scaling_factor=pause)[0] for d, p, e, pause in variants]
        torch.cuda.synchronize(dev)
        return out

    ways = {"grid": grid, "scalar": scalar}
    for _ in range(args.warmup):
        outs = {k: f() for k, f in ways.items()}
    frames = [r["frames"] for r in outs["grid"]]
    assert [w.numel() for w in outs["scalar"]] == [384 * n for n in frames]  # (the same variants: the durations do not depend on the batch)
    realised = [round(float(r["stats_after"][2]) / float(r["stats_before"][2]), 4) for r in outs["grid"]]
    outs = None
    ms = {k: [] for k in ways}
    for _ in range(args.steps):
        for k, f in ways.items():  # alternating: each round times both ways once
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
    n = len(variants)
    per = {k: {"median": round(float(np.median(v)) / n, 3), "min": round(min(v) / n, 3), "max": round(max(v) / n, 3)} for k, v in ms.items()}
    out = {"metric": "prosody_grid_ms_per_variant", "variants": n, "phonemes": args.phonemes, "precision": args.precision, "vocoder": "bigvgan",
           "frames_per_variant": frames, "realised_pitch_variance_ratio": realised, "ms": ms, "ms_per_variant": per,
           "scalar_over_grid": round(per["scalar"]["median"] / per["grid"]["median"], 3),
           "grid_below_scalar_in_every_round": all(a < b for a, b in zip(ms["grid"], ms["scalar"])), "gpu": torch.cuda.get_device_name(dev)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
