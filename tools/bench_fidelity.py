"""The spectral distances on the MI355X: framing, DFT and tail per resolution, beside the vocoder.  Prints one JSON line.

One batch (default 32 pairs of 245 760 samples, 10.24 s at 24 kHz: the waveform of the benchmark batch of bench.py, here seeded
noise against itself plus 1 % noise) through ``SpectralDistance.distance_packed`` at the reference resolution and at all three -
with the allocations, the uploads of the small tables and the one copy of the totals to the host that belong to a call - and per
resolution through its three parts on buffers made once: ``tts_frame_reflect``, the DFT (``tts_conv1d`` in fp32) and the tail
(``tts_spectral_distance`` + ``tts_spectral_reduce``).  Beside the tail of the reference resolution stands the same mel_l1 composed
from the launches the library had before: ``tts_complex_magnitude``, the mel projection as a conv, ``tts_log10_floor`` and an L1 in
torch (it yields one of the tail's three measures).  Device time from HIP events around --reps back-to-back calls, median (min, max)
of --rounds such windows after --warmup calls.  The yardstick is the fixture BigVGAN in bf16 on the mel of the same batch (640
frames per utterance).  Last, the ``mel_l1`` between the bf16, fp16 and fp32 outputs of the fixture BigVGAN on one fixture mel: the
weights are seeded, so this is a rounding figure, not a quality one.

    python tools/bench_fidelity.py --out profiles/fidelity_bench.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, fidelity, fixture_weights as fw, packing
from ims_toucan_prosody_variance_amd.ragged import Ragged


def windows(fn, dev, args, reps=None):
    reps = reps or args.reps
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / reps)
    return {"us": round(float(np.median(out)), 2), "us_min": round(min(out), 2), "us_max": round(max(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=245760)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fidelity.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, n = args.batch, args.samples
    m = fidelity.SpectralDistance(dev)
    ops = m.ops
    rng = np.random.default_rng(7)
    rec = 0.1 * rng.standard_normal((B, n))
    gen = rec + 0.001 * rng.standard_normal((B, n))
    packed = torch.from_numpy(np.stack([gen, rec], axis=1).astype(np.float32).reshape(-1)).to(dev)  # [a0 b0 a1 b1 ...]
    pair_spans = [(2 * p * n, (2 * p + 1) * n, n) for p in range(B)]
    spans = [s for a, b, k in pair_spans for s in ((a, k), (b, k))]
    ref = fidelity.REFERENCE_RESOLUTION
    rows = {"distance_1_resolution": windows(lambda: m.distance_packed(packed, pair_spans, (ref,)), dev, args),
            "distance_3_resolutions": windows(lambda: m.distance_packed(packed, pair_spans), dev, args)}
    mel_l1 = m.distance_packed(packed, pair_spans, (ref,))[0]["mel_l1"]
    for n_fft, hop in fidelity.DEFAULT_RESOLUTIONS:
        bins, key = n_fft // 2 + 1, f"{n_fft}"
        buf, rag = m.frame(packed, spans, hop)
        spec = ops.empty(rag.total_rows, 2 * bins)
        conv = lambda: ops.conv(m.basis(n_fft), buf, spec, rag, compute=capi.COMPUTE_F32, split_k=False)
        conv()
        pairs = [(rag.begins[2 * p], rag.begins[2 * p + 1], fidelity.frame_count(n, hop)) for p in range(B)]
        rows[key + ".tts_frame_reflect"] = windows(lambda: m.frame(packed, spans, hop), dev, args)
        rows[key + ".dft_conv"] = windows(conv, dev, args)
        rows[key + ".tail"] = windows(lambda: m.sums(spec, bins, pairs, (n_fft, hop) == ref), dev, args)
        if (n_fft, hop) == ref:
            # the same mel_l1 from the launches of the parent: magnitude, mel projection (a conv), log10 with a floor, L1 in torch
            mel_cw = packing.pack_conv(m.mel, None, dev)
            R, F = rag.lengths[0], fidelity.frame_count(n, hop)
            assert all(r == R for r in rag.lengths)

            def composed():
                mag = ops.empty(rag.total_rows, bins)
                capi.check(ops.lib.tts_complex_magnitude(spec.data_ptr(), 2 * bins, mag.data_ptr(), bins, rag.total_rows, bins, ops.stream()), "tts_complex_magnitude")
                melp = ops.conv(mel_cw, mag, ops.empty(rag.total_rows, fidelity.N_MELS), rag, compute=capi.COMPUTE_F32, split_k=False)
                lg = ops.empty(rag.total_rows, fidelity.N_MELS)
                capi.check(ops.lib.tts_log10_floor(melp.data_ptr(), fidelity.N_MELS, lg.data_ptr(), fidelity.N_MELS, rag.total_rows, fidelity.N_MELS, 1e-10,
                                                   ops.stream()), "tts_log10_floor")
                v = lg.view(B, 2, R, fidelity.N_MELS)[:, :, :F]
                return (v[:, 0] - v[:, 1]).abs().to(torch.float64).sum(dim=(1, 2)) / (F * fidelity.N_MELS)

            rows[key + ".tail_composed_mel_only"] = windows(composed, dev, args)
            composed_mel_l1 = float(composed()[0])

    # the yardstick: the fixture BigVGAN in bf16 on the mel of the same batch
    frames = n // fidelity.VOCODER_HOP
    sd = fw.bigvgan_state_dict()
    voc = {p: engine.VocoderEngine(sd, "bigvgan", dev, precision=p) for p in ("bf16", "f16", "f32")}
    mel = torch.from_numpy(np.concatenate([fw.reference_spectrogram(u % 4, frames) for u in range(B)])).to(dev)
    rag_mel = Ragged([frames] * B, dev)
    rows["vocoder_bigvgan_bf16"] = windows(lambda: voc["bf16"].forward(mel, rag_mel), dev, args, reps=2)

    # what a precision costs in the unit the vocoder is trained in (seeded weights: a rounding figure)
    one, rag_one = mel[:frames].contiguous(), Ragged([frames], dev)
    wav = {p: v.forward(one, rag_one)[0][: fidelity.VOCODER_HOP * frames].clone() for p, v in voc.items()}
    d = m.distance([wav["bf16"], wav["f16"], wav["bf16"]], [wav["f32"], wav["f32"], wav["f16"]])
    precision = {name: {"mel_l1": r["mel_l1"], **{f"{k[0]}": v for k, v in r["resolutions"].items()}}
                 for name, r in zip(("bf16_vs_f32", "f16_vs_f32", "bf16_vs_f16"), d)}

    res = {"metric": "fidelity_us_per_batch", "pairs": B, "samples": n, "rate": fidelity.SR, "reps": args.reps, "rounds": args.rounds, "times": rows,
           "mel_l1": mel_l1, "composed_mel_l1": composed_mel_l1, "share_of_vocoder": {k: round(v["us"] / rows["vocoder_bigvgan_bf16"]["us"], 5)
                                                                                   for k, v in rows.items() if k != "vocoder_bigvgan_bf16"},
           "precision_mel_l1": precision, "gpu": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
