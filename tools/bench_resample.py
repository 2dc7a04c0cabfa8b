"""Sample-rate conversion on the MI355X.  Prints one JSON line.

Kernel: one batch (default 32 utterances of 245 760 samples, 10.24 s at 24 kHz) through tts_resample for 24 -> 16 kHz and
24 -> 48 kHz (--rates adds others, e.g. 44100 and 22050 for the larger tables), float32 and PCM16 out: device time from HIP events around --reps back-to-back launches, median (min, max) of
--rounds such windows after --warmup launches, beside the bytes the conversion has to move (the batch read once, the result
written once) over the 6.29 TB/s a streaming copy reaches on this GPU.

End to end (--e2e): the benchmark batch (32 utterances x 128 phonemes x 5 frames, BigVGAN, fixture weights, the precision of
TOUCAN_PRECISION) through the interface, in alternation, --steps times each, on a host clock that ends with the waveforms on
the host: ``synthesize_batch(sample_rate=16000)``; what a caller did before the keyword existed - ``synthesize_batch()`` and
``style.resample_sinc`` per waveform (without the keywords ``synthesize_batch()`` is the code path it was before they existed: no
launch is added and the bits are the same, so it stands in for a build of the parent commit); and a plain
``synthesize_batch()``.  The first and the last are timed once more with the
waveforms left on the device (the clock ends in a synchronise): the cost of the stage without the smaller download.

    python tools/bench_resample.py --rates 16000 48000 8000 44100 22050 --e2e --out profiles/resample_bench.json
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

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, interface, resample, style, synthetic as syn

COPY_TBS = 6.29  # measured streaming-copy bandwidth of the MI355X, TB/s


def kernel_times(args, dev):
    res = resample.Resampler(dev)
    B, n = args.batch, args.samples
    rng = np.random.default_rng(7)
    wave = torch.from_numpy(np.clip(0.3 * rng.standard_normal(B * n), -1, 1).astype(np.float32)).to(dev)
    rows = []
    for sr_out in args.rates:
        orig, new, w, tab = res.table(24000, sr_out)
        count = resample.out_length(n, 24000, sr_out)
        spans = torch.tensor([[b * n, n, 0, 0, count, b * count] for b in range(B)], dtype=torch.int64, device=dev)
        for pcm16 in (False, True):
            y = torch.empty(B * count, dtype=torch.int16 if pcm16 else torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream

            def launch():
                rc = res.lib.tts_resample(wave.data_ptr(), tab.data_ptr(), spans.data_ptr(), B, count, orig, new, w, int(pcm16), y.data_ptr(), st)
                assert rc == 0, res.lib.tts_last_error()

            for _ in range(args.warmup):
                launch()
            torch.cuda.synchronize(dev)
            windows = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                e1.synchronize()
                windows.append(1e3 * e0.elapsed_time(e1) / args.reps)
            nbytes = 4 * B * n + y.element_size() * B * count
            us = float(np.median(windows))
            rows.append({"sr_out": sr_out, "out": "int16" if pcm16 else "float32", "orig": orig, "new": new, "taps": 2 * w + orig,
                         "table_bytes": 4 * new * (2 * w + orig), "table_in_lds": 4 * new * (2 * w + orig) <= capi.RESAMPLE_LDS_TABLE_BYTES,
                         "us": round(us, 2), "us_min": round(min(windows), 2), "us_max": round(max(windows), 2),
                         "bytes": nbytes, "us_at_copy_bandwidth": round(nbytes / (COPY_TBS * 1e6), 2),
                         "share_of_copy_bandwidth": round(nbytes / (COPY_TBS * 1e6) / us, 3),
                         "gflops": round(2.0 * B * count * (2 * w + orig) / (us * 1e3), 1)})
    return rows


def end_to_end(args, dev):
    models_dir = interface.MODELS_DIR
    with tempfile.TemporaryDirectory() as tmp:  # the constructor reads the checkpoints; nothing is read from there afterwards
        interface.write_fixture_checkpoints(tmp, n_lang=20)
        interface.MODELS_DIR = tmp
        try:
            tts = interface.ToucanTTSInterface(device=str(dev), tts_model_path="Meta", faster_vocoder=False)
        finally:
            interface.MODELS_DIR = models_dir
    B, L, fpp = args.batch, 128, 5
    feats = [torch.from_numpy(syn.utterance_features(u, L, word_boundaries=False)) for u in range(B)]
    kw = dict(durations=[torch.full((L,), fpp, dtype=torch.long) for _ in range(B)],
              z_noise=[torch.from_numpy(syn.postflow_noise(u, L * fpp)) for u in range(B)])

    def on_device():
        return [w.cpu().numpy() for w in tts.synthesize_batch(feats, sample_rate=16000, **kw)]

    def on_host():
        return [style.resample_sinc(w.cpu().numpy(), 24000, 16000) for w in tts.synthesize_batch(feats, **kw)]

    def plain():
        return [w.cpu().numpy() for w in tts.synthesize_batch(feats, **kw)]

    def left_on_device(**fmt):
        def run():
            out = tts.synthesize_batch(feats, **fmt, **kw)
            torch.cuda.synchronize(dev)
            return out
        return run

    # the first three end with the waveforms on the host; the last two leave them on the device: the cost of the stage itself
    ways = {"device_16k": on_device, "host_16k": on_host, "plain_24k": plain,
            "device_16k_no_download": left_on_device(sample_rate=16000), "plain_24k_no_download": left_on_device()}
    for _ in range(args.warmup):
        outs = {k: f() for k, f in ways.items()}
    worst = max(float(np.abs(a - b).max()) for a, b in zip(outs["device_16k"], outs["host_16k"]))
    n_samples, outs = int(outs["plain_24k"][0].shape[0]), None
    ms = {k: [] for k in ways}
    for _ in range(args.steps):
        for k, f in ways.items():  # alternating: each round times every way once
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"batch": B, "samples_per_utterance": n_samples, "precision": os.environ.get("TOUCAN_PRECISION", "f32"),
            "ms": ms, "median_ms": {k: round(float(np.median(v)), 3) for k, v in ms.items()},
            "device_below_host_in_every_round": all(a < b for a, b in zip(ms["device_16k"], ms["host_16k"])),
            "overhead_ms_over_plain_median": round(float(np.median(ms["device_16k"]) - np.median(ms["plain_24k"])), 3),
            "plain_spread_ms": round(max(ms["plain_24k"]) - min(ms["plain_24k"]), 3),
            "overhead_ms_over_plain_median_no_download": round(float(np.median(ms["device_16k_no_download"]) - np.median(ms["plain_24k_no_download"])), 3),
            "plain_spread_ms_no_download": round(max(ms["plain_24k_no_download"]) - min(ms["plain_24k_no_download"]), 3),
            "max_abs_difference_device_vs_host": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=245760)
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 48000])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=7, help="end to end: rounds, each timing every way once")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample.py measures on the MI355X"
    dev = torch.device("cuda:0")
    out = {"metric": "resample_us_per_batch", "batch": args.batch, "samples": args.samples, "reps": args.reps, "rounds": args.rounds,
           "kernel": kernel_times(args, dev), "gpu": torch.cuda.get_device_name(dev)}
    if args.e2e:
        out["end_to_end"] = end_to_end(args, dev)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
