"""What per-phoneme prosody curves cost in stage A, and what an emphasis sweep gains, on the MI355X.  Prints one JSON line.

Stage A (tts_encoder, tts_variance_predictors, control + length regulator) on 32 x 128 phonemes (seeded synthetic features,
fixture weights, --precision, default bf16, no vocoder):

  curves   the control step is tts_control_and_regulate_c: per-utterance scales, a curve table with one Span per utterance (the
           utterance's second word) and the statistics of utterances and spans; the time includes turning the Spans into the
           packed table on the host (prosody.resolve_curves), which is also reported on its own;
  scales   the control step is tts_control_and_regulate_v with the same per-utterance scales, on the same commit;
  scalars  the control step is the scalar tts_control_and_regulate with (1.02, 1.04, 0.96, 1.0), on the same commit;
  parent   the same as ``scales`` in a checkout of the parent commit built beside this one (--parent-root), where the curves do
           not exist: what stage A cost before.  --parent-entries scalars,scales,curves: a parent that has all three ways runs
           all three (keys parent_scalars, parent, parent_curves).

Every figure is a host clock around one stage A that ends in a device synchronise, --reps times after --warmup, the entries of one
process in alternation; this tree and the parent run in fresh child processes, alternating, --rounds times each, because two
builds of the library cannot share a process.  Reported per way: median, min, max, and the quartiles of the pooled repetitions,
plus the median of every round (the run-to-run spread the difference has to be read against).

The emphasis sweep: one 128-phoneme sentence with each of its words stressed in turn (BigVGAN, waveforms left on the device):

  grid       ONE ``synthesize_grid(curves=[emphasis(feats, [k]) ...])`` call;
  two_pass   the route the curves replace: one call that predicts, the prosody read back, then per word an edit on the host and
             a call with gold durations / pitch / energy.

    python tools/bench_prosody_curves.py --parent-root ../parent --out profiles/prosody_curves_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def _summary(ms):
    import numpy as np
    q = np.percentile(ms, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "q25": round(float(q[0]), 4), "q75": round(float(q[2]), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4), "n": len(ms)}


def stage_worker(args):
    """Child process: stage A of the tree at args.root with the entries it has."""
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    import ims_toucan_prosody_variance_amd  # noqa: F401
    from ims_toucan_prosody_variance_amd import fixture_weights as fw, native, prosody, synthetic as syn
    assert torch.cuda.is_available(), "bench_prosody_curves.py measures on the MI355X"
    dev = "cuda:0"
    pipe = native.NativePipeline(fw.acoustic_state_dict(), None, None, dev, precision=args.precision)
    B, L = args.batch, args.phonemes
    feats = [syn.utterance_features(u, L) for u in range(B)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in range(B)]))
    packed = pipe.pack_inputs([torch.from_numpy(f) for f in feats], embs, [syn.LANG_EN] * B, None, None, None)
    scales = [[1.0 + 0.01 * (u % 5) for u in range(B)], [1.0 + 0.02 * (u % 3) for u in range(B)], [1.0 - 0.02 * (u % 4) for u in range(B)], 1.0]
    st = pipe._stream()
    ways = {"scales": lambda: pipe._stage_a(packed, *scales, st)}
    if "scalars" in args.entries:  # one set of scalars for the batch: tts_control_and_regulate
        ways["scalars"] = lambda: pipe._stage_a(packed, 1.02, 1.04, 0.96, 1.0, st)
    if "curves" in args.entries:
        curves = []
        for f in feats:  # one Span per utterance: its second word (the first if it has one word only)
            words = prosody.word_spans(f)
            curves.append(prosody.emphasis(f, [min(1, len(words) - 1)]))
        ways["curves"] = lambda: pipe._stage_a(packed, *scales, st, prosody_curves=curves)
    frames = {}
    for _ in range(args.warmup):
        for k, f in ways.items():
            frames[k] = sum(f())
    ms = {k: [] for k in ways}
    for _ in range(args.reps):
        for k, f in ways.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3, 4))
    host = None
    if "curves" in args.entries:  # the host share of ``curves``: Spans -> packed table, in Python, before anything is enqueued
        t0 = time.perf_counter()
        for _ in range(args.reps):
            prosody.resolve_curves([L] * B, curves)
        host = round((time.perf_counter() - t0) * 1e3 / args.reps, 4)
    print("RESULT " + json.dumps({"ms": ms, "frames": frames, "resolve_curves_host_ms": host, "gpu": torch.cuda.get_device_name(0)}))


def _edit_on_the_host(feats, d, p, e, span):
    """What a caller of the two-pass route does for one Span: the definition on the host, in numpy."""
    import numpy as np
    d, p, e = d.copy(), p.copy(), e.copy()
    sl = slice(span.start, span.stop)
    d[sl] = np.rint(d[sl].astype(np.float32) * np.float32(span.duration)).astype(d.dtype)
    for seq, factor, offset in ((p, span.pitch, span.pitch_offset), (e, span.energy, span.energy_offset)):
        nz = seq[seq != 0]
        avg = nz.mean() if nz.size else np.float32("nan")
        if factor != 1.0:
            seq[sl] = np.maximum((seq[sl] - avg) * np.float32(factor) + avg, 0)
        if offset != 0.0:
            seq[sl] = np.where(seq[sl] != 0, np.maximum(seq[sl] + np.float32(offset), 0), seq[sl])
    return d, p, e


def sweep(args):
    import numpy as np
    import torch
    os.environ["TOUCAN_PRECISION"] = args.precision  # (read by the interface's constructor)
    sys.path.insert(0, os.path.dirname(HERE))
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
    feats_np = syn.utterance_features(0, args.phonemes)
    feats = torch.from_numpy(feats_np)
    words = prosody.word_spans(feats_np)[:tts.MAX_FILE_BATCH]
    curves = [prosody.emphasis(feats_np, [k]) for k in range(len(words))]

    def grid():
        out = tts.synthesize_grid(feats, curves=curves)
        torch.cuda.synchronize(dev)
        return [r["frames"] for r in out]

    def two_pass():
        tts.synthesize_batch([feats])
        d, p, e = (t[0].cpu().numpy() for t in (tts.last_durations, tts.last_pitch, tts.last_energy))  # (the read-back: a synchronise)
        frames = []
        for c in curves:
            dd, pp, ee = _edit_on_the_host(feats_np, d, p, e, c[0])
            w = tts.synthesize_batch([feats], durations=[torch.from_numpy(dd)], pitch=[torch.from_numpy(pp)], energy=[torch.from_numpy(ee)])
            frames.append(w[0].numel() // 384)
        torch.cuda.synchronize(dev)
        return frames

    ways = {"grid": grid, "two_pass": two_pass}
    for _ in range(2):
        frames = {k: f() for k, f in ways.items()}
    ms = {k: [] for k in ways}
    for _ in range(args.sweep_steps):
        for k, f in ways.items():  # alternating
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"words": len(words), "phonemes": args.phonemes, "vocoder": "bigvgan", "frames_per_variant": frames["grid"],
            "same_frame_counts_both_ways": frames["grid"] == frames["two_pass"], "ms": ms, "ms_per_sweep": {k: _summary(v) for k, v in ms.items()},
            "two_pass_over_grid": round(_summary(ms["two_pass"])["median"] / _summary(ms["grid"])["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phonemes", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep-steps", type=int, default=7)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--parent-entries", default="scales", help="the ways the parent has: scalars,scales,curves (keys parent_scalars, parent, parent_curves)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument("--entries", default="scales,curves", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return stage_worker(args)

    def child(root, entries):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--entries", entries, "--phonemes", str(args.phonemes),
               "--batch", str(args.batch), "--precision", args.precision, "--warmup", str(args.warmup), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, cwd=os.path.abspath(root))
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"stage worker in {root} failed ({r.returncode}):\n{r.stdout[-4000:]}")
        return json.loads(lines[-1][len("RESULT "):])

    pooled, rounds, frames, gpu, host = {}, {}, {}, None, []
    for _ in range(args.rounds):  # alternating processes: this tree, the parent, this tree, ...
        for name, root, entries in (("this", os.path.dirname(HERE), "scalars,scales,curves"), ("parent", args.parent_root, args.parent_entries)):
            if root is None:
                continue
            res = child(root, entries)
            gpu = res["gpu"]
            if res.get("resolve_curves_host_ms") is not None:
                host.append(res["resolve_curves_host_ms"])
            for k, v in res["ms"].items():
                key = k if name == "this" else "parent" if k == "scales" else "parent_" + k
                pooled.setdefault(key, []).extend(v)
                rounds.setdefault(key, []).append(_summary(v)["median"])
                frames[key] = res["frames"][k]
    stage = {"batch": args.batch, "phonemes": args.phonemes, "ms_per_stage_a": {k: _summary(v) for k, v in pooled.items()}, "median_of_every_round": rounds,
             "frames": frames, "resolve_curves_host_ms_every_round": host}
    base = "parent" if "parent" in pooled else "scales"
    stage["curves_minus_" + base + "_median_ms"] = round(stage["ms_per_stage_a"]["curves"]["median"] - stage["ms_per_stage_a"][base]["median"], 4)
    stage[base + "_round_to_round_spread_ms"] = round(max(rounds[base]) - min(rounds[base]), 4)
    out = {"metric": "prosody_curves_stage_a_ms", "precision": args.precision, "stage_a": stage, "emphasis_sweep": sweep(args), "gpu": gpu}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
