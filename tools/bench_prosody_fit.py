"""What a time budget costs in one pass, and what the two-pass route it replaces costs, on the MI355X.  Prints one JSON line.

The acoustic model (native.NativePipeline.forward, no vocoder: the vocoder's work is the same either way) on 32 x 128 phonemes
(seeded synthetic features, fixture weights, --precision, default bf16).  Every utterance gets a target of 1.2 x its unscaled frame
count, on the duration knob, exact=False: the pass then ends with exactly the durations of the solved scales, so both ways of (a)
run the same decoder work.

  fit        ONE pass with ``prosody_fit=`` (tts_control_and_regulate_t: the solver between the predictors and the control kernel);
  scales     (a) the same pass given the scales ``fit`` solved as plain per-utterance scales (tts_control_and_regulate_v);
  two_pass   (b) the route without the solver, with interfaces the parent commit has: the stage A of ``predict_frame_counts``
             (encoder, predictors and a host round trip; the inputs are packed once, outside the clock, for every way), a scale
             target / frames chosen on the host, then the pass with those per-utterance scales.
             --parent-root: a built checkout of the parent commit, where it is timed as well (key parent_two_pass, and
             parent_scales for the plain pass there).
  stage A alone (encoder .. length regulator) is reported for ``fit`` and ``scales`` too: the solver's share is read there.

Every figure is a host clock around one call that ends in a device synchronise, --reps times after --warmup, the ways of one
process in alternation; this tree and the parent run in fresh child processes, alternating, --rounds times each.  Reported per
way: median, quartiles, min, max of the pooled repetitions and the median of every round.

    python tools/bench_prosody_fit.py --parent-root ../parent --out profiles/prosody_fit_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def _summary(ms):
    import numpy as np
    q = np.percentile(ms, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "q25": round(float(q[0]), 4), "q75": round(float(q[2]), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4), "n": len(ms)}


def worker(args):
    """Child process: the tree at args.root with the ways it has."""
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    import ims_toucan_prosody_variance_amd  # noqa: F401
    from ims_toucan_prosody_variance_amd import fixture_weights as fw, native, synthetic as syn
    assert torch.cuda.is_available(), "bench_prosody_fit.py measures on the MI355X"
    dev = "cuda:0"
    pipe = native.NativePipeline(fw.acoustic_state_dict(), None, None, dev, precision=args.precision)
    B, L = args.batch, args.phonemes
    feats = [torch.from_numpy(syn.utterance_features(u, L)) for u in range(B)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in range(B)]))
    langs = [syn.LANG_EN] * B
    packed = pipe.pack_inputs(feats, embs, langs, None, None, None)
    base = pipe.predict_frame_counts(feats, embs, langs)
    targets = [int(round(1.2 * t)) for t in base]
    st = pipe._stream()

    def full(**kw):
        out = pipe.forward(feats, embs, langs, packed=packed, vocode=False, run_postflow=False, **kw)
        return [int(n) for n in out["rag_frame"].lengths], out

    def two_pass():
        frames = pipe._stage_a(packed, 1.0, 1.0, 1.0, 1.0, st)  # (predict_frame_counts without its packing: ends in the host round trip of its stage A)
        return full(duration_scaling_factor=[t / f for t, f in zip(targets, frames)])

    ways, info = {}, {}
    if "fit" in args.entries:
        from ims_toucan_prosody_variance_amd.prosody_fit import Fit
        fits = [Fit(target_frames=t, exact=False) for t in targets]
        frames, out = full(prosody_fit=fits)
        solved = [float(s) for s in out["prosody_fit"]["scales"][:, 0]]
        report = np.concatenate(out["prosody_fit"]["report"])
        info = {"status_counts": np.bincount(report[:, 4].astype(int), minlength=6).tolist(), "iterations_max": int(report[:, 5].max()),
                "frames_off_target_max": int(np.abs(report[:, 1] - report[:, 0]).max())}
        same, _ = full(duration_scaling_factor=solved)
        info["same_frames_both_ways"] = same == frames
        ways["fit"] = lambda: full(prosody_fit=fits)[0]
        ways["scales"] = lambda: full(duration_scaling_factor=solved)[0]
        ways["stage_a_fit"] = lambda: pipe._stage_a(packed, 1.0, 1.0, 1.0, 1.0, st, prosody_fit=fits)
        ways["stage_a_scales"] = lambda: pipe._stage_a(packed, solved, 1.0, 1.0, 1.0, st)
        exact = [Fit(target_frames=t) for t in targets]
        ways["fit_exact"] = lambda: full(prosody_fit=exact)[0]
    else:
        guess = [t / f for t, f in zip(targets, base)]
        ways["scales"] = lambda: full(duration_scaling_factor=guess)[0]
    ways["two_pass"] = lambda: two_pass()[0]
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
    print("RESULT " + json.dumps({"ms": ms, "frames": frames, "targets": sum(targets), "info": info, "gpu": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phonemes", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument("--entries", default="fit", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    def child(root, entries):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--entries", entries, "--phonemes", str(args.phonemes),
               "--batch", str(args.batch), "--precision", args.precision, "--warmup", str(args.warmup), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400, cwd=os.path.abspath(root))
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"worker in {root} failed ({r.returncode}):\n{r.stdout[-4000:]}")
        return json.loads(lines[-1][len("RESULT "):])

    pooled, rounds, frames, gpu, info, targets = {}, {}, {}, None, {}, None
    for _ in range(args.rounds):  # alternating processes: this tree, the parent, this tree, ...
        for name, root, entries in (("this", os.path.dirname(HERE), "fit"), ("parent", args.parent_root, "none")):
            if root is None:
                continue
            res = child(root, entries)
            gpu, targets = res["gpu"], res["targets"]
            if name == "this":
                info = res["info"]
            for k, v in res["ms"].items():
                key = k if name == "this" else "parent_" + k
                pooled.setdefault(key, []).extend(v)
                rounds.setdefault(key, []).append(_summary(v)["median"])
                frames[key] = res["frames"][k]
    med = {k: _summary(v) for k, v in pooled.items()}
    out = {"metric": "prosody_fit_ms", "precision": args.precision, "batch": args.batch, "phonemes": args.phonemes, "target_frames": targets,
           "ms_per_call": med, "median_of_every_round": rounds, "frames": frames, "fit": info,
           "a_fit_minus_scales_ms": round(med["fit"]["median"] - med["scales"]["median"], 4),
           "a_stage_a_fit_minus_scales_ms": round(med["stage_a_fit"]["median"] - med["stage_a_scales"]["median"], 4),
           "b_two_pass_minus_fit_ms": round(med["two_pass"]["median"] - med["fit"]["median"], 4),
           "scales_round_to_round_spread_ms": round(max(rounds["scales"]) - min(rounds["scales"]), 4), "gpu": gpu}
    if "parent_two_pass" in med:
        out["b_parent_two_pass_minus_fit_ms"] = round(med["parent_two_pass"]["median"] - med["fit"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
