"""Corpus scoring throughput on the MI355X: a seeded corpus (default 256 utterances of ~625 frames and ~100 phonemes,
fixture_weights.write_fixture_corpus) scored in batches of 32 by both scorers of scorer.py, from caches already read into host
memory.  Prints one JSON line: utterances/s of each scorer (median of --steps passes over the corpus) and the split of a pass into
aligner logits / CTC, and style embedding / acoustic stages / loss kernel, from HIP events.

    python tools/bench_score.py --utterances 256 --batch 32 --steps 3 --warmup 1

``--glow`` adds a phase after those: passes of the TTS scorer over the same corpus with and without ``include_glow``, alternated, and
the keys ``glow_*`` in the JSON line (the pass with the glow loss, the pass without it measured beside it, the HIP-event time of
``tts_postflow_nll``, and its cost per utterance).  Without the flag the output is what it was.
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
from ims_toucan_prosody_variance_amd import fixture_weights as fw, scorer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--glow", action="store_true", help="also time the TTS scorer with include_glow=True against without, alternated")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        fw.write_fixture_corpus(d, args.utterances, seed=42, words=(20, 22), max_duration=15)
        al_items, _ = scorer.read_aligner_cache(d)
        _, tts_items = scorer.read_tts_cache(d)
        t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
        torch.save({"asr_model": t(fw.aligner_state_dict())}, os.path.join(d, "aligner.pt"))
        torch.save({"model": t(fw.acoustic_state_dict())}, os.path.join(d, "model.pt"))
        torch.save({"style_emb_func": t(fw.style_state_dict())}, os.path.join(d, "emb.pt"))
        al = scorer.AlignmentScorer(os.path.join(d, "aligner.pt"), dev, timing=True)
        tts = scorer.TTSScorer(os.path.join(d, "model.pt"), dev, path_to_embedding_checkpoint=os.path.join(d, "emb.pt"), timing=True)
    lid = 12  # "en"
    res = {}
    for name, run, get in (("align", lambda: al.score_items(al_items, args.batch), lambda: al.last_phase_ms),
                           ("tts", lambda: tts.score_items(tts_items, lid, args.batch), lambda: tts.last_phase_ms)):
        for _ in range(args.warmup):
            run()
        wall, phases = [], []
        for _ in range(args.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()  # each batch ends with a device-to-host copy of its losses
            wall.append((time.perf_counter() - t0) * 1e3)
            phases.append(dict(get()))
        res[name] = (float(np.median(wall)), {k: float(np.median([p.get(k, 0.0) for p in phases])) for k in phases[0]})
    n, nb = args.utterances, -(-args.utterances // args.batch)
    (wa, pa), (wt, pt) = res["align"], res["tts"]
    r = lambda v: round(v, 3)
    out = {
        "metric": "score_utterances_per_s", "utterances": n, "batch": args.batch, "steps": args.steps,
        "mean_frames": round(float(np.mean([m.shape[0] for _, m in al_items])), 1),
        "mean_phonemes": round(float(np.mean([t_.shape[0] for t_, _ in al_items])), 1),
        "align_utterances_per_s": round(1e3 * n / wa, 1), "align_ms_per_pass": r(wa),
        "align_ms_logits": r(pa.get("logits", 0.0)), "align_ms_ctc": r(pa.get("ctc", 0.0)),
        "align_ms_ctc_per_batch": r(pa.get("ctc", 0.0) / nb),
        "tts_utterances_per_s": round(1e3 * n / wt, 1), "tts_ms_per_pass": r(wt),
        "tts_ms_style": r(pt.get("style", 0.0)), "tts_ms_acoustic": r(pt.get("acoustic", 0.0)), "tts_ms_loss": r(pt.get("loss", 0.0)),
        "gpu": torch.cuda.get_device_name(dev),
    }
    if args.glow:
        wall, glow_ms = {False: [], True: []}, []
        for step in range(args.warmup + args.steps):
            for on in (False, True):  # alternated: both see the same clocks and cache state
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                tts.score_items(tts_items, lid, args.batch, include_glow=on)
                if step >= args.warmup:
                    wall[on].append((time.perf_counter() - t0) * 1e3)
                    if on:
                        glow_ms.append(tts.last_phase_ms.get("glow", 0.0))
        w0, w1, g = float(np.median(wall[False])), float(np.median(wall[True])), float(np.median(glow_ms))
        out.update({"glow_tts_utterances_per_s": round(1e3 * n / w1, 1), "glow_tts_ms_per_pass": r(w1), "glow_off_ms_per_pass": r(w0),
                    "glow_ms_postflow_nll": r(g), "glow_ms_per_utterance": r(g / n)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
