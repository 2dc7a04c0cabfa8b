"""The aligner's on-line fine-tuning on the MI355X: one utterance (default 10 s = 625 frames, 100 tokens) through
finetune.AlignerFineTuner - five SGD steps of CTC training, then the eval-mode logits.  Prints one JSON line: ms per utterance (median
of --repeats, wall clock around the call, which ends with the read-back of the losses and norms) and its split into the phases from HIP
events: forward / ctc / bptt / gemm_gradients / update (all five steps together) and eval_logits.

    python tools/bench_finetune.py --frames 625 --tokens 100 --repeats 5 --warmup 2
    rocprofv3 --kernel-trace --stats -d /tmp/ft_prof -- python tools/bench_finetune.py     # per-kernel times of the same run
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
from ims_toucan_prosody_variance_amd import align, finetune, fixture_weights as fw, phonemes

PHASES = ("forward", "ctc", "bptt", "gemm_gradients", "update", "eval_logits")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=625)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5, help="timed repetitions of the whole procedure (its five SGD steps are fixed)")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T, L = args.frames, args.tokens
    ft = finetune.AlignerFineTuner(fw.aligner_state_dict(), dev, timing=True)
    syms = sorted(s for s, v in phonemes.phone_table().items() if v[15] == 1 and v[21] == 0)
    idx = (fw.uniform01("bench.syms0", L, 5) * len(syms)).astype(int)
    ids, _ = align.token_ids(phonemes.phones_to_features("".join(syms[i] for i in idx), handle_missing=False))
    mel = torch.from_numpy(fw.aligner_spectrogram(100, T)).to(dev)
    masks = finetune.dropout_masks(0, T)
    for _ in range(args.warmup):
        ft.fine_tune(mel, ids, masks)
    wall, phases = [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ft.fine_tune(mel, ids, masks)
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(dict(ft.last_phase_ms))
    med = lambda k: float(np.median([p.get(k, 0.0) for p in phases]))
    out = {"metric": "finetune_ms_per_utterance", "frames": T, "tokens": len(ids), "sgd_steps": finetune.STEPS, "repeats": args.repeats,
           "ms_per_utterance": round(float(np.median(wall)), 3)}
    out.update({f"ms_{k}": round(med(k), 3) for k in PHASES})
    out.update({"loss": [round(float(v), 4) for v in ft.last_loss], "norm": [round(float(v), 3) for v in ft.last_norm],
                "gpu": torch.cuda.get_device_name(dev)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
