"""The recording-free pronunciation check on the MI355X (pronunciation.PronunciationChecker): a batch (default 32 utterances of 128
phonemes and 10.2 s of 24 kHz audio, about 640 aligner frames each) with the fixture aligner.  Prints one JSON line: ms per call of
check() as a caller sees it (median of --steps on a host clock that ends in the device-to-host copies) for beam 0, 8 and 32; the time
of each new kernel's call (the upload of its utterance table and its launch) from HIP events around --reps back-to-back calls, the
median of --rounds such windows after a warm-up, the beam search at 1, 8 and 32; and beside them, measured the same way, the
waves' way to 16 kHz (compare.waves_to_16k: upload, resampler, download and the division by the peak on the host; one call per
window), the STFT with the log-mel, the aligner's forward pass (whose LSTM takes one launch per frame; one call per window),
tts_ctc_loss and tts_mas_durations.  With seeded weights the posteriors are close to flat: the beam search is then at its most expensive (every
candidate is alive), the edit distance sees hypotheses of a few tokens.

    python tools/bench_pronunciation.py --steps 10 --warmup 2 --out profiles/pronunciation_bench.json
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
from ims_toucan_prosody_variance_amd import compare, fixture_weights as fw, pronunciation as pron, scorer
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from tools.bench_pitch import event_ms, recording

SENTENCE = "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt dɹˈɪɹi wˈaɪl aɪ pˈɑːndɚd~#"


def text_of(n_phonemes, shift):
    """[L, 62] features with n_phonemes tokens that are not word boundaries: the sentence's rows, repeated from row `shift` on."""
    rows = phones_to_features(SENTENCE, handle_missing=False)
    out, k, n = [], shift, 0
    while n < n_phonemes:
        r = rows[k % len(rows)]
        k += 1
        if out and np.array_equal(out[-1], r):
            continue
        out.append(r)
        n += int(r[pron.align.IDX["word_boundary"]] == 0)
    return np.stack(out).astype(np.float32)


def median_event_ms(fn, reps, rounds):
    fn()
    return float(np.median([event_ms(fn, reps) for _ in range(rounds)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--phonemes", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=10.2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pronunciation.py measures on the MI355X"
    dev = torch.device("cuda:0")
    B, sr = args.utterances, 24000
    n = int(round(args.seconds * sr))
    waves = [recording(700 + u, n) for u in range(B)]
    feats = [text_of(args.phonemes, 3 * u) for u in range(B)]
    chk = pron.PronunciationChecker(fw.aligner_state_dict(), dev)
    for _ in range(args.warmup):
        for beam in (0, 8, 32):
            res = chk.check(feats, waves, sr, beam=beam)
    wall = {}
    for beam in (0, 8, 32):
        times = []
        for _ in range(args.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = chk.check(feats, waves, sr, beam=beam)
            times.append((time.perf_counter() - t0) * 1e3)
        wall[beam] = float(np.median(times))

    # the stages, each on what the stage before left on the device
    ext, al = chk.extractor, chk.aligner
    w16 = compare.waves_to_16k(chk, waves, [sr] * B, [f"utterance {b}" for b in range(B)])
    ms_16k = median_event_ms(lambda: compare.waves_to_16k(chk, waves, [sr] * B, [str(b) for b in range(B)]), 1, args.rounds)

    def front():
        spec, rag = ext.spectra(w16)
        return ext.log_mel(spec, rag), rag
    ms_front = median_event_ms(front, args.reps, args.rounds)
    mel, rag = front()
    ms_aligner = median_event_ms(lambda: al.logits(mel, rag), 1, args.rounds)
    logits = al.logits(mel, rag)
    toks = [pron.reference_tokens(f) for f in feats]
    ids, flags, full_ids, refs = [t[0] for t in toks], [t[1] for t in toks], [t[2] for t in toks], [t[3] for t in toks]
    stages = {"ms_ctc_best_path": median_event_ms(lambda: chk.best_path(logits, rag), args.reps, args.rounds)}
    for beam in (1, 8, 32):
        stages[f"ms_ctc_beam_search_{beam}"] = median_event_ms(lambda: chk.beam_search(logits, rag, beam), args.reps, args.rounds)
    dec = chk.beam_search(logits, rag, 8)
    for name, force in (("lds_or_scratch", False), ("scratch", True)):
        stages["ms_edit_distance_" + name] = median_event_ms(lambda: chk.edit_distance(refs, dec["hyp_id"], dec["n_hyp"], rag, force), args.reps, args.rounds)
    # the edit distance at full size: every utterance's hypothesis as long as its frames (the bound the host sizes the slot for)
    full = {"hyp_id": torch.randint(0, 40, (logits.shape[0],), dtype=torch.int32, device=dev),
            "n_hyp": torch.tensor(rag.lengths, dtype=torch.int32, device=dev)}
    stages["ms_edit_distance_hyp_as_long_as_frames"] = median_event_ms(lambda: chk.edit_distance(refs, full["hyp_id"], full["n_hyp"], rag), args.reps, args.rounds)
    stages["ms_ctc_loss"] = median_event_ms(lambda: scorer.ctc_loss_batch(chk.ops, logits, rag, ids), args.reps, args.rounds)
    stages["ms_mas_durations"] = median_event_ms(lambda: al.durations(logits, rag, ids, flags), args.reps, args.rounds)
    dur, _ = al.durations(logits, rag, ids, flags)
    stages["ms_phone_posteriors"] = median_event_ms(lambda: chk.phone_posteriors(logits, rag, dur, full_ids), args.reps, args.rounds)

    new = {b: stages["ms_ctc_best_path" if b == 0 else f"ms_ctc_beam_search_{b}"] + stages["ms_edit_distance_lds_or_scratch"] +
           stages["ms_phone_posteriors"] for b in (0, 8, 32)}
    out = {
        "metric": "pronunciation_ms_per_batch", "utterances": B, "phonemes": args.phonemes, "seconds": args.seconds, "frames": rag.lengths[0],
        "tokens_full_text": len(feats[0]), "steps": args.steps, "reps": args.reps, "rounds": args.rounds,
        **{f"ms_check_beam_{b}": round(wall[b], 3) for b in (0, 8, 32)},
        "utterances_per_s_beam_8": round(1e3 * B / wall[8], 1),
        "ms_waves_to_16k_with_host_round_trip_1_call": round(ms_16k, 4), "ms_stft_and_log_mel": round(ms_front, 4),
        "ms_aligner_forward_1_call": round(ms_aligner, 4),
        "lstm_launches": rag.max_len, **{k: round(v, 4) for k, v in stages.items()},
        **{f"new_kernels_share_of_check_beam_{b}": round(new[b] / wall[b], 4) for b in (0, 8, 32)},
        "aligner_share_of_check_beam_8": round(ms_aligner / wall[8], 4),
        "n_hyp_mean_beam_32": round(float(np.mean([r["n_hyp"] for r in res])), 2) if res else None,
        "per_mean": round(float(np.mean([r["per"] for r in res])), 4), "gop_mean": round(float(np.mean([r["gop_mean"] for r in res])), 4),
        "gpu": torch.cuda.get_device_name(dev),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
