"""Golden vectors for the aligner's on-line fine-tuning (UtteranceCloner.extract_prosody with on_line_fine_tune=True,
UtteranceCloner.py:75-94).  Runs ONLY where the reference exists; stores data only (tests/golden/aligner/finetune.npz).

Per case it runs the reference's own classes in the reference's loop - ``Aligner`` in training mode, its ``ctc_loss``, ``SGD(lr=0.1)``,
``clip_grad_norm_(..., 1.0)``, five steps, then ``eval()`` - on the seeded fixture weights and a seeded mel
(``fixture_weights.aligner_spectrogram(seed, T)``), with ``torch.manual_seed(seed)`` before the loop, so that the reference's own
``nn.Dropout`` draws the masks; it asserts that ``finetune.dropout_masks(seed, T)`` are those masks (the float32 restatement fed with
them lands on the reference's logits).  The same loop in float64 (the reference's modules ``.double()``, the dropout layers replaced by
the same masks) measures how far float32 rounding moves the fine-tuned logits: ``ft{c}_sens``, relative to the largest |logit|.

Input selection, as make_aligner_golden.py does for the MAS margins: seeds are tried from each case's start until the sensitivity is
<= 1e-4, the durations of the float32 reference, the float64 reference and tests/finetune_ref.py agree with a MAS margin of at
least 64 ulps in each, finetune_ref (float64) reproduces the stored losses, norms and running statistics within 8 x that sensitivity
(floor 1e-5), and a second float32 order (finetune_ref in float32) stays within 8 x that sensitivity of the reference.  Cases: (T 61, L 9) from seed 3, (T 97, L 31) from seed 5, and the text of make_aligner_golden's second clone
case (word boundaries, a repeated phoneme) on a seeded mel of 89 frames from seed 7.

It prints the reference's CPU time for the five steps at the bench shape (625 frames x 100 tokens).

    python tests/golden/make_finetune_golden.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_aligner_golden as mag  # noqa: E402  (stand-ins for unused third-party imports, sys.path, the reference's Aligner)
import torch  # noqa: E402

from ims_toucan_prosody_variance_amd import align, finetune, fixture_weights as fw, phonemes  # noqa: E402
from tests import aligner_ref as ar  # noqa: E402
from tests import finetune_ref as fr  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.AutoAligner.Aligner import Aligner  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.FastSpeech2.DurationCalculator import DurationCalculator  # noqa: E402

CASES = [(61, 9, 3, None), (97, 31, 5, None), (89, None, 7, 1)]  # (frames, tokens, first seed, index into make_aligner_golden.CLONE_CASES)
MAX_SENS, MIN_ULPS, STEPS = 1e-4, mag.MIN_ULPS, 5


class MaskDropout(torch.nn.Module):
    """Stands in for nn.Dropout(0.5) in the float64 run: the next stored mask, times 2."""

    def __init__(self, feed):
        super().__init__()
        self.feed = feed

    def forward(self, x):
        if not self.training:
            return x
        return x * torch.as_tensor(next(self.feed), dtype=x.dtype)[None] * 2.0


def reference_loop(sd, mel, ids, seed, masks=None, dtype=torch.float32):
    """The reference's fine-tuning loop on its own modules.  masks None: its own nn.Dropout after torch.manual_seed(seed)."""
    model = Aligner()
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(dtype)
    if masks is not None:
        feed = iter([m for step in masks for m in step])
        for i in range(1, 10, 2):
            model.convs[i] = MaskDropout(feed)
    tokens = torch.LongTensor(np.asarray(ids))
    tokens_len = torch.LongTensor([len(tokens)])
    x = torch.from_numpy(np.asarray(mel)).to(dtype)[None]
    mel_len = torch.LongTensor([x.shape[1]])
    optim = torch.optim.SGD(model.parameters(), lr=0.1)
    model.train()
    torch.manual_seed(int(seed))
    losses, norms = [], []
    for _ in range(STEPS):
        pred = model(x)
        loss = model.ctc_loss(pred.transpose(0, 1).log_softmax(2), tokens, mel_len, tokens_len)
        optim.zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)))
        optim.step()
        losses.append(float(loss.detach()))
    model.eval()
    with torch.no_grad():
        logits = model(x)[0].numpy()
    return model, logits, np.array(losses), np.array(norms)


def main():
    sd = fw.aligner_state_dict()
    dc = DurationCalculator(reduction_factor=1)
    out = {}
    for c, (T, L, first, clone) in enumerate(CASES):
        for seed in range(first, first + 300):
            mel = fw.aligner_spectrogram(seed, T)
            phones = mag.symbols_for(L, seed) if clone is None else mag.CLONE_CASES[clone]
            feats = phonemes.phones_to_features(phones, handle_missing=False)
            ids, flags = align.token_ids(feats)
            masks = finetune.dropout_masks(seed, T)
            model, lg32, loss32, norm32 = reference_loop(sd, mel, ids, seed)
            _, lg64, _, _ = reference_loop(sd, mel, ids, seed, masks=masks, dtype=torch.float64)
            top = float(np.abs(lg64).max())
            sens = float(np.abs(lg32 - lg64).max()) / top
            if sens > MAX_SENS:
                print(f"case {c} seed {seed}: fp32-vs-fp64 sensitivity {sens:.1e} of max |logit|: skipped")
                continue
            mine = fr.fine_tune(sd, mel, ids, masks)
            durs = [ar.mas(np.asarray(l, dtype=np.float32)[:, ids], log64=True) for l in (lg32, lg64, mine["logits"])]
            ulps = min(d[2] for d in durs)
            if not (np.array_equal(durs[0][0], durs[1][0]) and np.array_equal(durs[0][0], durs[2][0]) and ulps >= MIN_ULPS):
                print(f"case {c} seed {seed}: durations disagree or margin {ulps:.0f} ulps: skipped")
                continue
            # the stored per-step losses and norms and the running statistics must be as insensitive as the logits
            rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(1.0, float(np.abs(np.asarray(b)).max()))
            stat32 = lambda k: np.stack([model.state_dict()[f"convs.{2 * i}.bnorm.{k}"].numpy() for i in range(5)])
            stat64 = lambda k: np.stack([mine["state"][f"convs.{2 * i}.bnorm.{k}"] for i in range(5)])
            others = {"loss": float(np.abs(mine["loss"] - loss32).max() / loss32.max()), "norm": float(np.abs(mine["norm"] - norm32).max() / norm32.max()),
                      "running_mean": rel(stat64("running_mean"), stat32("running_mean")), "running_var": rel(stat64("running_var"), stat32("running_var"))}
            if max(others.values()) > max(8 * sens, 1e-5):
                print(f"case {c} seed {seed}: {others} beyond 8 x the sensitivity {sens:.1e}: skipped")
                continue
            # a second sample of the rounding sensitivity: the float32 restatement (another float32 order than the reference's)
            mine32 = fr.fine_tune(sd, mel, ids, masks, dtype=torch.float32)
            e32 = float(np.abs(mine32["logits"] - lg32).max()) / top
            if e32 > max(8 * sens, 1e-5):
                print(f"case {c} seed {seed}: two float32 orders differ by {e32:.1e}, more than 8 x the sensitivity {sens:.1e}: skipped")
                continue
            break
        else:
            raise SystemExit(f"case {c}: no seed found")
        # the reference's own alignment with the fine-tuned model
        with torch.inference_mode():
            nb = [int(i) for i in np.nonzero((flags & 1) == 0)[0]]
            path = model.inference(mel=torch.from_numpy(mel), tokens=torch.from_numpy(feats[nb]), return_ctc=False)
            dur_nb = dc(torch.LongTensor(path), vis=None).numpy()
        assert np.array_equal(dur_nb, durs[0][0]), (dur_nb, durs[0][0])
        dur = ar.postprocess(dur_nb, flags)  # zeros at the word boundaries and the repair of repeated phonemes (UtteranceCloner.py:95-131)
        # the recipe's masks are the reference's: the float32 restatement fed with them lands on its logits, the float64 one on its float64 logits
        e64 = float(np.abs(mine["logits"] - lg64).max()) / top
        assert e32 <= max(8 * sens, 1e-5) and e64 <= 1e-9, (e32, e64)
        state = model.state_dict()
        rm = np.stack([state[f"convs.{2 * i}.bnorm.running_mean"].numpy() for i in range(5)])
        rv = np.stack([state[f"convs.{2 * i}.bnorm.running_var"].numpy() for i in range(5)])
        assert max(others.values()) <= max(8 * sens, 1e-5), others
        moved = float(np.abs(lg32 - ar.aligner_logits(align.pack_aligner(sd), mel)).max())
        before = ar.mas(ar.aligner_logits(align.pack_aligner(sd), mel)[:, ids], log64=True)[0]
        print(f"case {c}: T {T} L {len(ids)} seed {seed}: sens {sens:.1e}, restatement fp32 {e32:.1e} fp64 {e64:.1e}, margin {ulps:.0f} ulps, "
              f"loss {loss32.round(3).tolist()}, norm {norm32.round(2).tolist()}, logits moved by {moved:.2f} (max |logit| {top:.2f}), "
              f"durations changed: {not np.array_equal(before, dur_nb)}")
        m8 = np.stack([np.stack(step) for step in masks])  # [5, 5, T, 512] bool
        out.update({f"ft{c}_seed": np.int64(seed), f"ft{c}_frames": np.int64(T), f"ft{c}_ids": ids.astype(np.int32), f"ft{c}_flags": flags,
                    f"ft{c}_masks": np.packbits(m8.reshape(-1)), f"ft{c}_loss": loss32, f"ft{c}_norm": norm32, f"ft{c}_logits": lg32.astype(np.float32),
                    f"ft{c}_running_mean": rm, f"ft{c}_running_var": rv, f"ft{c}_dur": dur, f"ft{c}_sens": np.float64(sens),
                    f"ft{c}_phones": np.array(phones)})
    out["n_cases"] = np.int64(len(CASES))
    np.savez_compressed(os.path.join(HERE, "aligner", "finetune.npz"), **out)
    print("wrote finetune.npz")

    # the reference's CPU time for the five steps at the bench shape
    mel = fw.aligner_spectrogram(99, 625)
    ids, _ = align.token_ids(phonemes.phones_to_features(mag.symbols_for(100, 99), handle_missing=False))
    t0 = time.perf_counter()
    reference_loop(sd, mel, ids, 99)
    print(f"reference fine-tuning (5 steps + eval logits), 625 frames x 100 tokens, CPU ({torch.get_num_threads()} threads): "
          f"{time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()
