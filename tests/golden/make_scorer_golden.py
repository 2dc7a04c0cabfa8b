"""Golden vectors for the corpus scorer (Utility/Scorer.py: AlignmentScorer, TTSScorer).  Runs ONLY where the reference exists.

Runs the reference's own code, in eval mode (the reference's scorers never call ``.eval()``: their own scores carry dropout and
batch-of-one BatchNorm statistics, a random result - INTEGRATION.md), with the seeded fixture weights loaded through strict
``load_state_dict``:

* CTC: ``Aligner`` with ``fixture_weights.aligner_state_dict`` on seeded mels (``fixture_weights.aligner_spectrogram(u, T)``, the
  seed stored) and seeded id sequences: a typical utterance, repeated consecutive ids, T barely feasible, T infeasible (the loss is
  0 through zero_infinity), one id, and a long case (T ~ 4000, whose logits are not stored).  The loss is formed as
  ``Aligner.inference(..., return_ctc=True)`` forms it (Aligner.py:105-107, the model's own ``ctc_loss`` module); beside it
  ``torch.nn.functional.ctc_loss`` in float64 on the same fp32 log-probabilities.
* TTS: the reference's TRAINING ``ToucanTTS`` (ToucanTTS.py:210-272, ``run_glow=False``) with ``StyleEmbedding`` and its
  ``ToucanTTSLoss``, called as ``TTSScorer.score`` calls them (Scorer.py:120-133), on ``write_fixture_corpus`` data, for the
  multilingual / multi-speaker checkpoint and the two fallback variants (``lang_embs=None``; ``lang_embs=None, utt_embed_dim=None``).
  Every fixture utterance carries nonzero gold pitch on its word boundaries and unvoiced phonemes, so an inference-time override
  would change the result.  The four losses per utterance are stored, and ``before_outs`` / ``after_outs`` of one utterance.

It asserts that tests/scorer_ref.py reproduces every stored value, restates the losses at batch 1 as ToucanTTSLoss writes them
(the variance weights applied twice sum to 1), stores everything in ``tests/golden/scorer/scorer.npz`` (data only) and prints the
reference's CPU time per utterance of the bench shape (625 frames, 100 phonemes) for each scorer.

    python tests/golden/make_scorer_golden.py
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stand-ins for unused third-party imports + sys.path)
import torch  # noqa: E402

make_golden._stub("parselmouth")
make_golden._stub("torch_complex")
make_golden._stub("torch_complex.tensor", ComplexTensor=make_golden._Dummy)

from ims_toucan_prosody_variance_amd import fixture_weights as fw, phonemes, scorer  # noqa: E402
from tests import scorer_ref as sr  # noqa: E402
from Preprocessing.TextFrontend import get_language_id  # noqa: E402
from TrainingInterfaces.Spectrogram_to_Embedding.StyleEmbedding import StyleEmbedding  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.AutoAligner.Aligner import Aligner  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.ToucanTTS.ToucanTTS import ToucanTTS  # noqa: E402

OUT = os.path.join(HERE, "scorer")
LOGITS_MAX_T = 1000  # the reference's logits are stored up to this many frames
CORPUS = dict(n=5, seed=7)  # write_fixture_corpus arguments of the TTS cases
VARIANTS = [("meta", dict(), dict()), ("monolingual", dict(n_lang=None, multispeaker=True), dict(lang_embs=None)),
            ("single", dict(n_lang=None, multispeaker=False), dict(lang_embs=None, utt_embed_dim=None))]


def seeded_ids(name, n, repeats=0):
    ids = (fw.uniform01("ctc.ids." + name, n, 5) * 110).astype(np.int64)  # ids of real symbols (0 .. 109), never the blank 144
    for k in range(1, n):
        if ids[k] == ids[k - 1]:
            ids[k] = (ids[k] + 1) % 110
    for k in range(repeats):  # k-th repeat: position 3 + 4k copies its predecessor
        p = 3 + 4 * k
        ids[p] = ids[p - 1]
    return ids


def min_frames(ids):
    return len(ids) + int(sum(1 for a, b in zip(ids[:-1], ids[1:]) if a == b))


def ctc_cases():
    """(name, frames, ids): ids seeded per case; "repeats" has consecutive equal ids; "feasible" / "infeasible" sit at / one frame
    below the shortest alignment (n + the number of adjacent equal pairs)."""
    rep = seeded_ids("repeats", 30, repeats=6)
    tight = seeded_ids("tight", 20, repeats=3)
    return [("typical", 200, seeded_ids("typical", 40)), ("repeats", 120, rep), ("feasible", min_frames(tight), tight),
            ("infeasible", min_frames(tight) - 1, tight), ("one_id", 50, seeded_ids("one", 1)), ("long", 4003, seeded_ids("long", 350, repeats=20))]


def ref_aligner():
    m = Aligner()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in fw.aligner_state_dict().items()}, strict=True)
    return m.eval()


def make_ctc(g):
    al = ref_aligner()
    meta = []
    for c, (name, T, ids) in enumerate(ctc_cases()):
        u = 500 + c
        mel = torch.from_numpy(fw.aligner_spectrogram(u, T))
        with torch.inference_mode():
            pred = al(mel.unsqueeze(0))  # Aligner.inference :104
            logp = pred.transpose(0, 1).log_softmax(2)
            loss = al.ctc_loss(logp, torch.LongTensor(ids), torch.LongTensor([len(pred[0])]), torch.LongTensor([len(ids)])).item()  # :106-107
            f64 = torch.nn.functional.ctc_loss(logp.double(), torch.LongTensor(ids), torch.LongTensor([T]), torch.LongTensor([len(ids)]),
                                               blank=144, reduction="mean", zero_infinity=True).item()
        lp = logp[:, 0].numpy()
        mine = sr.ctc_loss(lp, ids)
        assert abs(mine - f64) <= 1e-12 * max(1.0, abs(f64)), (name, mine, f64)
        assert abs(loss - f64) <= 1e-5 * max(1.0, abs(f64)), (name, loss, f64)
        if name == "infeasible":
            assert loss == 0.0 and f64 == 0.0
        else:
            assert f64 > 0
        g[f"ctc_{name}_ids"] = ids.astype(np.int32)
        g[f"ctc_{name}_u"] = np.int64(u)
        g[f"ctc_{name}_T"] = np.int64(T)
        g[f"ctc_{name}_ref"] = np.float32(loss)
        g[f"ctc_{name}_f64"] = np.float64(f64)
        if T <= LOGITS_MAX_T:
            g[f"ctc_{name}_logits"] = pred[0].numpy().astype(np.float32)
        meta.append(name)
        print(f"ctc {name:10s} T {T:5d} n {len(ids):4d}: reference fp32 {loss:.9g}, float64 {f64:.12g}, restated {mine:.12g}")
    g["ctc_cases"] = np.array(json.dumps(meta))


def ref_tts(sd, kw):
    m = ToucanTTS(**kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


def ref_style():
    s = StyleEmbedding()
    s.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in fw.style_state_dict().items()}, strict=True)
    return s.eval()


def make_tts(g):
    style = ref_style()
    lang = get_language_id("en")
    with tempfile.TemporaryDirectory() as d:
        fw.write_fixture_corpus(d, **CORPUS)
        datapoints, items = scorer.read_tts_cache(d)
    for it in items:  # word boundaries and unvoiced phonemes with nonzero gold pitch in every utterance
        wb = it["text"][:, phonemes.IDX["word_boundary"]] != 0
        unv = (it["text"][:, phonemes.IDX["phoneme"]] != 0) & (it["text"][:, phonemes.IDX["voiced"]] == 0)
        assert wb.any() and unv.any() and (it["pitch"][wb] != 0).all() and (it["pitch"][unv] != 0).all()
    for name, fw_kw, ref_kw in VARIANTS:
        sd = fw.acoustic_state_dict(**fw_kw)
        m = ref_tts(sd, ref_kw)
        losses, embs = [], []
        for index, dp in enumerate(datapoints):
            text, text_len, spec, spec_len, duration, energy, pitch, embed, filepath = dp
            with torch.inference_mode():
                se = style(batch_of_spectrograms=spec.unsqueeze(0), batch_of_spectrogram_lengths=spec_len.unsqueeze(0))
                kw = dict(text_tensors=text.unsqueeze(0), text_lengths=text_len, gold_speech=spec.unsqueeze(0), speech_lengths=spec_len,
                          gold_durations=duration.unsqueeze(0), gold_pitch=pitch.unsqueeze(0), gold_energy=energy.unsqueeze(0),
                          utterance_embedding=se, lang_ids=lang.unsqueeze(0))
                l1, dl, pl, el, _ = m(**kw, return_mels=False, run_glow=False)  # Scorer.py:120-130
                before, after, pd, pp, pe, _ = m._forward(text_tensors=kw["text_tensors"], text_lengths=text_len, gold_speech=kw["gold_speech"],
                                                          speech_lengths=spec_len, gold_durations=kw["gold_durations"],
                                                          gold_pitch=kw["gold_pitch"], gold_energy=kw["gold_energy"], is_inference=False,
                                                          utterance_embedding=se, lang_ids=kw["lang_ids"], run_glow=False)
            ref = np.array([l1.item(), dl.item(), pl.item(), el.item()])
            # ToucanTTSLoss applies the variance weights twice (:57-58 and :63-64); at batch 1 they sum to 1: the restatement is the plain mean
            mine = sr.tts_losses(before[0].numpy(), after[0].numpy(), spec.numpy(), pd[0].numpy(), pp[0].numpy(), pe[0].numpy(),
                                 duration.numpy(), pitch.numpy(), energy.numpy())
            assert np.all(np.abs(mine - ref) <= 2e-6 * np.abs(ref) + 1e-9), (name, index, mine, ref)
            losses.append(ref)
            embs.append(se[0].numpy())
            if name == "meta" and index == 0:
                g["tts_meta_before0"] = before[0].numpy().astype(np.float32)
                g["tts_meta_after0"] = after[0].numpy().astype(np.float32)
                g["tts_meta_pred0"] = np.stack([pd[0].numpy(), pp[0, :, 0].numpy(), pe[0, :, 0].numpy()]).astype(np.float32)
        g[f"tts_{name}_losses"] = np.array(losses, dtype=np.float64)
        g[f"tts_{name}_style"] = np.array(embs, dtype=np.float32)
        g[f"tts_{name}_fixture"] = np.array(json.dumps(fw_kw))
        print(f"tts {name:12s}: losses (l1, dur, pitch, energy) per utterance\n{np.array(losses)}")
    g["tts_corpus"] = np.array(json.dumps(CORPUS))
    g["tts_lang_id"] = np.int64(lang.item())


def cpu_times():
    al = ref_aligner()
    ids = seeded_ids("bench", 100)
    mel = torch.from_numpy(fw.aligner_spectrogram(900, 625))
    with torch.inference_mode():
        al(mel.unsqueeze(0))
        t0 = time.perf_counter()
        for _ in range(3):
            pred = al(mel.unsqueeze(0))
            al.ctc_loss(pred.transpose(0, 1).log_softmax(2), torch.LongTensor(ids), torch.LongTensor([625]), torch.LongTensor([100])).item()
        ta = (time.perf_counter() - t0) / 3
    m, style = ref_tts(fw.acoustic_state_dict(), {}), ref_style()
    with tempfile.TemporaryDirectory() as d:
        fw.write_fixture_corpus(d, n=3, seed=99, words=(20, 22), max_duration=15)
        datapoints, _ = scorer.read_tts_cache(d)
    lang = get_language_id("en")
    with torch.inference_mode():
        t0 = time.perf_counter()
        for dp in datapoints:
            text, text_len, spec, spec_len, duration, energy, pitch, _, _ = dp
            se = style(batch_of_spectrograms=spec.unsqueeze(0), batch_of_spectrogram_lengths=spec_len.unsqueeze(0))
            m(text_tensors=text.unsqueeze(0), text_lengths=text_len, gold_speech=spec.unsqueeze(0), speech_lengths=spec_len,
              gold_durations=duration.unsqueeze(0), gold_pitch=pitch.unsqueeze(0), gold_energy=energy.unsqueeze(0), utterance_embedding=se,
              lang_ids=lang.unsqueeze(0), return_mels=False, run_glow=False)
        tt = (time.perf_counter() - t0) / len(datapoints)
    shapes = [(int(dp[1][0]), int(dp[3][0])) for dp in datapoints]
    print(f"reference CPU time per utterance ({torch.get_num_threads()} threads): AlignmentScorer {ta:.3f} s (625 frames, 100 ids); "
          f"TTSScorer {tt:.3f} s ((phonemes, frames) {shapes})")


def main():
    os.makedirs(OUT, exist_ok=True)
    g = {}
    make_ctc(g)
    make_tts(g)
    np.savez_compressed(os.path.join(OUT, "scorer.npz"), **g)
    print("wrote", os.path.join(OUT, "scorer.npz"), os.path.getsize(os.path.join(OUT, "scorer.npz")), "bytes")
    cpu_times()


if __name__ == "__main__":
    main()
