"""Golden vectors for the prosody cloner's extraction path (UtteranceCloner.extract_prosody).  Runs ONLY where the reference exists.

Runs the reference's own code with the seeded fixture aligner weights (``fixture_weights.aligner_state_dict``, loaded through the
reference's strict ``load_state_dict``):

* ``Aligner.inference`` (MAS) + ``DurationCalculator`` on seeded mels (``fixture_weights.aligner_spectrogram(seed, T)``, the seed stored), T < L, T == L, L == 1 and a long case (T ~ 4000, whose
  logits are not stored: 2.3 MB; its durations are checked from the restated and the GPU logits, asserted here to give the same);
* ``binarize_alignment`` + ``DurationCalculator`` on crafted matrices with exact ties;
* the whole ``extract_prosody`` body on seeded waves (``fixture_weights.reference_wave``, the seed stored), with stand-ins only at the edges that are unavailable offline: an instance
  made with ``UtteranceCloner.__new__``, ``sf.read``, the silero ``get_speech_timestamps`` (the whole wave is speech), Praat's
  ``_calculate_f0`` (a seeded track), the audio preprocessor (peak normalisation, and a float64 restatement of the log-mel because
  librosa is absent - the mel is stored as an input) and ``string_to_tensor`` with ``input_phonemes=True``.

It asserts that tests/aligner_ref.py reproduces every stored duration / energy / pitch, stores inputs and outputs in
``tests/golden/aligner/aligner.npz`` (data only), captures the aligner id of every phoneme symbol (``get_phone_to_id`` resolved through
``text_vectors_to_id_sequence``) into ``ims-toucan-prosody-variance_amd/data/phone_ids.json``, and the reference's id sequences for
the strings of frontend.json into ``tests/golden/aligner/aligner_ids.json``.  It prints the MAS decision margins and the reference's CPU
time for one utterance of the bench shape (625 frames, 100 tokens).

    python tests/golden/make_aligner_golden.py
"""
import functools
import json
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stand-ins for unused third-party imports + sys.path)
import torch  # noqa: E402

make_golden._stub("parselmouth")
make_golden._stub("torch_complex")
make_golden._stub("torch_complex.tensor", ComplexTensor=make_golden._Dummy)

from ims_toucan_prosody_variance_amd import align, fixture_weights as fw, phonemes, style  # noqa: E402
from tests import aligner_ref as ar  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.AutoAligner.Aligner import Aligner, binarize_alignment  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.FastSpeech2.DurationCalculator import DurationCalculator  # noqa: E402
from TrainingInterfaces.Text_to_Spectrogram.FastSpeech2.PitchCalculator import Parselmouth  # noqa: E402
from InferenceInterfaces import UtteranceCloner as uc_mod  # noqa: E402

REPO = make_golden.REPO
MAS_CASES = [(5, 9), (12, 12), (50, 1), (200, 31), (640, 97), (4003, 350)]  # (frames, tokens)
CLONE_CASES = [  # phoneme strings with word boundaries, 2 and 3 repeated phonemes, nasal vowels, non-phoneme tokens
    "~həlˈoʊ wˈɜːld~#",
    "~bɔ̃ʒˈuʁ mˈɛsjø lɛ ssˈɑ̃ zˈaaa?~#",
    "~ˈɪt ɪz nnˈaʊ ˈɔːlmoʊst tˈɛn!~#",
]
CLONE_SAMPLES = [256 * 120 + 77, 256 * 301 + 3, 256 * 233 + 200]
MIN_ULPS = 64  # smallest accepted MAS decision margin, in ulps of the compared scores
LOGITS_MAX_T = 1000  # the reference's logits are stored up to this many frames; longer cases keep their durations only


class EvalAligner(Aligner):
    """extract_prosody builds Aligner() and calls eval() only after the on-line fine-tuning (UtteranceCloner.py:57-93): with
    on_line_fine_tune=False the reference aligns in TRAINING mode (dropout 0.5, batch statistics), a random result.  The golden
    takes the eval-mode model, i.e. the fine-tuning path's mode without its five SGD steps."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.eval()


def ref_aligner(sd):
    m = Aligner()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


def symbols_for(n, u):
    """n seeded phoneme symbols (no boundaries, no punctuation) as a string for phones_to_features."""
    table = phonemes.phone_table()
    syms = sorted(s for s, v in table.items() if v[15] == 1 and v[21] == 0)
    idx = (fw.uniform01("alsyms%d" % u, n, 77) * len(syms)).astype(int)
    return "".join(syms[i] for i in idx)


def dump_phone_ids(tf):
    ids = {}
    for sym in sorted(phonemes.phone_table()):
        if sym not in tf.phone_to_vector:
            continue
        seq = tf.text_vectors_to_id_sequence(text_vector=torch.tensor([tf.phone_to_vector[sym]], dtype=torch.float32))
        if seq:
            ids[sym] = int(seq[0])
    path = os.path.join(REPO, "ims-toucan-prosody-variance_amd", "data", "phone_ids.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(ids, f, ensure_ascii=False, sort_keys=True, indent=0)
    print(f"wrote {path}: {len(ids)} symbols")
    align._PHONE_IDS = align._KEY_TO_ID = None


def dump_frontend_ids(tf):
    cases = json.load(open(os.path.join(HERE, "frontend.json"), encoding="utf-8"))["cases"]
    out = []
    for c in cases:
        vec = tf.string_to_tensor(c["phones"], handle_missing=True, input_phonemes=True)
        ref = [int(i) for i in tf.text_vectors_to_id_sequence(text_vector=vec)]
        mine = align.token_ids(phonemes.phones_to_features(c["phones"], handle_missing=True))[0].tolist()
        assert ref == mine, (c["phones"], ref, mine)
        out.append({"phones": c["phones"], "ids": ref})
    with open(os.path.join(HERE, "aligner", "aligner_ids.json"), "w", encoding="utf-8") as f:
        json.dump({"cases": out}, f, ensure_ascii=False, indent=1)
    print(f"wrote aligner_ids.json: {len(out)} strings")


def logmel64(wave):
    """float64 restatement of AudioPreprocessor.logmelfilterbank (librosa.stft centre/reflect, |X|, Slaney mel, log10 floor)."""
    x = np.pad(np.asarray(wave, np.float64), 512, mode="reflect")
    n = 1 + (len(x) - 1024) // 256
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1024) / 1024)
    frames = np.stack([x[i * 256:i * 256 + 1024] * win for i in range(n)])
    mag = np.abs(np.fft.rfft(frames, axis=1))
    mel = mag @ style.mel_filterbank().astype(np.float64).T
    return np.log10(np.maximum(1e-10, mel)).astype(np.float32)  # [frames, 80]


def seeded_f0(u, frames):
    n = frames - 3 + 2 * (u % 3)  # shorter and longer than the mel: exercises the centred pad and the truncation
    f = 100.0 + 80.0 * fw.uniform01("clone.f0%d" % u, n, 12000 + u)
    f[fw.uniform01("clone.uv%d" % u, n, 12000 + u) < 0.25] = 0.0
    return f.astype(np.float32)


def main():
    sd = fw.aligner_state_dict()
    model = ref_aligner(sd)
    tf = model.tf
    dump_phone_ids(tf)
    dump_frontend_ids(tf)
    packed = align.pack_aligner(sd)
    dc = DurationCalculator(reduction_factor=1)
    out = {}
    with torch.inference_mode():
        for c, (T, L) in enumerate(MAS_CASES):
            for u in range(c, c + 400, 10):  # the first seed whose MAS decisions are far from fp32 rounding (the restatement decides)
                mel = fw.aligner_spectrogram(u, T)
                feats = phonemes.phones_to_features(symbols_for(L, u), handle_missing=False)
                ids, _ = align.token_ids(feats)
                if ar.mas(ar.aligner_logits(packed, mel)[:, ids])[2] >= MIN_ULPS:
                    break
            logits = model(torch.from_numpy(mel)[None])[0].numpy()
            t0 = time.perf_counter()
            path = model.inference(mel=torch.from_numpy(mel), tokens=torch.from_numpy(feats), return_ctc=False)
            dt = time.perf_counter() - t0
            dur = dc(torch.LongTensor(path), vis=None).numpy()
            mine, margin, ulps = ar.mas(logits[:, ids])
            assert np.array_equal(mine, dur), (T, L, mine, dur)
            assert np.array_equal(ar.mas(logits[:, ids], log64=True)[0], dur), "the kernel's correctly rounded log changes the path"
            ol = ar.aligner_logits(packed, mel)
            err = float(np.abs(ol - logits).max() / np.abs(logits).max())
            assert err < 1e-5, err
            # the restated (and the GPU's) logits differ from the reference's by ~1e-6: the stored durations must not depend on that
            assert np.array_equal(ar.mas(ol[:, ids], log64=True)[0], dur), "durations change under the restated logits"
            print(f"mas case {c}: T {T} L {L}: durations {dur.min()}..{dur.max()}, min margin {margin:.3e} ({ulps:.0f} ulps), folded-weight "
                  f"logits rel err {err:.1e}, reference inference {dt:.3f} s")
            out[f"mas{c}_ids"], out[f"mas{c}_dur"] = ids, dur  # mel: the seed below
            if T <= LOGITS_MAX_T:
                out[f"mas{c}_logits"] = logits.astype(np.float32)
            out[f"mas{c}_margin"] = np.float64(margin)
            out[f"mas{c}_seed"] = np.int64(u)
        # crafted matrices with exact ties (equal columns, constant rows, equal path sums)
        ties = [np.zeros((6, 4), np.float32), np.ones((7, 3), np.float32), np.tile(np.float32([0.5, 0.25, 0.5, 0.25]), (9, 1)),
                np.float32([[1, 0, 0], [0, 1, 0], [1, 1, 1], [0, 0, 1], [1, 1, 1]]), np.full((3, 5), -2.0, np.float32)]
        for k, m in enumerate(ties):
            dur = dc(torch.LongTensor(binarize_alignment(m.copy())), vis=None).numpy()
            assert np.array_equal(ar.mas(m)[0], dur), (k, dur)
            out[f"tie{k}_p"], out[f"tie{k}_dur"] = m, dur
            print(f"tie case {k}: {m.shape} -> {dur.tolist()}")

        # the whole extract_prosody body
        cl = uc_mod.UtteranceCloner.__new__(uc_mod.UtteranceCloner)
        cl.tf = tf
        tf.string_to_tensor = functools.partial(type(tf).string_to_tensor, tf, input_phonemes=True)
        cl.device = "cpu"
        cl.aligner_weights = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
        cl.silero_model = None
        cl.get_speech_timestamps = lambda wave, model, sampling_rate: [{"start": 0, "end": len(wave)}]
        state = {}
        cl.ap = types.SimpleNamespace(
            sr=16000,
            audio_to_wave_tensor=lambda normalize, audio: torch.from_numpy(style.normalize_reference_audio(audio, 16000)),
            audio_to_mel_spec_tensor=lambda audio, normalize, explicit_sampling_rate: torch.from_numpy(state["mel"].T.copy()))
        uc_mod.sf.read = lambda path: (state["wave"], 16000)
        Parselmouth._calculate_f0 = lambda self, x: torch.from_numpy(state["f0"])
        uc_mod.Aligner = EvalAligner
        for u, (ph, n) in enumerate(zip(CLONE_CASES, CLONE_SAMPLES)):
            feats = phonemes.phones_to_features(ph, handle_missing=False)
            ids, flags = align.token_ids(feats)
            for seed in range(u, u + 400, 10):
                wave = fw.reference_wave(seed, n)
                norm = style.normalize_reference_audio(wave, 16000)
                mel = logmel64(norm)
                if ar.mas(ar.aligner_logits(packed, mel)[:, ids])[2] >= MIN_ULPS:
                    break
            f0 = seeded_f0(u, mel.shape[0])
            state.update(wave=wave, mel=mel, f0=f0)
            dur, pitch, energy, s0, s1 = cl.extract_prosody(ph, "ref.wav", lang=tf.language, on_line_fine_tune=False)
            dur, pitch, energy = dur.numpy(), pitch.reshape(-1).numpy(), energy.reshape(-1).numpy()
            assert np.array_equal(flags, ar.flags_of(feats))
            logits = model(torch.from_numpy(mel)[None])[0].numpy()
            nb, margin, ulps = ar.mas(logits[:, ids])
            mine = ar.postprocess(nb, flags)
            assert np.array_equal(ar.mas(logits[:, ids], log64=True)[0], nb), "the kernel's correctly rounded log changes the path"
            assert np.array_equal(mine, dur), (u, mine, dur)
            ol = ar.aligner_logits(packed, mel)
            assert np.array_equal(ar.postprocess(ar.mas(ol[:, ids], log64=True)[0], flags), dur), "durations change under the restated logits"
            spec = np.fft.rfft(np.stack([np.pad(norm.astype(np.float64), 512, mode="reflect")[i * 256:i * 256 + 1024]
                                         * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)) for i in range(mel.shape[0])]), axis=1)
            e_frames = np.sqrt(np.maximum((np.abs(spec) ** 2).sum(1), 1e-10)).astype(np.float32)
            e_mine = ar.token_average(e_frames, dur, feats[:, 15] != 0, 0)
            p_mine = ar.token_average(ar.adjust_centered(f0, mel.shape[0]), dur, feats[:, 61] != 0, 1)
            e_err, p_err = float(np.abs(e_mine - energy).max()), float(np.abs(p_mine - pitch).max())
            assert e_err < 1e-5 and p_err < 1e-6, (e_err, p_err)
            print(f"clone case {u}: {len(ph)} chars, {len(dur)} tokens, {mel.shape[0]} frames, durations {dur.tolist()}, min margin "
                  f"{margin:.3e} ({ulps:.0f} ulps), energy err {e_err:.1e}, pitch err {p_err:.1e}, silences {s0} {s1}")
            # the wave is fixture_weights.reference_wave(seed, samples); the mel (float64 restatement) is stored as an input
            out.update({f"clone{u}_seed": np.int64(seed), f"clone{u}_samples": np.int64(n), f"clone{u}_mel": mel, f"clone{u}_f0": f0,
                        f"clone{u}_dur": dur, f"clone{u}_energy": energy,
                        f"clone{u}_pitch": pitch, f"clone{u}_margin": np.float64(margin)})
        out["clone_phones"] = np.array(CLONE_CASES)
        out["mas_cases"] = np.array(MAS_CASES)

        # the reference's CPU time for the bench shape (one utterance of 625 frames, 100 tokens; Aligner.inference, MAS included)
        mel = fw.aligner_spectrogram(99, 625)
        feats = torch.from_numpy(phonemes.phones_to_features(symbols_for(100, 99), handle_missing=False))
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            model.inference(mel=torch.from_numpy(mel), tokens=feats, return_ctc=False)
            ts.append(time.perf_counter() - t0)
        print(f"reference Aligner.inference, 625 frames x 100 tokens, CPU ({torch.get_num_threads()} threads): "
              f"{', '.join('%.3f' % t for t in ts)} s per utterance")
    np.savez_compressed(os.path.join(HERE, "aligner", "aligner.npz"), **out)
    print("wrote aligner.npz")


if __name__ == "__main__":
    main()
