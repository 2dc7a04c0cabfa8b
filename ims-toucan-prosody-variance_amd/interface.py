"""Drop-in counterpart of InferenceInterfaces/ToucanTTSInterface.py (:21-309) on the HIP engines.

Same class name, constructor keywords, methods and behaviour as the reference's ``ToucanTTSInterface`` so that a
script written against the reference (run_text_to_file_reader.py:8-16) works unchanged when this repository's
``InferenceInterfaces`` package is the one on ``sys.path``:

* path shorthand ``"Meta"`` -> ``Models/ToucanTTS_Meta/best.pt``; vocoder default ``Models/{Avocodo|BigVGAN}/best.pt`` (:33-40)
* checkpoints are the reference's own formats: ``{"model": state_dict, "default_emb": tensor}`` and ``{"generator": state_dict}``
  (run_weight_averaging.py:108-116); weight norm folding / flow inverses happen in ``packing.py``
* ``forward`` / ``__call__`` (:132-229), ``read_to_file`` (:231-285: 10 600 samples of silence around sentences, blank
  strings skipped, 24 kHz output or sample-doubled 48 kHz PCM16), ``read_aloud`` (:287-309), the language / embedding setters
* additive API: ``synthesize_batch`` (ragged batches, optionally sharded over the ranks of torch.distributed; every prosody scale
  a scalar or one value per utterance), ``synthesize_grid`` (one text over a grid of prosody scales, with the statistics of what
  each scale did), ``prosody_curves=`` / ``curves=`` (per-phoneme prosody curves: stress one word, prosody.emphasis),
  ``prosody_fit=`` (an utterance, its pauses or a span of phonemes in exactly N frames or seconds: prosody_fit.Fit),
  ``evaluate_against_recordings`` (synthesise and measure against recordings of the same sentences: MCD along a DTW path and
  the F0 errors, compare.py), ``check_pronunciation`` / ``synthesize_grid(check_pronunciation=True)`` (synthesise and ask the aligner
  whether the waveform still says the text, without a recording: phoneme error rate of the decoded CTC posteriors and per-phoneme
  goodness of pronunciation over the forced alignment, pronunciation.py), ``loudness=`` / ``peak_ceiling=`` (every utterance brought to a target integrated loudness after
  ITU-R BS.1770 under a sample-peak ceiling, on the device: loudness.py; ``true_peak_ceiling=`` / ``limiter=`` add a true-peak
  ceiling and a look-ahead limiter: truepeak.py), ``speech_level=`` (the same for the active
  speech level after ITU-T P.56: activity.py), ``trim_silence=`` on ``set_utterance_embedding``

* ``set_utterance_embedding(path)`` (:103-114): reference audio -> log-mel -> GST style embedding on the GPU (style.py)

What is NOT here (unavailable offline): grapheme-to-phoneme conversion (espeak-ng / phonemizer: raw text
raises - pass phoneme strings with ``input_is_phones=True``) and the silero voice-activity trim of the reference audio.
"""
import os
import warnings
import wave as _wave

import numpy as np
import torch

from . import engine, prosody
from . import prosody_fit as prosody_fit_mod
from .phonemes import ArticulatoryCombinedTextFrontend, get_language_id
from .ragged import Ragged

MODELS_DIR = os.environ.get("TOUCAN_MODELS_DIR", "Models/")  # Utility/storage_config.py:1


def float2pcm(sig, dtype="int16"):
    """Float waveform in [-1, 1) -> integer PCM the way the reference's writer does it (Utility/utils.py:20-33): scale by half the
    integer range around the type's mid point, saturate, and let the integer cast drop the fraction (no rounding step)."""
    sig, dt = np.asarray(sig), np.dtype(dtype)
    if sig.dtype.kind != "f":
        raise TypeError("'sig' must be a float array")
    if dt.kind not in "iu":
        raise TypeError("'dtype' must be an integer type")
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    half_range = float(1 << (8 * dt.itemsize - 1))
    mid = lo + half_range  # 0 for signed types, the centre of the range for unsigned ones
    return np.clip(sig * half_range + mid, lo, hi).astype(dt)


def write_wav(path, data, samplerate):
    """soundfile.write(file, data, samplerate) for a .wav target (PCM_16 is soundfile's WAV default); uses soundfile when present."""
    try:
        import soundfile
        soundfile.write(file=path, data=data, samplerate=samplerate, subtype="PCM_16")
        return
    except ImportError:
        pass
    pcm = data if np.asarray(data).dtype.kind in "iu" else float2pcm(np.asarray(data, dtype=np.float32))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with _wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(samplerate)
        f.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def _load_checkpoint(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: checkpoint not found (the reference downloads it with run_model_downloader.py; "
                                f"offline, write fixture checkpoints with ims_toucan_prosody_variance_amd.interface.write_fixture_checkpoints)")
    return torch.load(path, map_location="cpu", weights_only=True)


def _to_numpy_sd(sd):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}


def write_fixture_checkpoints(models_dir=MODELS_DIR, n_lang=8000):
    """Write the seeded fixture weights in the reference's checkpoint layout (Models/ToucanTTS_Meta, Avocodo, BigVGAN)."""
    from . import fixture_weights as fw
    t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    for sub, obj in (("ToucanTTS_Meta", {"model": t(fw.acoustic_state_dict(n_lang=n_lang)),
                                         "default_emb": torch.from_numpy(fw.default_utterance_embedding())}),
                     ("Avocodo", {"generator": t(fw.hifigan_state_dict())}),
                     ("BigVGAN", {"generator": t(fw.bigvgan_state_dict())}),
                     ("Embedding", {"style_emb_func": t(fw.style_state_dict())})):
        os.makedirs(os.path.join(models_dir, sub), exist_ok=True)
        torch.save(obj, os.path.join(models_dir, sub, "embedding_function.pt" if sub == "Embedding" else "best.pt"))


def write_fixture_aligner_checkpoint(models_dir=MODELS_DIR):
    """Write the seeded fixture aligner in the reference's layout: Models/Aligner/aligner.pt = {"asr_model": state_dict}
    (UtteranceCloner.py:33-34)."""
    from . import fixture_weights as fw
    os.makedirs(os.path.join(models_dir, "Aligner"), exist_ok=True)
    path = os.path.join(models_dir, "Aligner", "aligner.pt")
    torch.save({"asr_model": {k: torch.from_numpy(np.array(v)) for k, v in fw.aligner_state_dict().items()}}, path)
    return path


def write_fixture_gan_checkpoint(models_dir=MODELS_DIR, params=None, seed=2718):
    """Write the seeded fixture speaker-embedding GAN in the reference's layout (wgan_qc.py:260-275, read by GAN.py:32-40):
    Models/Embedding/embedding_gan.pt = {"model_parameters", "generator_state_dict", "critic_state_dict" (both "module."-prefixed),
    "dataset_mean", "dataset_std"}."""
    from . import fixture_weights as fw
    params = dict(fw.GAN_PARAMS if params is None else params)
    params["data_dim"] = tuple(params["data_dim"])
    gen, critic = fw.gan_state_dicts(params, seed)
    t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    mean, std = fw.gan_dataset_stats(params["data_dim"][-1], seed)
    os.makedirs(os.path.join(models_dir, "Embedding"), exist_ok=True)
    path = os.path.join(models_dir, "Embedding", "embedding_gan.pt")
    torch.save({"model_parameters": params, "generator_state_dict": t(gen), "critic_state_dict": t(critic),
                "dataset_mean": torch.from_numpy(mean), "dataset_std": torch.from_numpy(std)}, path)
    return path


class ToucanTTSInterface(torch.nn.Module):

    def __init__(self,
                 device="cpu",
                 tts_model_path=os.path.join(MODELS_DIR, "ToucanTTS_Meta", "best.pt"),
                 embedding_model_path=None,
                 vocoder_model_path=None,
                 faster_vocoder=True,
                 language="en"):
        super().__init__()
        self.device = device
        if not tts_model_path.endswith(".pt"):
            tts_model_path = os.path.join(MODELS_DIR, f"ToucanTTS_{tts_model_path}", "best.pt")
        if vocoder_model_path is None:
            vocoder_model_path = os.path.join(MODELS_DIR, "Avocodo" if faster_vocoder else "BigVGAN", "best.pt")

        self.text2phone = ArticulatoryCombinedTextFrontend(language=language, add_silence_to_end=True)

        checkpoint = _load_checkpoint(tts_model_path)
        sd = _to_numpy_sd(checkpoint["model"])
        # variant detection: the reference retries load_state_dict (:55-63); the schema tells us directly
        self.use_lang_id = "encoder.language_embedding.weight" in sd
        # precision of the MFMA GEMMs: fp32 (exact-parity default), TOUCAN_PRECISION=bf16 / f16 (BASELINE.json configs[2] / [4]),
        # f32x3 (fp32 tensors, dense products as three fp16 MFMAs on split operands: keeps the fp32 tolerances), or mixed / mixed3:
        # acoustic model in fp32 / f32x3 (the mel keeps the fp32 parity), vocoder on the fp16 matrix cores
        precision = os.environ.get("TOUCAN_PRECISION", "f32")
        voc_precision = "f16" if precision in ("mixed", "mixed3") else precision
        precision = {"mixed": "f32", "mixed3": "f32x3"}.get(precision, precision)
        voc = _load_checkpoint(vocoder_model_path)
        voc_sd, kind = _to_numpy_sd(voc["generator"]), "hifigan" if faster_vocoder else "bigvgan"
        # On a GPU the whole pass runs through the stage API (native.NativePipeline -> csrc/pipeline.hip: the kernels are sequenced in
        # C++, a dozen C calls per batch).  TOUCAN_PY_SEQUENCER=1 - and the CPU test emulator - keep engine.py's Python sequencing.
        import ctypes
        from . import capi
        self.pipe = None
        if torch.device(device).type == "cuda" and isinstance(capi.lib(), ctypes.CDLL) and not os.environ.get("TOUCAN_PY_SEQUENCER"):
            from . import native
            self.pipe = native.NativePipeline(sd, voc_sd, kind, device, precision=precision, vocoder_precision=voc_precision)
            self.phone2mel = self.mel2wav = self.pipe  # (the reference's attribute names; both stages live in the one handle)
        else:
            self.phone2mel = engine.AcousticEngine(sd, device, precision=precision)
            self.mel2wav = engine.VocoderEngine(voc_sd, kind, device, precision=voc_precision)

        self.embedding_model_path = embedding_model_path  # GST network: loaded on the first set_utterance_embedding(path)
        self._style = None
        self.last_prosody_stats = None  # (before, after) of the last batch that took per-utterance prosody scales or curves
        self.last_prosody_span_stats = None  # per utterance (before, after) of its Spans, of the last batch that took prosody curves
        self.last_prosody_fit = None  # dict(report, scales, extra) of the last batch that took time budgets (prosody_fit.py)
        self.last_delivery = None  # float64 [B, 8] on the device (truepeak.DELIVERY_COLUMNS) of the last call that took true_peak_ceiling= / limiter=
        self.last_loudness = None  # float64 [B, 8] on the device (loudness.LOUDNESS_COLUMNS) of the last call that took loudness=
        self.last_speech_activity = None  # (stats [B, 8], runs [B, 64, 2], counts [B, 16]) on the device of the last call that took speech_level=


        self.default_utterance_embedding = checkpoint["default_emb"].to(self.device)
        self.lang_id = get_language_id_tensor(language) if self.use_lang_id else None
        self.eval()

    # ---- setters (:103-130) -------------------------------------------------------------------------
    _warned_trim = False

    def set_utterance_embedding(self, path_to_reference_audio="", embedding=None, trim_silence=False):
        """``trim_silence`` (additive; the reference's ``cut_silence=True`` uses silero, which is not reproduced): cut the normalised
        16 kHz wave to the bounds of the speech that the ITU-T P.56 activity meter finds (activity.py, 30 ms lead) before the
        log-mel.  If it finds none, or fewer than 513 samples are left, the wave stays uncut, with one warning."""
        if embedding is not None:
            self.default_utterance_embedding = embedding.squeeze().to(self.device)
            return
        assert os.path.exists(path_to_reference_audio)
        # reference audio -> mono, peak-normalised, 16 kHz -> log-mel -> GST style embedding, the last two on the GPU (style.py).
        # Deviation (network-only dependency): the reference also trims leading / trailing silence with the silero VAD.
        from . import style
        if self._style is None:
            path = self.embedding_model_path or os.path.join(MODELS_DIR, "Embedding", "embedding_function.pt")  # :71-77
            self._style = (style.LogMel(self.device), style.StyleEngine(_to_numpy_sd(_load_checkpoint(path)["style_emb_func"]), self.device))
        data, sr = style.read_audio(path_to_reference_audio)
        logmel, gst = self._style
        wave16 = style.normalize_reference_audio(data, sr)
        if trim_silence:
            from . import activity
            packed = torch.from_numpy(np.asarray(wave16, dtype=np.float32).reshape(-1)).to(self.device)
            found = activity.bounds(self._activity().measure(packed, [(0, packed.numel())], style.SR), lead=style.SR * activity.DEFAULT_LEAD_MS // 1000)[0]
            if found is not None and found[1] - found[0] >= 513:
                wave16 = wave16[found[0]:found[1]]
            elif not ToucanTTSInterface._warned_trim:
                ToucanTTSInterface._warned_trim = True
                warnings.warn("trim_silence=True: no speech of at least 513 samples was found in the reference audio; it is used uncut")
        spec = logmel.forward(wave16)
        self.default_utterance_embedding = gst.forward([spec])[0].to(self.device)

    def set_language(self, lang_id):
        self.set_phonemizer_language(lang_id=lang_id)
        self.set_accent_language(lang_id=lang_id)

    def set_phonemizer_language(self, lang_id):
        self.text2phone = ArticulatoryCombinedTextFrontend(language=lang_id, add_silence_to_end=True)

    def set_accent_language(self, lang_id):
        self.lang_id = get_language_id_tensor(lang_id).to(self.device) if self.use_lang_id else None

    # ---- synthesis -----------------------------------------------------------------------------------
    def _lang(self):
        return None if self.lang_id is None else int(self.lang_id.reshape(-1)[0])

    def forward(self,
                text,
                view=False,
                duration_scaling_factor=1.0,
                pitch_variance_scale=1.0,
                energy_variance_scale=1.0,
                pause_duration_scaling_factor=1.0,
                durations=None,
                pitch=None,
                energy=None,
                input_is_phones=False,
                return_plot_as_filepath=False,
                z_noise=None,
                sample_rate=None,
                pcm16=False,
                prosody_curves=None,
                loudness=None,
                peak_ceiling=-1.0,
                speech_level=None,
                true_peak_ceiling=None,
                limiter=False,
                prosody_fit=None):
        """The reference's signature (ToucanTTSInterface.py:132-143) plus additive keywords.  ``z_noise`` [80, T]: the PostFlow
        noise 0.8 N(0,1) the reference draws inside the model (Glow.py:363), so that a call can be reproduced and checked
        against the oracle; None draws it on the device.  ``sample_rate`` / ``pcm16``: the waveform at another rate than 24 kHz
        and / or as int16, converted on the device (resample.py); the figure of ``view`` keeps drawing the 24 kHz wave.
        ``prosody_curves``: this utterance's per-phoneme curves, an [L, 5] array or a list of ``prosody.Span`` (as one entry of
        ``synthesize_batch``'s keyword, documented there); None is the call as it was.  ``prosody_fit``: a ``prosody_fit.Fit`` (this
        utterance in a given number of frames or seconds) or a list of span ``Fit``s, as one entry of ``synthesize_batch``'s keyword;
        None is the call as it was.  ``loudness`` / ``peak_ceiling``: as in
        ``synthesize_batch``; the figure of ``view`` then draws the normalised 24 kHz wave.  ``speech_level``, ``true_peak_ceiling`` / ``limiter``: as in
        ``synthesize_batch``."""
        self._check_output_format(sample_rate, pcm16)
        self._check_loudness(loudness, peak_ceiling)
        self._check_speech_level(loudness, speech_level, peak_ceiling)
        self._check_delivery(loudness, speech_level, true_peak_ceiling, limiter)
        with torch.inference_mode():
            phones = self.text2phone.string_to_tensor(text, input_phonemes=input_is_phones)
            curves = {} if prosody_curves is None else dict(prosody_curves=[prosody_curves])
            if prosody_fit is not None:
                prosody_fit_mod.resolve_fits([int(phones.shape[0])], [prosody_fit])  # (ValueError before anything runs)
                curves["prosody_fit"] = [prosody_fit]
            wav24, spans = self._synthesize_packed([phones], [self.default_utterance_embedding], [self._lang()],
                                                   z_noise=None if z_noise is None else [z_noise],
                                                   durations=None if durations is None else [durations],
                                                   pitch=None if pitch is None else [pitch],
                                                   energy=None if energy is None else [energy],
                                                   duration_scaling_factor=duration_scaling_factor, pitch_variance_scale=pitch_variance_scale,
                                                   energy_variance_scale=energy_variance_scale,
                                                   pause_duration_scaling_factor=pause_duration_scaling_factor, **curves)
            wav24 = self._normalize(wav24, spans, loudness, peak_ceiling, speech_level, true_peak_ceiling, limiter)
            wav, out_spans = self._convert(wav24, spans, sample_rate, pcm16)
            wavs = [wav[b:b + n] for b, n in out_spans]
        if view or return_plot_as_filepath:  # ToucanTTSInterface.py:171-226 (matplotlib only: plotting.py)
            from . import plotting
            if input_is_phones:
                labels = text.replace(" ", "|")
            else:
                labels = self.text2phone.get_phone_string(text, for_plot_labels=True)
            b24, n24 = spans[0]
            fig = plotting.draw(wav24[b24:b24 + n24].cpu().numpy(), self.last_mel[0].cpu().numpy(), self.last_durations[0].cpu().numpy(),
                                self.last_pitch[0].cpu().numpy(), labels, text)
            if return_plot_as_filepath:
                return wavs[0], plotting.show_or_save(fig, "tmp.png")
            plotting.show_or_save(fig)
        return wavs[0]

    def _synthesize_packed(self, phones, embs, langs, z_noise=None, **kw):
        """One ragged batch through both engines.  Returns (packed waveform, [(first sample, sample count)] per utterance)."""
        emb = torch.stack([e.reshape(-1).to(torch.float32).cpu() for e in embs])
        lang_ids = None if any(l is None for l in langs) else langs
        if self.pipe is not None:
            out = self.pipe.forward(phones, emb, lang_ids, z_noise=z_noise, **kw)
            self.last_durations, self.last_pitch, self.last_energy = out["durations"], out["pitch"], out["energy"]
            self.last_mel = out["mel"]
            self.last_prosody_stats = out.get("prosody_stats")
            self.last_prosody_span_stats = out.get("prosody_span_stats")
            self.last_prosody_fit = out.get("prosody_fit")
            return out["wav"], out["wav_spans"]
        out = self.phone2mel.forward(phones, emb, lang_ids, z_noise=z_noise, **kw)
        wav, rag = self.mel2wav.forward(out["mel_packed"], out["rag_mel"])
        self.last_durations, self.last_pitch, self.last_energy = out["durations"], out["pitch"], out["energy"]
        self.last_mel = out["mel"]
        self.last_prosody_stats = out.get("prosody_stats")
        self.last_prosody_span_stats = out.get("prosody_span_stats")
        self.last_prosody_fit = out.get("prosody_fit")
        return wav, list(zip(rag.begins, rag.lengths))

    def _synthesize(self, phones, embs, langs, z_noise=None, sample_rate=None, pcm16=False, loudness=None, peak_ceiling=-1.0, speech_level=None,
                    true_peak_ceiling=None, limiter=False, **kw):
        wav, spans = self._synthesize_packed(phones, embs, langs, z_noise=z_noise, **kw)
        wav = self._normalize(wav, spans, loudness, peak_ceiling, speech_level, true_peak_ceiling, limiter)
        wav, spans = self._convert(wav, spans, sample_rate, pcm16)
        return [wav[b:b + n] for b, n in spans]

    SAMPLE_RATE = 24000  # what both vocoders generate

    @staticmethod
    def _check_output_format(sample_rate, pcm16):
        """ValueError for a rate the resampler cannot serve; True if the 24 kHz float32 waveform has to be converted at all."""
        if sample_rate is None or sample_rate == ToucanTTSInterface.SAMPLE_RATE:
            return bool(pcm16)
        from . import resample
        resample.ratio(ToucanTTSInterface.SAMPLE_RATE, sample_rate)
        return True

    def _resampler(self):
        if getattr(self, "_resampler_obj", None) is None:
            from . import resample
            self._resampler_obj = resample.Resampler(self.device)
        return self._resampler_obj

    def _convert(self, wav, spans, sample_rate, pcm16):
        """The packed 24 kHz waveform and its spans at ``sample_rate`` (None: 24 kHz), as int16 with ``pcm16``, every utterance
        converted on its own on the device, behind the vocoder on its stream.  24 kHz float32 is returned as it came."""
        if not self._check_output_format(sample_rate, pcm16):
            return wav, spans
        return self._resampler().resample(wav.contiguous(), spans, self.SAMPLE_RATE, sample_rate or self.SAMPLE_RATE, pcm16)

    @staticmethod
    def _check_loudness(loudness, peak_ceiling):
        """ValueError for a target or a ceiling that is not finite, or a ceiling above 0 dBFS; True if the waveform is to be
        normalised at all (``loudness`` is not None)."""
        if loudness is None:
            return False
        from . import loudness as ld
        ld.check_target(loudness, peak_ceiling)
        return True

    def _meter(self):
        if getattr(self, "_meter_obj", None) is None:
            from . import loudness as ld
            self._meter_obj = ld.LoudnessMeter(self.device)
        return self._meter_obj

    @staticmethod
    def _check_speech_level(loudness, speech_level, peak_ceiling):
        """ValueError for ``loudness`` and ``speech_level`` together, for a target or a ceiling that is not finite, or a ceiling
        above 0 dBFS; True if the waveform is to be brought to an active speech level at all (``speech_level`` is not None)."""
        if speech_level is None:
            return False
        if loudness is not None:
            raise ValueError("loudness and speech_level are two normalisations of the same waveform: give one of them")
        from . import activity as ac
        ac.check_target(speech_level, peak_ceiling)
        return True

    @staticmethod
    def _check_delivery(loudness, speech_level, true_peak_ceiling, limiter):
        """ValueError for ``true_peak_ceiling`` or ``limiter`` without ``loudness`` or together with ``speech_level``, for a ceiling
        that is not finite or above 0 dBTP; True if the normalisation is to hold a true-peak ceiling at all."""
        if true_peak_ceiling is None and not limiter:
            return False
        if speech_level is not None:
            raise ValueError("true_peak_ceiling and limiter belong to the loudness normalisation: they do not combine with speech_level")
        if loudness is None:
            raise ValueError("true_peak_ceiling and limiter belong to the loudness normalisation: give loudness= as well")
        from . import truepeak as tp
        if true_peak_ceiling is not None:
            tp.check_ceiling(true_peak_ceiling)
        return True

    def _delivery(self):
        if getattr(self, "_delivery_obj", None) is None:
            from . import truepeak as tp
            self._delivery_obj = tp.DeliveryMeter(self.device, self._meter())
        return self._delivery_obj

    def _activity(self):
        if getattr(self, "_activity_obj", None) is None:
            from . import activity as ac
            self._activity_obj = ac.SpeechActivity(self.device)
        return self._activity_obj

    def _normalize(self, wav, spans, loudness, peak_ceiling, speech_level=None, true_peak_ceiling=None, limiter=False):
        """The packed 24 kHz waveform with every utterance at ``loudness`` LUFS (ITU-R BS.1770 integrated loudness) or at the
        active speech level ``speech_level`` dB (ITU-T P.56), or as close as the sample-peak ceiling ``peak_ceiling`` dBFS allows,
        measured and scaled on the device behind the vocoder on its stream; ``self.last_loudness`` or
        ``self.last_speech_activity`` gets the statistics.  Both None returns the waveform as it came, without a launch.  With
        ``true_peak_ceiling`` (dBTP; None with ``limiter`` alone: -1) the loudness normalisation also holds the true peak under
        that ceiling - by its one gain, or with ``limiter`` by a look-ahead limiter behind the gain to the target (truepeak.py) -
        and ``self.last_delivery`` gets the statistics of the result."""
        delivery = self._check_delivery(loudness, speech_level, true_peak_ceiling, limiter)
        if self._check_speech_level(loudness, speech_level, peak_ceiling):
            meter = self._activity()
            wav, stats = meter.normalize(wav.contiguous(), spans, self.SAMPLE_RATE, speech_level, peak_ceiling)
            self.last_speech_activity = (stats, meter.last_runs, meter.last_counts)
            return wav
        if not self._check_loudness(loudness, peak_ceiling):
            return wav
        if delivery:
            wav, self.last_loudness, self.last_delivery = self._delivery().normalize(
                wav.contiguous(), spans, self.SAMPLE_RATE, loudness, peak_ceiling, -1.0 if true_peak_ceiling is None else true_peak_ceiling, bool(limiter))
            return wav
        wav, self.last_loudness = self._meter().normalize(wav.contiguous(), spans, self.SAMPLE_RATE, loudness, peak_ceiling)
        return wav

    def predict_frame_counts(self, feats, embs, pitch=None, energy=None, **kw):
        """Mel frames each utterance will get (stage A only) - the balancing key of the multi-GPU deal."""
        emb = torch.stack([e.reshape(-1).to(torch.float32).cpu() for e in embs])
        langs = None if self.lang_id is None else [self._lang()] * len(feats)
        return self.phone2mel.predict_frame_counts(feats, emb, langs, pitch=pitch, energy=energy, **kw)

    def synthesize_batch(self, texts, input_is_phones=True, utterance_embeddings=None, z_noise=None, durations=None, pitch=None,
                         energy=None, duration_scaling_factor=1.0, pitch_variance_scale=1.0, energy_variance_scale=1.0,
                         pause_duration_scaling_factor=1.0, distributed=False, sample_rate=None, pcm16=False, prosody_curves=None,
                         loudness=None, peak_ceiling=-1.0, speech_level=None, true_peak_ceiling=None, limiter=False, prosody_fit=None):
        """Additive API: a ragged batch in one pass; each utterance equals the reference run on it alone (16-bit configurations: bit
        for bit whatever the batch; fp32: durations / pitch / energy bit for bit, the mel to fp32 rounding order - DESIGN.md section 4).
        texts: phoneme strings (or [L,62] feature tensors).  durations / pitch / energy: optional per-utterance gold prosody (the
        cloner-style call, UtteranceCloner.py:163).  With ``distributed=True`` and an initialised process group the utterances are
        dealt over the ranks by frame count and every rank returns all waveforms (distributed.py).  ``sample_rate`` / ``pcm16``:
        the waveforms at another rate than 24 kHz and / or as int16, converted on the device (not with ``distributed=True``).
        The four prosody scales: each a scalar for the batch or a sequence with one value per utterance.  Any sequence takes the
        per-utterance kernels - an utterance still equals the call on it alone with its own scalars - and leaves
        ``self.last_prosody_stats`` = (before, after): float32 [B, 8] arrays (columns ``prosody.STATS``) of every utterance's pitch /
        energy / durations before and after its scales; an all-scalar call leaves None there.  ValueError for a sequence of the
        wrong length, a duration factor that is not positive (the message names the utterance), and sequences with
        ``distributed=True`` (the sharded deal does not carry them).
        ``prosody_curves``: None, or a list with one entry per utterance - None, a float [L_u, 5] array with the columns
        ``prosody.CURVE_COLUMNS`` (duration factor, pitch variance scale, energy variance scale, all neutral at 1; pitch offset, energy
        offset, neutral at 0) or a list of ``prosody.Span`` (``prosody.emphasis(feats, [k])`` stresses word k), overlapping Spans
        multiplying their factors and adding their offsets.  Every phoneme's effective scale is the utterance's scale times its
        curve value: a variance scale moves the phoneme away from (above 1) or towards (below 1) the mean of
        the WHOLE utterance's non-zero entries, an offset is added to non-zero entries afterwards, both clamp at 0, and a phoneme
        whose five values are neutral keeps the bits of the call without curves.  The reference's quirk is kept: a zero entry (an
        unvoiced phoneme, a pause) inside a Span scaled below 1 becomes mean * (1 - scale).  A call with curves leaves
        ``self.last_prosody_stats`` as above and ``self.last_prosody_span_stats``: per utterance (before [n, 8], after [n, 8]) for its
        Spans in list order (empty for arrays); column 6 of a Span's block is the frames it occupies after the curves, which with the
        frames in front of it (``self.last_durations``) tells which samples carry the emphasised word.  ValueError for a wrong
        shape, a Span outside its utterance, a value that is not finite or a duration factor that is not positive (the message
        names the utterance and the phoneme), and for curves with ``distributed=True``.
        ``prosody_fit``: None (the call as it was: the same entry, the same bits), or a list with one entry per utterance - None, a
        ``prosody_fit.Fit`` or a list of span ``Fit``s.  ``Fit(target_frames=N)`` / ``Fit(target_seconds=3.2)`` gives the utterance
        exactly that many mel frames (384 samples each) by solving for its duration scale on the device, between the predictors and
        the control kernel of the same pass; ``knob="pause"`` keeps the speech tempo and lets the pauses absorb the slot;
        ``Fit(..., start=a, stop=b)`` fits phonemes [a, b) alone.  Where no scale reaches the target (the frame count is a step
        function of the scale) ``exact=True`` hands the missing frames to the phonemes next in line, evenly spread; ``exact=False``
        takes the nearest scale.  It composes with the scales, ``prosody_curves`` and gold ``durations``: the fit varies its one
        knob, everything else stays as given.  ``self.last_prosody_fit`` = dict(report: per utterance [n_u, 8] with the columns
        ``prosody_fit.FIT_COLUMNS`` (status: ``prosody_fit.STATUS``; a target outside the knob's bounds is reported CLAMPED, not
        raised), scales: the solved [B, 4] table, extra: per utterance the frames handed out); ``self.last_prosody_stats`` is
        filled as above.  ValueError (the message names the utterance and the segment) for both or neither target, a target that is
        no whole number of frames in 1 .. 2^24, bad bounds, a span outside its utterance, overlapping spans, a whole-utterance Fit
        beside spans, and with ``distributed=True``.
        ``loudness``: None (the call as it was: no launch, the same bits) or a target in LUFS, e.g. -23 (EBU R 128).  Every
        utterance's integrated loudness after ITU-R BS.1770-4 (K-weighting, 400 ms blocks, absolute gate at -70 LUFS, relative gate
        at -10 LU) is measured at 24 kHz on the device and the utterance scaled by one gain to the target, before the conversion of
        ``sample_rate`` / ``pcm16``; ``peak_ceiling`` (dBFS, at most 0) limits the gain so that no SAMPLE exceeds it - a sample peak,
        not an oversampled true peak (``true_peak_ceiling`` below adds that).  An utterance without a loudness (shorter than 400 ms, or silent) keeps its bits.
        ``self.last_loudness``: float64 [B, 8] on the device, columns ``loudness.LOUDNESS_COLUMNS`` (the loudness found, the peak,
        the blocks and what each gate kept, the loudest block, the gain applied, the loudness reached).  ValueError for a target or
        ceiling that is not finite, a ceiling above 0, and with ``distributed=True``.
        ``speech_level``: None (the call as it was) or a target active speech level in dB re full scale, e.g. -26 (the convention
        of listening tests).  Every utterance's active speech level after ITU-T P.56 method B (activity.py, DESIGN.md section 18;
        agreement with the ITU's sv56 is unpinned) is measured at 24 kHz on the device and the utterance scaled to the target, in
        the same place and under the same ``peak_ceiling`` as ``loudness``; an utterance without a level keeps its bits.
        ``self.last_speech_activity`` = (stats float64 [B, 8], columns ``activity.ACTIVITY_COLUMNS``: both levels, the activity
        factor, the threshold, the bounds of the speech in samples, the gain, the level reached; runs int64 [B, 64, 2]: the runs of
        speech, ``activity.pauses`` gives the pauses between them; counts int64 [B, 16]: the active samples per threshold and the
        number of runs), all on the device.  ValueError together with ``loudness`` and wherever ``loudness`` raises one.
        ``true_peak_ceiling`` / ``limiter`` (with ``loudness``; None and False are the call as it was: the same launches, the same
        bits): a ceiling in dBTP, at most 0, for the TRUE peak after ITU-R BS.1770-4 Annex 2 - the 24 kHz utterance oversampled 4x
        on the device (truepeak.py) - which the one gain then respects as well as ``peak_ceiling``: the
        meter's own reading of the result is at or under it.  A peaky utterance then ends below the target; ``limiter=True``
        instead applies the gain to the target and runs a look-ahead limiter (2 ms, feed-forward) that holds samples and true
        peak under the lower of the two ceilings (``true_peak_ceiling=None`` then means -1).  ``self.last_delivery``: float64
        [B, 8] on the device, columns ``truepeak.DELIVERY_COLUMNS`` (true peak, the same in dBTP, sample peak, largest short-term
        loudness, loudness range with its two percentiles, short-term blocks kept) of the waveforms as returned at 24 kHz;
        ``self.last_loudness`` holds the gain and the loudness reached (measured again behind the limiter).  ValueError without
        ``loudness``, together with ``speech_level``, for a ceiling that is not finite or above 0, and with ``distributed=True``."""
        if distributed and (true_peak_ceiling is not None or limiter):
            raise ValueError("true_peak_ceiling / limiter are not available with distributed=True: the sharded exchange carries the waveforms as synthesised")
        if distributed and loudness is not None:
            raise ValueError("loudness is not available with distributed=True: the sharded exchange carries the waveforms as synthesised")
        if distributed and speech_level is not None:
            raise ValueError("speech_level is not available with distributed=True: the sharded exchange carries the waveforms as synthesised")
        self._check_loudness(loudness, peak_ceiling)
        self._check_speech_level(loudness, speech_level, peak_ceiling)
        self._check_delivery(loudness, speech_level, true_peak_ceiling, limiter)
        if distributed and (sample_rate is not None or pcm16):
            raise ValueError("sample_rate / pcm16 are not available with distributed=True: the sharded exchange carries 24 kHz float32")
        self._check_output_format(sample_rate, pcm16)
        per_utterance = prosody.resolve_scales(len(texts), duration_scaling_factor, pitch_variance_scale, energy_variance_scale,
                                               pause_duration_scaling_factor) is not None
        if distributed and per_utterance:
            raise ValueError("per-utterance prosody scales are not available with distributed=True: the sharded deal carries scalars")
        if distributed and prosody_curves is not None:
            raise ValueError("prosody curves are not available with distributed=True: the sharded deal carries scalars")
        if distributed and prosody_fit is not None:
            raise ValueError("prosody_fit is not available with distributed=True: the sharded deal carries scalars")
        feats = [t if torch.is_tensor(t) else self.text2phone.string_to_tensor(t, input_phonemes=input_is_phones) for t in texts]
        embs = utterance_embeddings if utterance_embeddings is not None else [self.default_utterance_embedding] * len(feats)
        kw = dict(duration_scaling_factor=duration_scaling_factor, pitch_variance_scale=pitch_variance_scale,
                  energy_variance_scale=energy_variance_scale, pause_duration_scaling_factor=pause_duration_scaling_factor)
        if not distributed:
            if prosody_curves is not None:
                prosody.resolve_curves([int(f.shape[0]) for f in feats], prosody_curves)  # (ValueError before anything runs)
                kw["prosody_curves"] = prosody_curves
            if prosody_fit is not None:
                prosody_fit_mod.resolve_fits([int(f.shape[0]) for f in feats], prosody_fit)  # (ValueError before anything runs)
                kw["prosody_fit"] = prosody_fit
            with torch.inference_mode():
                return self._synthesize(feats, embs, [self._lang()] * len(feats), z_noise=z_noise, durations=durations, pitch=pitch,
                                        energy=energy, sample_rate=sample_rate, pcm16=pcm16, loudness=loudness, peak_ceiling=peak_ceiling,
                                        speech_level=speech_level, true_peak_ceiling=true_peak_ceiling, limiter=limiter, **kw)
        from . import distributed as dd
        return dd.synthesize_sharded(self, feats, embs, z_noise, durations, pitch, energy, kw)

    def _comparator(self):
        if getattr(self, "_comparator_obj", None) is None:
            from . import compare
            self._comparator_obj = compare.SpeechComparator(self.device)
        return self._comparator_obj

    def evaluate_against_recordings(self, texts, recordings, input_is_phones=True, keep_waves=False, f0="track", **synthesis_keywords):
        """Additive API: synthesise ``texts`` as one batch (``synthesize_batch`` with ``synthesis_keywords``: prosody scales, curves,
        gold prosody, ``z_noise``, ``utterance_embeddings``) and measure how close each waveform is to a recording of the same
        sentence (compare.SpeechComparator.compare): mel-cepstral distortion along the warping path, F0 RMSE in
        Hz and cents, log-F0 correlation, GPE, VDE and FFE, the recording being the reference side.  recordings: per text a path
        (style.read_audio) or a (wave, sample rate) tuple; several channels are averaged.  f0: as ``compare`` takes it.  -> one dict
        per text; with ``keep_waves`` it also holds "synth" (float32, 24 kHz), "recording" (mono, float32) and "recording_sr", the two
        waves that were compared.  ValueError for lists of unequal length, for ``distributed=True`` and for ``sample_rate`` /
        ``pcm16`` (the comparison takes the 24 kHz float waveform), for ``loudness`` and ``speech_level`` (both waves are divided by their peaks anyway), and
        what ``compare`` refuses."""
        if synthesis_keywords.get("distributed"):
            raise ValueError("evaluate_against_recordings is not available with distributed=True: the comparison runs on one device")
        if synthesis_keywords.get("sample_rate") is not None or synthesis_keywords.get("pcm16"):
            raise ValueError("evaluate_against_recordings compares the 24 kHz float waveform: sample_rate / pcm16 do not apply")
        if synthesis_keywords.get("loudness") is not None:
            raise ValueError("evaluate_against_recordings divides both waves by their peaks before it compares them: loudness does not apply")
        if synthesis_keywords.get("speech_level") is not None:
            raise ValueError("evaluate_against_recordings divides both waves by their peaks before it compares them: speech_level does not apply")
        if len(texts) != len(recordings):
            raise ValueError(f"{len(texts)} texts for {len(recordings)} recordings")
        from . import style
        recs, srs = [], []
        for r in recordings:
            data, sr = style.read_audio(r) if isinstance(r, (str, os.PathLike)) else r
            data = np.asarray(data, dtype=np.float32)
            recs.append(data.mean(axis=1) if data.ndim == 2 else data.reshape(-1))
            srs.append(int(sr))
        synth = [w.float().cpu().numpy() for w in self.synthesize_batch(texts, input_is_phones=input_is_phones, **synthesis_keywords)]
        results = self._comparator().compare(synth, recs, self.SAMPLE_RATE, srs, f0=f0)
        if keep_waves:
            for r, s, w, sr in zip(results, synth, recs, srs):
                r.update(synth=s, recording=w, recording_sr=sr)
        return results

    def vocoder_fidelity(self, recordings, sr=None, keep_waves=False, intelligibility=False):
        """Additive API: copy-synthesis of ``recordings`` through this interface's own vocoder, at the precision it runs at
        (fidelity.CopySynthesis): every recording goes to 24 kHz and is cut to whole mel frames, its 16 kHz /
        80-bin log-mel - what the acoustic model would hand the vocoder - is vocoded, and the result is compared with the cut
        recording: ``mel_l1`` (the reference's vocoder training loss without its weight), the frame it is worst at, and per STFT
        resolution the spectral convergence and the log-magnitude L1.  recordings: paths (style.read_audio), (wave, sample rate)
        tuples, or waveforms at ``sr``; several channels are averaged.  -> one dict per recording
        (``fidelity.SpectralDistance.distance`` documents it); with ``keep_waves`` it also holds "generated" and "recording", the
        two 24 kHz signals that were compared, on the device; with ``intelligibility`` also ``stoi``, ``estoi`` and
        ``intelligibility_status`` of the same two signals (intelligibility.py, DESIGN.md section 23: what the precision or the
        faster vocoder costs in intelligibility).  Everything from the first resampling on stays on the device."""
        from . import fidelity, style
        if getattr(self, "_fidelity_obj", None) is None:
            vocode = self.mel2wav.vocode if self.pipe is not None else self.mel2wav.forward
            self._fidelity_obj = fidelity.CopySynthesis(vocode, self.device)
        waves, rates = [], []
        for r in recordings:
            if isinstance(r, (str, os.PathLike)):
                data, rate = style.read_audio(r)
            elif isinstance(r, tuple):
                data, rate = r
            else:
                if sr is None:
                    raise ValueError("waveforms need their sample rate: vocoder_fidelity(waves, sr=...)")
                data, rate = r, sr
            waves.append(data)
            rates.append(int(rate))
        results = [None] * len(waves)
        for rate in sorted(set(rates)):  # one batch holds one rate
            idx = [i for i, x in enumerate(rates) if x == rate]
            for i, rec in zip(idx, self._fidelity_obj.run([waves[i] for i in idx], rate, keep_waves=keep_waves, intelligibility=intelligibility)):
                results[i] = rec
        return results

    def _checker(self):
        """The pronunciation checker, built on first use from the aligner checkpoint the cloner loads (Models/Aligner/aligner.pt)."""
        if getattr(self, "_checker_obj", None) is None:
            from . import pronunciation
            path = os.path.join(MODELS_DIR, "Aligner", "aligner.pt")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path}: aligner checkpoint not found (offline, write the fixture one with "
                                        f"ims_toucan_prosody_variance_amd.interface.write_fixture_aligner_checkpoint)")
            sd = torch.load(path, map_location="cpu", weights_only=True)["asr_model"]
            self._checker_obj = pronunciation.PronunciationChecker(sd, self.device)
        return self._checker_obj

    def check_pronunciation(self, texts, input_is_phones=True, beam=8, ignore_ids=(), keep_waves=False, **synthesis_keywords):
        """Additive API: synthesise ``texts`` as one batch (``synthesize_batch`` with ``synthesis_keywords``: prosody scales, curves,
        gold prosody, ``z_noise``, ``utterance_embeddings``) and ask the aligner whether each waveform still says its text, without
        any recording (pronunciation.PronunciationChecker.check): the phoneme error rate of the decoded
        phonemes (``beam``: the width of the CTC prefix beam search, 0 for the greedy best path) with the substituted, deleted and
        inserted phonemes, the CTC loss, and per phoneme of the text its frames in the forced alignment, mean log-posterior,
        goodness of pronunciation and frame accuracy.  ``ignore_ids``: aligner ids left out of both the text and the decode
        (silences, punctuation).  -> one dict per text (``check_logits`` documents it); with ``keep_waves`` it also holds "synth"
        (float32, 24 kHz).  The numbers are the aligner's opinion, meant for comparing settings of one sentence against each
        other, not an absolute intelligibility score.  ValueError for ``distributed=True``, for ``sample_rate`` / ``pcm16`` (the
        check takes the 24 kHz float waveform), for ``loudness`` and ``speech_level`` (the wave is divided by its peak anyway),
        and what ``check`` refuses."""
        if synthesis_keywords.get("distributed"):
            raise ValueError("check_pronunciation is not available with distributed=True: the check runs on one device")
        if synthesis_keywords.get("sample_rate") is not None or synthesis_keywords.get("pcm16"):
            raise ValueError("check_pronunciation checks the 24 kHz float waveform: sample_rate / pcm16 do not apply")
        if synthesis_keywords.get("loudness") is not None:
            raise ValueError("check_pronunciation divides the wave by its peak before it checks it: loudness does not apply")
        if synthesis_keywords.get("speech_level") is not None:
            raise ValueError("check_pronunciation divides the wave by its peak before it checks it: speech_level does not apply")
        from . import pronunciation
        pronunciation.check_beam(beam)
        pronunciation.drop_mask(ignore_ids)
        feats = [t if torch.is_tensor(t) else self.text2phone.string_to_tensor(t, input_phonemes=input_is_phones) for t in texts]
        synth = [w.float().cpu().numpy() for w in self.synthesize_batch(feats, input_is_phones=input_is_phones, **synthesis_keywords)]
        results = self._checker().check([f.float().cpu().numpy() for f in feats], synth, self.SAMPLE_RATE, beam=beam, ignore_ids=ignore_ids)
        if keep_waves:
            for r, w in zip(results, synth):
                r["synth"] = w
        return results

    def _prominence(self):
        if getattr(self, "_prominence_obj", None) is None:
            from . import prominence
            self._prominence_obj = prominence.ProminenceMeter(self.device)
        return self._prominence_obj

    def word_prominence(self, texts, input_is_phones=True, weights=(1.0, 1.0, 0.5), band=(1, 3), keep_waves=False, **synthesis_keywords):
        """Additive API: synthesise ``texts`` as one batch (``synthesize_batch`` with ``synthesis_keywords``: prosody scales, curves,
        gold prosody, ``z_noise``, ``utterance_embeddings``) and measure in the AUDIO which words came out prominent and how strong
        the breaks between them are (prominence.ProminenceMeter.measure): the waveform goes through the pitch
        tracker and the frame energy, the phonemes are laid onto its frames by the durations the synthesis used
        (``self.last_durations``), and the wavelet transform of the three tracks is read at every word of
        ``prosody.word_spans``.  -> one dict per text: ``report`` (float64 [words, 8], columns ``prominence.COLUMNS``), ``words``
        (their (start, stop) phonemes) and ``durations`` (frames per phoneme); with ``keep_waves`` also "synth" (float32, 24 kHz).
        ``prominence.to_emphasis(feats, report)`` turns a report into Spans for ``prosody_curves=``.  The numbers compare settings of
        one sentence, or a recording with its clone; they are of this definition alone (parity with the authors' toolkit is
        unpinned).  ValueError for ``distributed=True``, for ``sample_rate`` / ``pcm16`` (the meter takes the 24 kHz float
        waveform), for ``loudness`` and ``speech_level`` (the wave is divided by its peak anyway), a weight that is negative or not
        finite, a band outside 0 .. 5, and what ``measure`` refuses."""
        if synthesis_keywords.get("distributed"):
            raise ValueError("word_prominence is not available with distributed=True: the meter runs on one device")
        if synthesis_keywords.get("sample_rate") is not None or synthesis_keywords.get("pcm16"):
            raise ValueError("word_prominence measures the 24 kHz float waveform: sample_rate / pcm16 do not apply")
        if synthesis_keywords.get("loudness") is not None:
            raise ValueError("word_prominence divides the wave by its peak before it measures it: loudness does not apply")
        if synthesis_keywords.get("speech_level") is not None:
            raise ValueError("word_prominence divides the wave by its peak before it measures it: speech_level does not apply")
        from . import prominence
        prominence.check_weights(weights)
        prominence.check_band(band)
        feats = [t if torch.is_tensor(t) else self.text2phone.string_to_tensor(t, input_phonemes=input_is_phones) for t in texts]
        synth = [w.float().cpu().numpy() for w in self.synthesize_batch(feats, input_is_phones=input_is_phones, **synthesis_keywords)]
        durations = [d.cpu().numpy() for d in self.last_durations]
        host = [f.float().cpu().numpy() for f in feats]
        reports = self._prominence().measure(synth, self.SAMPLE_RATE, host, durations=durations, weights=weights, band=band)
        results = [{"report": r, "words": prosody.word_spans(f), "durations": d} for r, f, d in zip(reports, host, durations)]
        if keep_waves:
            for r, w in zip(results, synth):
                r["synth"] = w
        return results

    def synthesize_ensemble(self, text, utterance_embeddings, durations=None, pitch=None, energy=None, input_is_phones=True, z_noise=None,
                            sample_rate=None, pcm16=False, loudness=None, peak_ceiling=-1.0, speech_level=None, true_peak_ceiling=None,
                            limiter=False):
        """Several voices speaking one text with the same prosody, averaged (UtteranceCloner.py:166-194's ensemble) - as ONE batch
        over the voices instead of a loop that swaps the default embedding.  Without gold durations the voices may predict
        different lengths; the mean is then taken over the common prefix.  ``sample_rate`` / ``pcm16`` convert the 24 kHz mean;
        ``loudness`` / ``peak_ceiling`` (with ``true_peak_ceiling`` / ``limiter``) or ``speech_level`` (as in ``synthesize_batch``)
        normalise the mean, before that conversion."""
        convert = self._check_output_format(sample_rate, pcm16)
        self._check_loudness(loudness, peak_ceiling)
        self._check_speech_level(loudness, speech_level, peak_ceiling)
        self._check_delivery(loudness, speech_level, true_peak_ceiling, limiter)
        n = len(utterance_embeddings)
        rep = lambda v: None if v is None else [v] * n
        waves = self.synthesize_batch([text] * n, input_is_phones=input_is_phones, utterance_embeddings=list(utterance_embeddings),
                                      durations=rep(durations), pitch=rep(pitch), energy=rep(energy), z_noise=z_noise)
        m = min(w.numel() for w in waves)
        mean = torch.stack([w[:m] for w in waves]).mean(dim=0)
        with torch.inference_mode():
            mean = self._normalize(mean, [(0, m)], loudness, peak_ceiling, speech_level, true_peak_ceiling, limiter)
        if not convert:
            return mean
        wav, spans = self._convert(mean, [(0, m)], sample_rate, pcm16)
        return wav[spans[0][0]:spans[0][0] + spans[0][1]]

    def synthesize_grid(self, text, duration_scaling_factors=(1.0,), pitch_variance_scales=(1.0,), energy_variance_scales=(1.0,),
                        pause_duration_scaling_factors=(1.0,), input_is_phones=True, utterance_embedding=None, durations=None, pitch=None,
                        energy=None, z_noise=None, sample_rate=None, pcm16=False, curves=None, loudness=None, peak_ceiling=-1.0,
                        speech_level=None, check_pronunciation=False, beam=8, true_peak_ceiling=None, limiter=False, word_prominence=False):
        """Additive API: ONE text (a phoneme string, or its [L, 62] feature tensor) at every combination of the four tuples of prosody scales - the Cartesian product in row-major
        order of the tuples as listed (the pause factor varies fastest) - synthesised as ragged batches of at most MAX_FILE_BATCH
        variants with per-utterance scales instead of one pass per setting.  Returns one dict per variant, in that order:
        ``scales`` (duration, pitch, energy, pause), ``wave``, ``frames`` (mel frames of the wave), ``stats_before`` /
        ``stats_after`` (float32 [8], columns ``prosody.STATS``: the variant's pitch / energy / durations after the linguistic
        overrides, before and after its scales - their ratio is what a scale really did, the reference's clamp at 0 and its shift of
        the zeros included).  Every variant equals ``forward`` of the text with its four scalars.  durations / pitch / energy: gold
        prosody of the text, shared by the variants; ``z_noise``: None or one [80, T] entry per variant; ``sample_rate`` / ``pcm16`` as
        in ``forward``.  The variants are replicated on the host: every one runs the whole model.
        ``curves``: None, or a list of K alternative per-phoneme curves of the text (each None, an [L, 5] array or a list of
        ``prosody.Span``, as one entry of ``synthesize_batch``'s ``prosody_curves``).  They form a fifth, SLOWEST axis of the product:
        all scale variants under curves[0], then under curves[1], ...  The dicts then also hold ``curve`` (the index into
        ``curves``) and ``span_stats`` = (before [n, 8], after [n, 8]) of that alternative's Spans; column 6 of a Span's block is the
        frames it occupies.  ``curves=[prosody.emphasis(feats, [k]) for k in range(len(prosody.word_spans(feats)))]`` is the emphasis
        sweep over the words of a sentence in one call.
        ``loudness`` / ``peak_ceiling`` (as in ``synthesize_batch``): every variant is normalised on its own and its dict gains
        ``loudness``, its float64 [8] row of statistics on the device; ``self.last_loudness`` holds all rows, in variant order.
        ``true_peak_ceiling`` / ``limiter`` (as in ``synthesize_batch``): every dict also gains ``delivery``, its float64 [8] row of
        ``truepeak.DELIVERY_COLUMNS``, and ``self.last_delivery`` holds all rows, in variant order.
        ``speech_level`` (as in ``synthesize_batch``) likewise: every dict gains ``speech_activity`` = (its stats row [8], its runs
        [64, 2], its counts [16]) - what ``pause_duration_scaling_factor`` really did to the pauses can be read from the runs
        (``activity.pauses``) - and ``self.last_speech_activity`` holds all rows, in variant order.
        ``check_pronunciation`` / ``beam``: every dict gains ``pronunciation``, what ``check_pronunciation`` returns for that variant
        alone (the 24 kHz float waveform as synthesised, before ``loudness`` / ``speech_level`` / ``sample_rate``): phoneme error rate
        and minimum goodness of pronunciation against the scales or the emphasised word - how far a knob goes before the words
        break, in the aligner's opinion.
        ``word_prominence``: every dict gains ``prominence``, the float64 [words, 8] report of ``word_prominence`` for that variant
        alone (the 24 kHz float waveform as synthesised, the durations the variant was synthesised with).  With the emphasis sweep
        as ``curves`` the reports form the matrix "word stressed x word measured": did the stressed word come out stressed, and
        how far can its factors be lowered before it no longer does."""
        self._check_output_format(sample_rate, pcm16)
        if check_pronunciation:
            from . import pronunciation
            pronunciation.check_beam(beam)
        normalise = self._check_loudness(loudness, peak_ceiling)
        level = self._check_speech_level(loudness, speech_level, peak_ceiling)
        delivery = self._check_delivery(loudness, speech_level, true_peak_ceiling, limiter)
        rows, activity_rows, delivery_rows = [], [], []
        variants = prosody.grid(duration_scaling_factors, pitch_variance_scales, energy_variance_scales, pause_duration_scaling_factors)
        which = [None] * len(variants)  # the curve alternative of every variant
        if curves is not None:
            if len(curves) == 0:
                raise ValueError("every axis of a prosody grid needs at least one value")
            which = [k for k in range(len(curves)) for _ in variants]
            variants = variants * len(curves)
        if z_noise is not None and len(z_noise) != len(variants):
            raise ValueError(f"z_noise holds {len(z_noise)} entries, the grid has {len(variants)} variants")
        prosody.resolve_scales(len(variants), *[[v[k] for v in variants] for k in range(4)])  # (the duration factors, before anything runs)
        emb = self.default_utterance_embedding if utterance_embedding is None else utterance_embedding
        results = []
        with torch.inference_mode():
            phones = text if torch.is_tensor(text) else self.text2phone.string_to_tensor(text, input_phonemes=input_is_phones)
            if curves is not None:
                prosody.resolve_curves([int(phones.shape[0])] * len(curves), curves)  # (ValueError before anything runs; "utterance" = alternative)
            for lo in range(0, len(variants), self.MAX_FILE_BATCH):
                chunk = variants[lo:lo + self.MAX_FILE_BATCH]
                n = len(chunk)
                rep = lambda v: None if v is None else [v] * n
                kw = {} if curves is None else dict(prosody_curves=[curves[k] for k in which[lo:lo + n]])
                wav24, spans24 = self._synthesize_packed([phones] * n, [emb] * n, [self._lang()] * n,
                                                         z_noise=None if z_noise is None else list(z_noise[lo:lo + n]),
                                                         durations=rep(durations), pitch=rep(pitch), energy=rep(energy),
                                                         **{name: [v[k] for v in chunk] for k, name in enumerate(prosody.KNOBS)}, **kw)
                before, after = self.last_prosody_stats
                checked = measured = None
                if check_pronunciation or word_prominence:
                    host24 = wav24.float().cpu().numpy()
                if word_prominence:
                    measured = self._prominence().measure([host24[b:b + m] for b, m in spans24], self.SAMPLE_RATE, [phones.float().cpu().numpy()] * n,
                                                          durations=[d.cpu().numpy() for d in self.last_durations])
                if check_pronunciation:
                    checked = self._checker().check([phones.float().cpu().numpy()] * n, [host24[b:b + m] for b, m in spans24], self.SAMPLE_RATE, beam=beam)
                wav24 = self._normalize(wav24, spans24, loudness, peak_ceiling, speech_level, true_peak_ceiling, limiter)
                if normalise:
                    rows.append(self.last_loudness)
                if delivery:
                    delivery_rows.append(self.last_delivery)
                if level:
                    activity_rows.append(self.last_speech_activity)
                wav, spans = self._convert(wav24, spans24, sample_rate, pcm16)
                for i, scales in enumerate(chunk):
                    results.append({"scales": scales, "wave": wav[spans[i][0]:spans[i][0] + spans[i][1]], "frames": int(spans24[i][1]) // 384,
                                    "stats_before": before[i], "stats_after": after[i]})
                    if checked is not None:
                        results[-1]["pronunciation"] = checked[i]
                    if measured is not None:
                        results[-1]["prominence"] = measured[i]
                    if normalise:
                        results[-1]["loudness"] = rows[-1][i]
                    if delivery:
                        results[-1]["delivery"] = delivery_rows[-1][i]
                    if level:
                        results[-1]["speech_activity"] = tuple(t[i] for t in activity_rows[-1])
                    if curves is not None:  # (a chunk whose alternatives are all None took the path without curves: no Spans, no blocks)
                        none = np.zeros((0, len(prosody.STATS)), dtype=np.float32)
                        per = self.last_prosody_span_stats
                        results[-1].update(curve=which[lo + i], span_stats=(none, none) if per is None else per[i])
            if normalise:
                self.last_loudness = torch.cat(rows)
            if delivery:
                self.last_delivery = torch.cat(delivery_rows)
            if level:
                self.last_speech_activity = tuple(torch.cat([r[k] for r in activity_rows]) for k in range(3))
        return results

    def stream(self, text, input_is_phones=False, chunk_frames=512, halo_frames=None, max_batch=4, z_noise=None, sample_rate=None, pcm16=False, loudness=None,
               peak_ceiling=-1.0, speech_level=None, true_peak_ceiling=None, limiter=False, **prosody):
        """Generator of waveform pieces for ONE (long) text: the acoustic model runs once, the vocoder chunk-wise with overlap
        (streaming.py) - the concatenation equals ``self(text, ...)`` bit for bit, the first piece is ready after one chunk and the
        vocoder's workspace is bounded by ``max_batch`` chunks.  prosody: the keyword arguments of ``forward`` (gold durations /
        pitch / energy, scaling factors, ``prosody_curves``).  ``sample_rate`` / ``pcm16``: the pieces at another rate and / or as int16, converted as
        they come (resample.Resampler.streamer); their concatenation equals ``self(text, sample_rate=..., pcm16=...)`` bit for bit.
        ``loudness`` and ``speech_level`` raise ValueError: both are properties of the whole utterance, which a stream does not have;
        so do ``true_peak_ceiling`` and ``limiter``, which belong to ``loudness``."""
        if true_peak_ceiling is not None or limiter:
            raise ValueError("stream() cannot hold a true-peak ceiling: the gain under it needs the whole utterance; use forward(loudness=..., true_peak_ceiling=...)")
        if loudness is not None:
            raise ValueError("stream() cannot normalise loudness: the integrated loudness needs the whole utterance; use forward(loudness=...)")
        if speech_level is not None:
            raise ValueError("stream() cannot normalise the speech level: the active speech level needs the whole utterance; use forward(speech_level=...)")
        if prosody.get("prosody_fit") is not None:
            raise ValueError("stream() does not take prosody_fit; use forward(prosody_fit=...)")
        from . import streaming
        convert = self._check_output_format(sample_rate, pcm16)
        halo = streaming.DEFAULT_HALO if halo_frames is None else halo_frames
        listed = {k: [v] for k, v in prosody.items() if k in ("durations", "pitch", "energy", "prosody_curves") and v is not None}
        scales = {k: v for k, v in prosody.items() if k.endswith("_factor") or k.endswith("_scale")}
        with torch.inference_mode():
            phones = self.text2phone.string_to_tensor(text, input_phonemes=input_is_phones)
            emb = self.default_utterance_embedding.reshape(1, -1).to(torch.float32).cpu()
            langs = None if self.lang_id is None else [self._lang()]
            if self.pipe is not None:
                out = self.pipe.forward([phones], emb, langs, z_noise=None if z_noise is None else [z_noise], vocode=False, **listed, **scales)
                vocode = self.pipe.vocode
            else:
                out = self.phone2mel.forward([phones], emb, langs, z_noise=None if z_noise is None else [z_noise], **listed, **scales)
                vocode = self.mel2wav.forward
            self.last_durations, self.last_pitch, self.last_energy = out["durations"], out["pitch"], out["energy"]
            if "prosody_curves" in listed:
                self.last_prosody_stats, self.last_prosody_span_stats = out.get("prosody_stats"), out.get("prosody_span_stats")
            pieces = streaming.stream_vocode(vocode, out["mel"][0].contiguous(), chunk_frames, halo, max_batch)
            if not convert:
                yield from pieces
                return
            st = self._resampler().streamer(self.SAMPLE_RATE, sample_rate or self.SAMPLE_RATE, pcm16)
            for piece in pieces:
                done = st.push(piece)
                if done.numel():
                    yield done
            done = st.finish()
            if done.numel():
                yield done

    SILENCE_SAMPLES = 10600   # between sentences in read_to_file (ToucanTTSInterface.py:267)
    MAX_FILE_BATCH = 32       # sentences synthesised per ragged batch by read_to_file

    def read_to_file(self,
                     text_list,
                     file_location,
                     duration_scaling_factor=1.0,
                     pitch_variance_scale=1.0,
                     energy_variance_scale=1.0,
                     silent=False,
                     dur_list=None,
                     pitch_list=None,
                     energy_list=None,
                     increased_compatibility_mode=False,
                     input_is_phones=False,
                     sample_rate=None,
                     pcm16=False,
                     loudness=None,
                     peak_ceiling=-1.0,
                     speech_level=None,
                     true_peak_ceiling=None,
                     limiter=False):
        """Same result as the reference's sentence loop (:231-285: silence, sentence, silence, ... with blank strings skipped,
        24 kHz float file or sample-doubled 48 kHz PCM16), but the sentences go through the engines as ragged batches of up to
        MAX_FILE_BATCH utterances and the file is assembled once on the host.  ``sample_rate`` / ``pcm16`` (additive): every
        sentence is converted on the device on its own, the silence is ceil(10600 new / orig) samples and the file has that rate;
        with ``pcm16`` the writer gets the device's int16.  Not with ``increased_compatibility_mode``, which stays the
        reference's doubling.  ``loudness`` / ``peak_ceiling`` (additive, as in ``synthesize_batch``): every sentence is normalised on
        its own (a measurement of the whole file gates the silences out, but not the blocks that straddle the edge of a sentence: it
        reads a little below the sentences);
        ``self.last_loudness`` holds the rows of the spoken sentences in file order.  Not with ``increased_compatibility_mode``.
        ``speech_level`` (additive, as in ``synthesize_batch``) likewise: every sentence on its own, ``self.last_speech_activity``
        holds the rows of the spoken sentences in file order; not with ``increased_compatibility_mode``.
        ``true_peak_ceiling`` / ``limiter`` (additive, as in ``synthesize_batch``): applied with ``loudness`` to every sentence on its
        own; ``self.last_delivery`` holds the rows of the spoken sentences in file order; not with ``increased_compatibility_mode``."""
        if increased_compatibility_mode and (true_peak_ceiling is not None or limiter):
            raise ValueError("increased_compatibility_mode is the reference's path as it is: it does not combine with true_peak_ceiling / limiter")
        if increased_compatibility_mode and loudness is not None:
            raise ValueError("increased_compatibility_mode is the reference's path as it is: it does not combine with loudness")
        if increased_compatibility_mode and speech_level is not None:
            raise ValueError("increased_compatibility_mode is the reference's path as it is: it does not combine with speech_level")
        normalise = self._check_loudness(loudness, peak_ceiling)
        level = self._check_speech_level(loudness, speech_level, peak_ceiling)
        delivery = self._check_delivery(loudness, speech_level, true_peak_ceiling, limiter)
        activity_rows, delivery_rows = {}, {}
        if increased_compatibility_mode and (sample_rate is not None or pcm16):
            raise ValueError("increased_compatibility_mode is the reference's sample doubling to 48 kHz PCM16: it does not combine with "
                             "sample_rate / pcm16")
        self._check_output_format(sample_rate, pcm16)
        n = len(text_list)
        column = lambda lst: list(lst) + [None] * (n - len(lst)) if lst else [None] * n
        durs, pits, enes = column(dur_list), column(pitch_list), column(energy_list)
        spoken = [i for i, t in enumerate(text_list) if t.strip() != ""]
        pieces, rows = {}, {}
        for lo in range(0, len(spoken), self.MAX_FILE_BATCH):
            chunk = spoken[lo:lo + self.MAX_FILE_BATCH]
            if not silent:
                for i in chunk:
                    print("Now synthesizing: {}".format(text_list[i]))
            # gold prosody is per sentence and optional per sentence: sentences that share the same set of gold quantities
            # form one batch (the engines take a quantity either for every utterance of a batch or for none)
            groups = {}
            for i in chunk:
                groups.setdefault((durs[i] is not None, pits[i] is not None, enes[i] is not None), []).append(i)
            for (has_d, has_p, has_e), idx in groups.items():
                waves = self.synthesize_batch([text_list[i] for i in idx], input_is_phones=input_is_phones,
                                              durations=[durs[i] for i in idx] if has_d else None,
                                              pitch=[pits[i] for i in idx] if has_p else None,
                                              energy=[enes[i] for i in idx] if has_e else None,
                                              duration_scaling_factor=duration_scaling_factor, pitch_variance_scale=pitch_variance_scale,
                                              energy_variance_scale=energy_variance_scale, sample_rate=sample_rate, pcm16=pcm16,
                                              loudness=loudness, peak_ceiling=peak_ceiling, speech_level=speech_level,
                                              true_peak_ceiling=true_peak_ceiling, limiter=limiter)
                for r, (i, w) in enumerate(zip(idx, waves)):
                    pieces[i] = w.cpu().numpy()
                    if normalise:
                        rows[i] = self.last_loudness[r]
                    if delivery:
                        delivery_rows[i] = self.last_delivery[r]
                    if level:
                        activity_rows[i] = tuple(t[r] for t in self.last_speech_activity)
        if normalise:
            self.last_loudness = torch.stack([rows[i] for i in spoken]) if spoken else torch.zeros((0, 8), dtype=torch.float64, device=self.device)
        if delivery:
            self.last_delivery = torch.stack([delivery_rows[i] for i in spoken]) if spoken else torch.zeros((0, 8), dtype=torch.float64, device=self.device)
        if level:
            empty = (torch.zeros((0, 8), dtype=torch.float64, device=self.device), torch.zeros((0, 64, 2), dtype=torch.int64, device=self.device),
                     torch.zeros((0, 16), dtype=torch.int64, device=self.device))
            self.last_speech_activity = tuple(torch.stack([activity_rows[i][k] for i in spoken]) for k in range(3)) if spoken else empty
        rate = self.SAMPLE_RATE if sample_rate is None else int(sample_rate)
        gap = self.SILENCE_SAMPLES
        if rate != self.SAMPLE_RATE:
            from . import resample
            gap = resample.out_length(gap, self.SAMPLE_RATE, rate)
        total = gap + sum(pieces[i].shape[0] + gap for i in spoken)
        audio = np.zeros(total, dtype=np.int16 if pcm16 else np.float32)
        at = gap
        for i in spoken:
            audio[at:at + pieces[i].shape[0]] = pieces[i]
            at += pieces[i].shape[0] + gap
        if increased_compatibility_mode:  # 24 kHz is less widely supported than 48 kHz: every sample twice, 16-bit integers
            write_wav(file_location, float2pcm(np.repeat(audio, 2)), 48000)
        else:
            write_wav(file_location, audio, rate)

    def read_aloud(self, text, view=False, duration_scaling_factor=1.0, pitch_variance_scale=1.0, energy_variance_scale=1.0,
                   blocking=False, increased_compatibility_mode=False):
        """Synthesise and play one text through the sound card (:287-309); half a second of silence is appended."""
        if not text.strip():
            return
        try:
            import sounddevice
        except ImportError as e:
            raise RuntimeError("read_aloud needs the sounddevice package") from e
        speech = self(text, view, duration_scaling_factor=duration_scaling_factor, pitch_variance_scale=pitch_variance_scale,
                      energy_variance_scale=energy_variance_scale)
        audio = np.concatenate([speech.cpu().numpy(), np.zeros(12000, dtype=np.float32)])
        if increased_compatibility_mode:
            sounddevice.play(float2pcm(np.repeat(audio, 2)), samplerate=48000)
        else:
            sounddevice.play(audio, samplerate=24000)
        if blocking:
            sounddevice.wait()


def get_language_id_tensor(language):
    """Preprocessing/TextFrontend.py:490-524 returns a LongTensor([id])."""
    i = get_language_id(language)
    if i is None:
        raise ValueError(f"language {language!r} has no id (TextFrontend.py:490-524)")
    return torch.LongTensor([i])
