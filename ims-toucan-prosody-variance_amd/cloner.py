"""Drop-in counterpart of InferenceInterfaces/UtteranceCloner.py (:19-194) on the HIP engines: the reference's constructor and
methods, with the prosody extracted on the GPU (align.py) for one recording or a ragged batch of them.

Stated deviations: the transcript is a phoneme string (no G2P offline); by default ``on_line_fine_tune=True`` is
accepted with a one-time warning and not performed (the reference's five SGD steps of CTC training), so the result is that of the
eval-mode aligner - an instance made with ``fine_tune_aligner=True`` performs it on the GPU (finetune.py), per utterance from the
checkpoint's weights, with dropout masks drawn from ``torch.Generator(fine_tune_seed)`` as the reference draws them on a CPU device
(or given as ``dropout_masks=``); there is no silero voice-activity trim (the silences are 0 unless ``speech_bounds`` gives the speech span, or is "detect": the ITU-T P.56 activity meter then finds it);
pitch comes from ``f0=``: a frame-level track, or ``"track"`` for the device pitch tracker (pitch.py: Praat's autocorrelation
method restated from its publication, parity with Praat unpinned and therefore opt-in; ``track_pitch=True`` makes it the default of
this instance); with neither, pitch is None and the acoustic model predicts it from the cloned durations.
"""
import os
import warnings

import torch

from . import align, pitch, style
from . import interface
from .interface import ToucanTTSInterface, write_wav


class UtteranceCloner:
    _warned_fine_tune = False

    def __init__(self, model_id, device, language="en", speed_over_quality=False, track_pitch=False, fine_tune_aligner=False,
                 fine_tune_seed=0):
        self.tts = ToucanTTSInterface(device=device, tts_model_path=model_id, faster_vocoder=speed_over_quality, language=language)
        self.device = device
        self.language = language
        self.track_pitch = track_pitch  # additive: methods called without f0= behave as f0="track"
        self.fine_tune_aligner = fine_tune_aligner  # additive: on_line_fine_tune=True is performed instead of warned about
        self.fine_tune_seed = fine_tune_seed  # every utterance's dropout masks start from this seed
        path = os.path.join(interface.MODELS_DIR, "Aligner", "aligner.pt")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path}: aligner checkpoint not found (offline, write the fixture one with "
                                    f"ims_toucan_prosody_variance_amd.interface.write_fixture_aligner_checkpoint)")
        self.aligner_weights = torch.load(path, map_location="cpu", weights_only=True)["asr_model"]
        self.extractor = align.ProsodyExtractor(self.aligner_weights, device)

    def _fine_tune_notice(self, on_line_fine_tune):
        if on_line_fine_tune and not UtteranceCloner._warned_fine_tune:
            UtteranceCloner._warned_fine_tune = True
            warnings.warn("on_line_fine_tune=True: the aligner's on-line CTC fine-tuning is not performed; the durations are those of "
                          "the aligner as loaded (the reference's on_line_fine_tune=False, in eval mode)", stacklevel=3)

    def extract_prosody_batch(self, transcripts, waves, sr, f0=None, speech_bounds=None, on_line_fine_tune=True, dropout_masks=None):
        """Per utterance (durations, pitch or None, energy, start_silence, end_silence) for phoneme transcripts and recordings at `sr`.
        speech_bounds: None, per utterance a (start, end) pair or "detect", or "detect" for all (align.extract_prosody_batch).
        dropout_masks (fine_tune_aligner instances): per utterance [5 steps][5 layers] boolean [T, 512] keep-masks in place of the
        ones drawn from fine_tune_seed."""
        fine_tune = None
        if dropout_masks is not None and not (self.fine_tune_aligner and on_line_fine_tune):
            raise ValueError("dropout_masks= needs fine_tune_aligner=True and on_line_fine_tune=True")
        if self.fine_tune_aligner:
            if on_line_fine_tune:
                fine_tune = [self.fine_tune_seed] * len(waves) if dropout_masks is None else list(dropout_masks)
        else:
            self._fine_tune_notice(on_line_fine_tune)
        if f0 is None and self.track_pitch:
            f0 = pitch.TRACK
        return align.extract_prosody_batch(self.extractor, transcripts, waves, sr, f0=f0, speech_bounds=speech_bounds, fine_tune=fine_tune)

    def extract_prosody(self, transcript, ref_audio_path, lang="de", on_line_fine_tune=True, f0=None, speech_bounds=None, dropout_masks=None):
        """UtteranceCloner.py:46-145: (duration, pitch, energy, start_silence, end_silence) for one recording.  `lang` only selects
        the phonemizer in the reference; the transcript here is already phonemes."""
        if not self.fine_tune_aligner:
            self._fine_tune_notice(on_line_fine_tune)
        wave, sr = style.read_audio(ref_audio_path)
        return self.extract_prosody_batch([transcript], [wave], sr, f0=None if f0 is None else [f0],  # [f0]: an array or "track"
                                          speech_bounds=None if speech_bounds is None else [speech_bounds],
                                          on_line_fine_tune=on_line_fine_tune and self.fine_tune_aligner,
                                          dropout_masks=None if dropout_masks is None else [dropout_masks])[0]

    def word_prominence(self, transcript, path, speech_bounds=None, weights=(1.0, 1.0, 0.5), band=(1, 3)):
        """Additive: which words the speaker of a recording stresses (prominence.ProminenceMeter.measure).  The
        speech span of the normalised 16 kHz recording (``speech_bounds`` as ``extract_prosody`` takes it: None, a (start, end)
        pair or "detect") goes through the pitch tracker and the frame energy, the aligner of this cloner and MAS lay the
        transcript's phonemes onto its frames.  -> dict ``report`` (float64 [words, 8], columns ``prominence.COLUMNS``), ``words``
        ((start, stop) phonemes of every word) and ``durations``; ``prominence.to_emphasis(feats, report)`` turns it into Spans that
        give another voice the same emphasis without cloning every duration."""
        from . import prominence, prosody
        from .phonemes import phones_to_features
        if getattr(self, "_prominence_obj", None) is None:
            self._prominence_obj = prominence.ProminenceMeter(self.device, extractor=self.extractor)
        wave, sr = style.read_audio(path)
        norm = style.normalize_reference_audio(wave, sr)
        if isinstance(speech_bounds, str):
            if speech_bounds != align.DETECT:
                raise ValueError(f"speech_bounds takes a (start, end) pair or {align.DETECT!r}, not {speech_bounds!r}")
            speech_bounds = align.detect_speech_bounds(self.extractor, [norm])[0]
        if speech_bounds is not None:
            norm = norm[int(speech_bounds[0]):int(speech_bounds[1])]
        feats = phones_to_features(transcript, handle_missing=False) if isinstance(transcript, str) else transcript
        feats = feats.float().cpu().numpy() if torch.is_tensor(feats) else feats
        meter = self._prominence_obj
        report = meter.measure([norm], style.SR, [feats], weights=weights, band=band)[0]
        phones = meter.last["phoneme_frames"][0]
        return {"report": report, "words": prosody.word_spans(feats), "durations": phones[:, 1] - phones[:, 0]}

    def clone_utterance(self, path_to_reference_audio_for_intonation, path_to_reference_audio_for_voice, transcription_of_intonation_reference,
                        filename_of_result=None, lang="de", f0=None, speech_bounds=None, z_noise=None, evaluate=False):
        """UtteranceCloner.py:147-164: the voice of one recording speaking with the prosody of another.  evaluate (additive): also
        return how close the clone is to the intonation reference - (waveform, dict) with the measures of
        compare.SpeechComparator.compare (MCD along the warping path, F0 RMSE, log-F0 correlation, GPE, VDE, FFE): the 24 kHz clone
        without its padded silences against the speech span of the normalised 16 kHz reference, the wave the prosody was taken from."""
        self.tts.set_utterance_embedding(path_to_reference_audio=path_to_reference_audio_for_voice)
        duration, pitch, energy, sil_start, sil_end = self.extract_prosody(transcription_of_intonation_reference,
                                                                           path_to_reference_audio_for_intonation, lang=lang, f0=f0,
                                                                           speech_bounds=speech_bounds)
        self.tts.set_language(lang)
        cloned = self.tts(transcription_of_intonation_reference, view=False, durations=duration, pitch=pitch, energy=energy,
                          input_is_phones=True, z_noise=z_noise)
        utt = self._pad_and_write(cloned, sil_start, sil_end, filename_of_result)
        if not evaluate:
            return utt
        data, sr = style.read_audio(path_to_reference_audio_for_intonation)
        ref16 = style.normalize_reference_audio(data, sr)
        if isinstance(speech_bounds, str):  # "detect": the span that was found is what the silences leave
            ref16 = ref16[sil_start:len(ref16) - sil_end]
        elif speech_bounds is not None:
            ref16 = ref16[int(speech_bounds[0]):int(speech_bounds[1])]
        report = self.tts._comparator().compare([cloned.reshape(-1).float().cpu().numpy()], [ref16], self.tts.SAMPLE_RATE, style.SR)[0]
        return utt, report

    def biblical_accurate_angel_mode(self, path_to_reference_audio_for_intonation, transcription_of_intonation_reference,
                                     list_of_speaker_references_for_ensemble, filename_of_result=None, lang="de", f0=None, speech_bounds=None,
                                     z_noise=None):
        """UtteranceCloner.py:166-194: several voices with the same prosody, averaged - one batch over the voices."""
        duration, pitch, energy, sil_start, sil_end = self.extract_prosody(transcription_of_intonation_reference,
                                                                           path_to_reference_audio_for_intonation, lang=lang, f0=f0,
                                                                           speech_bounds=speech_bounds)
        self.tts.set_language(lang)
        prev = self.tts.default_utterance_embedding.clone()
        embs = []
        for p in list_of_speaker_references_for_ensemble:
            self.tts.set_utterance_embedding(path_to_reference_audio=p)
            embs.append(self.tts.default_utterance_embedding.clone())
        self.tts.default_utterance_embedding = prev  # return to normal
        cloned = self.tts.synthesize_ensemble(transcription_of_intonation_reference, embs, durations=duration, pitch=pitch, energy=energy,
                                              input_is_phones=True, z_noise=z_noise)
        return self._pad_and_write(cloned, sil_start, sil_end, filename_of_result)

    def _pad_and_write(self, cloned, sil_start, sil_end, filename):
        # silences are counted at 16 kHz, the output runs at 48 kHz in the reference's arithmetic: x 3 (UtteranceCloner.py:158-159)
        start = torch.zeros([sil_start * 3])
        end = torch.zeros([sil_end * 3])
        utt = torch.cat((start, cloned.reshape(-1).float().cpu(), end), dim=0).numpy()
        if filename is not None:
            write_wav(filename, utt, 24000)
        return utt
