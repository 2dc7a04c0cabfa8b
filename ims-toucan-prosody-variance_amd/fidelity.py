"""How far a generated 24 kHz waveform is from the recording it was generated from, on the GPU (csrc/fidelity.hip,
include/toucan_fidelity.h) for ragged batches of pairs: ``mel_l1``, the reference's vocoder training loss without its weight
(MelSpectrogramLoss.py: 1536-point Hann STFT, hop 384, 100 Slaney bands from 80 Hz to 12 kHz, L1 of log10 amplitudes), the same
per frame, and per STFT resolution the spectral convergence and the log-magnitude L1.  include/toucan_fidelity.h holds the
definition, DESIGN.md section 21 the decisions, tests/fidelity_ref.py the float64 restatement.

* ``SpectralDistance``: the measure between two lists of waveforms.
* ``VocoderScorer``: the reference's copy-synthesis (HiFiGANDataset.__getitem__ without the random window and without the
  corruption) - the recording at 24 kHz cut to whole frames, its 16 kHz / 80-bin log-mel, the vocoder on that mel, the distance
  between what the vocoder returns and the cut recording - with the bookkeeping of the corpus scorers (scorer.py).

The waveform is framed where it lies (tts_frame_reflect), the DFT is the fp32 conv that style.LogMel uses, and one pass over the two
spectra of a pair leaves four fp64 sums per frame (tts_spectral_distance, tts_spectral_reduce).  A batch returns bit for bit what
its pairs return alone.
"""
import math
import os

import numpy as np
import torch

from . import align, capi, engine, packing, resample, style
from .capi import MODE_LINEAR
from .ragged import Ragged

SR = 24000                      # what both vocoders generate and the reference's loss is defined at
N_MELS, FMIN, FMAX = 100, 80.0, 12000.0
REFERENCE_RESOLUTION = (1536, 384)  # (N, hop): the only one with a mel filterbank
DEFAULT_RESOLUTIONS = ((768, 192), (1536, 384), (3072, 768))
VOCODER_HOP = 384               # 24 kHz samples per mel frame
SUM_COLUMNS = ("mel", "diff_sq", "ref_sq", "log_mag")  # the rows of tts_spectral_distance / tts_spectral_reduce


def band_runs(mel):
    """A filterbank [n_mels, bins] whose bands are one run of non-zero bins each -> (int32 [n_mels, 2] = (first, count), float32
    weights of all runs one after the other).  ValueError for a band with a gap."""
    mel = np.asarray(mel, dtype=np.float32)
    bands, weights = np.zeros((mel.shape[0], 2), dtype=np.int32), []
    for m, row in enumerate(mel):
        nz = np.flatnonzero(row)
        if nz.size == 0:
            continue  # (0, 0): the band's energy is 0, its logarithm the floor's
        if nz[-1] - nz[0] + 1 != nz.size:
            raise ValueError(f"band {m} of the filterbank is not one run of bins")
        bands[m] = (nz[0], nz.size)
        weights.append(row[nz[0]: nz[-1] + 1])
    return bands, np.concatenate(weights) if weights else np.zeros(0, dtype=np.float32)


def dft_basis(n_fft):
    """float32 [4, hop, 2 (N / 2 + 1)]: the periodic Hann window folded into [cos | -sin], cut into the four rows of a frame."""
    n = np.arange(n_fft, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    ang = 2.0 * np.pi * np.outer(n, np.arange(n_fft // 2 + 1, dtype=np.float64)) / n_fft
    basis = np.concatenate([win[:, None] * np.cos(ang), -win[:, None] * np.sin(ang)], axis=1)
    return basis.reshape(4, n_fft // 4, -1).astype(np.float32)


def check_resolution(n_fft, hop):
    if int(n_fft) != n_fft or int(hop) != hop or n_fft != 4 * hop or hop % 4 or hop < 4 or n_fft // 2 + 1 > capi.FIDELITY_MAX_BINS:
        raise ValueError(f"resolution ({n_fft!r}, {hop!r}): N = 4 hop, hop a multiple of 4, N at most {2 * (capi.FIDELITY_MAX_BINS - 1)}")
    return int(n_fft), int(hop)


def frame_count(n, hop):
    """Frames of the centred STFT of n samples."""
    return 1 + int(n) // int(hop)


def padded_rows(n, hop):
    """Rows of ``hop`` samples that hold n samples with their reflection of 2 hop on both sides."""
    return 4 + -(-int(n) // int(hop))


def check_length(n, n_fft, what="the signal"):
    if n <= n_fft // 2:
        raise ValueError(f"{what} has {n} samples: the centred {n_fft}-point STFT with reflection padding needs more than {n_fft // 2}")


def copy_synthesis_plan(n24, resolutions=DEFAULT_RESOLUTIONS):
    """A recording of n24 samples at 24 kHz -> (F, 384 F, 256 F): the mel frames the vocoder is fed, the samples of the cut
    recording (and of what the vocoder returns) and the samples at 16 kHz whose log-mel has F + 1 frames, the last one dropped.
    ValueError where the cut recording is too short for a resolution."""
    F = int(n24) // VOCODER_HOP
    for n_fft, _ in resolutions:
        check_length(VOCODER_HOP * F, n_fft, f"a recording of {int(n24)} samples at 24 kHz, cut to {F} frames,")
    check_length(256 * F, style.N_FFT, "the 16 kHz side of the recording")
    return F, VOCODER_HOP * F, (VOCODER_HOP * F * 2) // 3


def _wave_on(device, w):
    """One waveform, array or tensor, mono -> float32 [n] on the device (a tensor that is there already is not copied)."""
    if torch.is_tensor(w):
        t = w.detach()
    else:
        a = np.asarray(w)
        if a.ndim == 2:
            a = a.mean(axis=1)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).reshape(-1).contiguous()


class SpectralDistance:
    """``distance(waves_a, waves_b, ...)`` for ragged lists of waveforms; holds the DFT bases, the filterbank runs and the
    ``Resampler``.  ``frame(packed, spans, hop)`` is the framing alone."""

    def __init__(self, device):
        self.ops = engine.Ops(device)
        self.lib, self.device = self.ops.lib, self.ops.device
        self.resampler = resample.Resampler(self.device)
        self.frames_per_group = int(self.lib.tts_spectral_frames_per_group())
        self.reduce_sweep = int(self.lib.tts_spectral_reduce_sweep())
        self._bases = {}
        self.mel = style.mel_filterbank(SR, REFERENCE_RESOLUTION[0], N_MELS, FMIN, FMAX)
        self.bands, weights = band_runs(self.mel)
        self.bands_d = torch.from_numpy(self.bands).to(self.device)
        self.weights_d = torch.from_numpy(weights).to(self.device)
        self.last_frame_sums = {}  # (N, hop) -> float64 [B, max_frames, 4] on the device, of the last call

    def basis(self, n_fft):
        """The packed conv weights of the DFT (cached).  packing.ConvWeights pads Cin to a multiple of 32 and Cout to the conv's
        column tile with zeros: 770 / 1538 / 3074 columns are not multiples of it."""
        if n_fft not in self._bases:
            self._bases[n_fft] = packing.ConvWeights(dft_basis(n_fft), None, MODE_LINEAR, 1, 0, self.device)
        return self._bases[n_fft]

    def _i64(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.device)

    @torch.inference_mode()
    def frame(self, packed, spans, hop):
        """packed: float32 [S] on the device; spans: [(first sample, sample count)] -> (rows [total_rows, hop], Ragged of the rows of
        every utterance): 2 hop reflected samples, the utterance, 2 hop reflected samples, zeros to the end of the last row - the
        buffer align.batched_spectra builds on the host.  One launch, no host copy of the waveform."""
        assert packed.dtype == torch.float32 and packed.dim() == 1 and packed.device == self.device and packed.is_contiguous()
        sp = np.asarray([(int(b), int(n)) for b, n in spans], dtype=np.int64).reshape(-1, 2)
        for u, (_, n) in enumerate(sp):
            check_length(int(n), 4 * hop, f"utterance {u}")
        counts = [padded_rows(n, hop) for _, n in sp]
        begins = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if len(counts) else np.zeros(0, dtype=np.int64)
        total = int(sum(counts))
        rows = torch.empty((total, hop), dtype=torch.float32, device=self.device)
        if len(sp):
            sp_d, rb_d = self._i64(sp), self._i64(begins)
            capi.check(self.lib.tts_frame_reflect(packed.data_ptr(), packed.numel(), sp_d.data_ptr(), sp.ctypes.data, len(sp), int(sp[:, 1].max()),
                                                  int(hop), rb_d.data_ptr(), begins.ctypes.data, total, rows.data_ptr(), self.ops.stream()),
                       "tts_frame_reflect")
        return rows, Ragged(counts, self.device, begins=[int(b) for b in begins])

    @torch.inference_mode()
    def spectra(self, packed, spans, n_fft):
        """-> (spectrum [total_rows, 2 bins] = [re | im] per row, Ragged of the padded rows): frame f of utterance u is row
        rag.begins[u] + f.  Both launches cover every span."""
        n_fft, hop = check_resolution(n_fft, n_fft // 4)
        rows, rag = self.frame(packed, spans, hop)
        spec = self.ops.conv(self.basis(n_fft), rows, self.ops.empty(rag.total_rows, n_fft + 2), rag, compute=capi.COMPUTE_F32, split_k=False)
        return spec, rag

    @torch.inference_mode()
    def sums(self, spec, bins, pairs, with_mel):
        """spec [rows, >= 2 bins]; pairs: [(first row of a, first row of b, frames)] -> (frame sums float64 [B, max_frames, 4] - the
        slots past a pair's frames are not written -, totals float64 [B, 4]) on the device, columns ``SUM_COLUMNS``."""
        assert spec.dtype == torch.float32 and spec.dim() == 2 and spec.stride(1) == 1 and spec.device == self.device
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
        B, max_frames = len(pr), max(1, int(pr[:, 2].max()) if len(pr) else 1)
        frame_sums = torch.empty((B, max_frames, capi.FIDELITY_SUMS), dtype=torch.float64, device=self.device)
        totals = torch.empty((B, capi.FIDELITY_SUMS), dtype=torch.float64, device=self.device)
        if B == 0:
            return frame_sums, totals
        pr_d = self._i64(pr)
        n_bands = len(self.bands) if with_mel else 0
        if with_mel:
            assert bins == self.mel.shape[1]
        capi.check(self.lib.tts_spectral_distance(spec.data_ptr(), int(spec.stride(0)), int(bins), int(spec.shape[0]), pr_d.data_ptr(), pr.ctypes.data, B,
                                                  max_frames, self.bands_d.data_ptr() if with_mel else None, self.bands.ctypes.data if with_mel else None,
                                                  n_bands, self.weights_d.data_ptr() if with_mel else None, self.weights_d.numel() if with_mel else 0,
                                                  frame_sums.data_ptr(), self.ops.stream()), "tts_spectral_distance")
        capi.check(self.lib.tts_spectral_reduce(frame_sums.data_ptr(), pr_d.data_ptr(), B, max_frames, totals.data_ptr(), self.ops.stream()),
                   "tts_spectral_reduce")
        return frame_sums, totals

    @torch.inference_mode()
    def distance_packed(self, packed, pair_spans, resolutions=DEFAULT_RESOLUTIONS, keep_frames=False, lengths=None):
        """packed: float32 [S] on the device; pair_spans: [(first sample of a, first sample of b, samples)] -> one record per pair
        (see ``distance``).  Per resolution: one framing launch and one DFT launch for both signals of all pairs, one distance
        launch, one reduce launch; the totals come to the host once, at the end."""
        resolutions = [check_resolution(n, h) for n, h in resolutions]
        spans = [s for a, b, n in pair_spans for s in ((a, n), (b, n))]
        for n_fft, _ in resolutions:
            for p, (_, _, n) in enumerate(pair_spans):
                check_length(int(n), n_fft, f"pair {p}")
        B = len(pair_spans)
        totals, self.last_frame_sums = {}, {}
        for n_fft, hop in resolutions:
            spec, rag = self.spectra(packed, spans, n_fft)
            pairs = [(rag.begins[2 * p], rag.begins[2 * p + 1], frame_count(pair_spans[p][2], hop)) for p in range(B)]
            self.last_frame_sums[(n_fft, hop)], totals[(n_fft, hop)] = self.sums(spec, n_fft // 2 + 1, pairs, (n_fft, hop) == REFERENCE_RESOLUTION)
        host = {k: v.cpu().numpy() for k, v in totals.items()}
        records = []
        for p, (_, _, n) in enumerate(pair_spans):
            rec = {"samples": int(n), "lengths": tuple(lengths[p]) if lengths is not None else (int(n), int(n)), "mel_l1": None, "resolutions": {}}
            for n_fft, hop in resolutions:
                t, F, bins = host[(n_fft, hop)][p], frame_count(n, hop), n_fft // 2 + 1
                rec["resolutions"][(n_fft, hop)] = {"spectral_convergence": float(np.sqrt(t[1]) / np.sqrt(t[2])), "log_magnitude_l1": float(t[3] / (F * bins))}
                if (n_fft, hop) == REFERENCE_RESOLUTION:
                    per_frame = self.last_frame_sums[(n_fft, hop)][p, :F, 0] / N_MELS
                    worst = int(torch.argmax(per_frame))  # (a NaN frame is the largest)
                    rec.update(mel_l1=float(t[0] / (F * N_MELS)), frames=F, worst_frame=worst, worst_frame_seconds=worst * hop / SR)
                    if keep_frames:
                        rec["frame_mel_l1"] = per_frame
            records.append(rec)
        return records

    @torch.inference_mode()
    def distance(self, waves_a, waves_b, sr_a=SR, sr_b=None, resolutions=DEFAULT_RESOLUTIONS, keep_frames=False):
        """waves_a: the generated signals, waves_b: the recordings - lists of 1-D arrays or device tensors of any lengths, at sr_a and
        sr_b (default: sr_a); what is not at 24 kHz is converted on the device.  A pair is cut to its shorter signal.  -> one dict
        per pair: ``mel_l1``, ``frames``, ``worst_frame`` (the frame with the largest mel distance) and ``worst_frame_seconds`` (its
        centre) - these four only with the reference resolution (1536, 384) among ``resolutions``, else ``mel_l1`` is None -,
        ``frame_mel_l1`` (float64 [frames] on the device) with keep_frames, ``resolutions``: {(N, hop): {``spectral_convergence``,
        ``log_magnitude_l1``}}, ``lengths``: the samples of both signals at 24 kHz before the cut, ``samples``: after it.
        ValueError where a pair is not longer than N / 2 of a resolution."""
        if len(waves_a) != len(waves_b):
            raise ValueError(f"{len(waves_a)} generated signals for {len(waves_b)} recordings")
        sides = []
        for waves, sr in ((waves_a, sr_a), (waves_b, sr_a if sr_b is None else sr_b)):
            ts = [_wave_on(self.device, w) for w in waves]
            if int(sr) != SR and ts:
                counts = [t.numel() for t in ts]
                begins = np.concatenate([[0], np.cumsum(counts)[:-1]])
                y, out = self.resampler.resample(torch.cat(ts), list(zip(begins.tolist(), counts)), int(sr), SR)
                ts = [y[b: b + n] for b, n in out]
            sides.append(ts)
        parts, pair_spans, lengths, at = [], [], [], 0
        for a, b in zip(*sides):
            n = min(a.numel(), b.numel())
            parts += [a[:n], b[:n]]
            pair_spans.append((at, at + n, n))
            lengths.append((a.numel(), b.numel()))
            at += 2 * n
        packed = torch.cat(parts) if parts else torch.empty(0, dtype=torch.float32, device=self.device)
        return self.distance_packed(packed, pair_spans, resolutions, keep_frames, lengths)


class CopySynthesis:
    """The chain behind ``VocoderScorer`` and ``ToucanTTSInterface.vocoder_fidelity`` for a vocoder given as a callable
    ``vocode(mel_packed [rows, 80], Ragged) -> (packed 24 kHz wave, Ragged of samples)``."""

    def __init__(self, vocode, device):
        self.measure = SpectralDistance(device)
        self.device, self.ops = self.measure.device, self.measure.ops
        self.logmel = style.LogMel(self.device)
        self.vocode = vocode
        self._intelligibility = None  # intelligibility.Intelligibility, built on first use

    @torch.inference_mode()
    def recordings_24k(self, waves, sr):
        """waves at sr -> (packed 24 kHz wave on the device, [(first sample, 384 F)] of the cut recordings, [F])."""
        ts = [_wave_on(self.device, w) for w in waves]
        counts = [t.numel() for t in ts]
        begins = np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist() if ts else []
        packed, spans = torch.cat(ts), list(zip(begins, counts))
        if int(sr) != SR:
            packed, spans = self.measure.resampler.resample(packed, spans, int(sr), SR)
        frames = [copy_synthesis_plan(n)[0] for _, n in spans]
        return packed, [(int(b), VOCODER_HOP * F) for (b, _), F in zip(spans, frames)], frames

    @torch.inference_mode()
    def log_mel_16k(self, packed24, spans24, frames):
        """The cut recordings -> (log-mel [rows, 80] as the vocoders are fed it - 16 kHz, 80 bins, not normalised -, Ragged of the F
        frames of every utterance: the front end's last frame is dropped).  Framed on the device; the same launches behind the
        framing as align.batched_spectra and align.batched_log_mel."""
        wave16, spans16 = self.measure.resampler.resample(packed24, spans24, SR, style.SR)
        rows, rag_rows = self.measure.frame(wave16, spans16, style.HOP)
        spec = self.ops.conv(self.logmel.dft, rows, self.ops.empty(rag_rows.total_rows, 2 * self.logmel.bins), rag_rows, compute=capi.COMPUTE_F32,
                             split_k=False)
        for (_, n16), F in zip(spans16, frames):
            assert frame_count(n16, style.HOP) == F + 1
        rag = Ragged(frames, self.device, begins=rag_rows.begins)
        return align.batched_log_mel(self.ops, self.logmel, spec, rag_rows), rag

    @torch.inference_mode()
    def intelligibility_of(self, both, pair_spans):
        """both: the packed 24 kHz wave; pair_spans: [(first sample of the generated signal, of the recording, samples)] -> the
        records of ``intelligibility.Intelligibility.score_packed`` on the two at 10 kHz."""
        if self._intelligibility is None:
            from . import intelligibility
            self._intelligibility = intelligibility.Intelligibility(self.device)
        spans = [s for ga, rb, n in pair_spans for s in ((rb, n), (ga, n))]
        wave10, spans10 = self.measure.resampler.resample(both, spans, SR, capi.STOI_RATE)
        return self._intelligibility.score_packed(wave10, [(spans10[2 * p][0], spans10[2 * p + 1][0], spans10[2 * p][1]) for p in range(len(pair_spans))])

    @torch.inference_mode()
    def run(self, waves, sr, resolutions=DEFAULT_RESOLUTIONS, keep_frames=False, keep_waves=False, intelligibility=False):
        """-> one record of ``SpectralDistance.distance`` per recording; keep_waves adds ``generated`` and ``recording``, the two
        24 kHz signals that were compared (device tensors); intelligibility adds ``stoi``, ``estoi`` and ``intelligibility_status``
        of the same two signals at 10 kHz (intelligibility.py)."""
        if len(waves) == 0:
            return []
        packed24, spans24, frames = self.recordings_24k(waves, sr)
        mel, rag = self.log_mel_16k(packed24, spans24, frames)
        wav, rag_w = self.vocode(mel, rag)
        assert rag_w.lengths == [VOCODER_HOP * F for F in frames]
        at = wav.numel()
        both = torch.cat([wav, packed24])
        pair_spans = [(ga, at + rb, n) for ga, (rb, n) in zip(rag_w.begins, spans24)]
        records = self.measure.distance_packed(both, pair_spans, resolutions, keep_frames)
        if intelligibility:
            for rec, got in zip(records, self.intelligibility_of(both, pair_spans)):
                rec.update(stoi=got["stoi"], estoi=got["estoi"], intelligibility_status=got["status"])
        if keep_waves:
            for rec, (ga, rb, n) in zip(records, pair_spans):
                rec["generated"], rec["recording"] = both[ga: ga + n], both[rb: rb + n]
        return records


class ScoredRecordings:
    """What ``current_dset`` is for the corpus scorers (scorer.ScoredCorpus), without a cache file: ``datapoints`` are the keys of
    the recordings that are left."""

    def __init__(self, datapoints):
        self.datapoints = datapoints

    def __len__(self):
        return len(self.datapoints)

    def remove_samples(self, list_of_samples_to_remove):
        for remove_id in sorted(set(int(i) for i in list_of_samples_to_remove), reverse=True):  # (an id listed twice is removed once)
            self.datapoints.pop(remove_id)
        print("Dataset updated!")


class ScoreBook:
    """The bookkeeping the corpus scorers share (scorer.py), for scores that come with a key each: ``path_to_score``, the NaNs,
    listing and removal.  A NaN among the n worst is removed once (the scorers' deviation row)."""

    def __init__(self):
        self.path_to_score, self.path_to_id, self.path_to_record = dict(), dict(), dict()
        self.nans, self.nan_indexes = list(), list()
        self.nans_removed = False
        self.current_dset = None

    def record_scores(self, keys, scores, records=None):
        """keys in the order they were given, one score each."""
        self.path_to_score, self.path_to_id, self.path_to_record = dict(), dict(), dict()
        self.nans, self.nan_indexes = list(), list()
        self.current_dset = ScoredRecordings(list(keys))
        for index, key in enumerate(keys):
            loss = float(scores[index])
            if math.isnan(loss):
                self.nans.append(key)
                self.nan_indexes.append(index)
            self.path_to_score[key] = loss
            self.path_to_id[key] = index
            if records is not None:
                self.path_to_record[key] = records[index]
        if len(self.nans) > 0:
            print("NaNs detected during scoring!")
            for path in self.nans:
                print(path)
            print("\n\n")
        self.nans_removed = False

    def show_samples_with_highest_loss(self, n=-1):
        """
        NaN samples will always be shown.
        To see all samples, pass -1, otherwise n samples will be shown.
        """
        from . import scorer
        scorer._show(self.path_to_score, self.nans, n, trailing_blank=True)

    def remove_samples_with_highest_loss(self, n=10):
        if self.current_dset is None:
            print("Please run the scoring first.")
        elif self.nans_removed:
            print("Indexes are no longer accurate. Please re-run the scoring. \n\n"
                  "This function also removes NaNs, so if you want to remove the NaN samples and the n samples "
                  "with the highest loss, only call this function.")
        else:
            remove_ids = list(self.nan_indexes)
            for index, path in enumerate(sorted(self.path_to_score, key=self.path_to_score.get, reverse=True)):
                if index < n:
                    remove_ids.append(self.path_to_id[path])
            self.current_dset.remove_samples(remove_ids)
            self.nans_removed = True


class VocoderScorer(ScoreBook):
    """Copy-synthesis scores of recordings for one vocoder checkpoint at one precision: ``score`` fills ``path_to_score`` with the
    ``mel_l1`` of every recording (``path_to_record``: the whole record), ``show_samples_with_highest_loss`` and
    ``remove_samples_with_highest_loss`` as the corpus scorers have them; ``current_dset.datapoints`` are the keys that are left."""

    def __init__(self, path_to_vocoder_model=None, device="cuda", faster_vocoder=False, precision=None):
        from .interface import MODELS_DIR, _load_checkpoint, _to_numpy_sd
        super().__init__()
        if path_to_vocoder_model is None:
            path_to_vocoder_model = os.path.join(MODELS_DIR, "Avocodo" if faster_vocoder else "BigVGAN", "best.pt")
        if precision is None:  # as the interface reads it: its vocoder runs "mixed" configurations on the fp16 matrix cores
            precision = os.environ.get("TOUCAN_PRECISION", "f32")
            precision = "f16" if precision in ("mixed", "mixed3") else precision
        self.precision = precision
        sd = _to_numpy_sd(_load_checkpoint(path_to_vocoder_model)["generator"])
        self.vocoder = engine.VocoderEngine(sd, "hifigan" if faster_vocoder else "bigvgan", device, precision=precision)
        self.device = self.vocoder.device
        self.chain = CopySynthesis(self.vocoder.forward, self.device)

    def score_waves(self, waves, sr, batch_size=32, keep_frames=False, intelligibility=False):
        """waves: 1-D arrays or tensors at sr -> the records in the waves' order, batches of batch_size sorted by length;
        intelligibility: every record also holds ``stoi``, ``estoi`` and ``intelligibility_status``."""
        from . import scorer
        records = [None] * len(waves)
        for batch in scorer._batches([int(np.shape(w)[0]) for w in waves], batch_size):
            for i, rec in zip(batch, self.chain.run([waves[i] for i in batch], sr, keep_frames=keep_frames, intelligibility=intelligibility)):
                records[i] = rec
        return records

    def score(self, paths_or_waves, sr=None, batch_size=32, intelligibility=False, rank_by="mel_l1"):
        """
        call this to update the path_to_score dict with scores for these recordings: paths of audio files, or waveforms at ``sr``
        (their keys are "wave <index>"); intelligibility adds STOI and ESTOI to the records, and rank_by="estoi" (which implies it)
        makes 1 - estoi the score the listing and the removal go by
        """
        if rank_by not in ("mel_l1", "estoi"):
            raise ValueError(f"rank_by is 'mel_l1' or 'estoi', not {rank_by!r}")
        intelligibility = bool(intelligibility) or rank_by == "estoi"
        keys, waves, rates = [], [], []
        for index, item in enumerate(paths_or_waves):
            if isinstance(item, (str, os.PathLike)):
                data, rate = style.read_audio(item)
                keys.append(str(item))
            else:
                if sr is None:
                    raise ValueError("waveforms need their sample rate: score(waves, sr=...)")
                data, rate = item, int(sr)
                keys.append(f"wave {index}")
            waves.append(_wave_on("cpu", data))
            rates.append(rate)
        records = [None] * len(waves)
        for rate in sorted(set(rates)):  # one batch holds one rate
            idx = [i for i, r in enumerate(rates) if r == rate]
            for i, rec in zip(idx, self.score_waves([waves[i] for i in idx], rate, batch_size, intelligibility=intelligibility)):
                records[i] = rec
        self.record_scores(keys, [1.0 - r["estoi"] if rank_by == "estoi" else r["mel_l1"] for r in records], records)
