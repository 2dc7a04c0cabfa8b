"""Which words came out prominent in the AUDIO, and how strong the breaks between them are, on the GPU (csrc/prominence.hip,
include/toucan_prominence.h) for ragged batches: the continuous wavelet transform of a composite prosodic signal - f0, energy and
phoneme rate per frame, gap-filled and z-normalised - whose word-scale band has its maxima at the prominent words and its minima
at the phrase breaks (Suni, Simko, Aalto, Vainio 2017).  The measure is restated from the publication, with the band sum standing in
for its lines of maximum amplitude: PARITY with the authors' toolkit is UNPINNED, and numbers compare only with numbers of this
definition.  include/toucan_prominence.h holds the definition, DESIGN.md section 24 the decisions, tests/prominence_ref.py the
float64 restatement.

The front ends are the project's own, all at 62.5 frames/s: the cloner's STFT with tts_frame_energy, pitch.PitchTracker laid onto
the STFT's frames by align.adjust_num_frames_centered, and phoneme durations from the synthesis (``tts.last_durations``) or from the
aligner with MAS.  A batch returns bit for bit what its utterances return alone.

The module-level functions need no GPU.
"""
import math

import numpy as np
import torch

from . import capi, prosody

COLUMNS = ("prominence", "peak_frame", "mean", "pitch_part", "energy_part", "rate_part", "boundary_after", "valley_frame")  # a row of a report
CHANNELS = ("pitch", "energy", "rate")
N_SCALES, MAX_TAPS, TABLE_LD = capi.PROMINENCE_SCALES, capi.PROMINENCE_MAX_TAPS, capi.PROMINENCE_TABLE_LD
SCALES = tuple(2 ** (j + 1) for j in range(N_SCALES))  # frames
MAX_FRAMES = capi.PROMINENCE_MAX_FRAMES  # of one utterance: 17.5 minutes
SR, HOP = 16000, 256
FRAME_RATE = SR / HOP
DEFAULT_WEIGHTS = (1.0, 1.0, 0.5)  # pitch, energy, rate: chosen here, not measured against listeners
DEFAULT_BAND = (1, 3)  # scales of 4, 8 and 16 frames: 64 to 256 ms, the span of a syllable to a short word


def wavelet_table():
    """float64 [6, 1026]: row j holds psi(k / s_j), k = -8 s_j .. 8 s_j, for s_j = 2^(j + 1) - 16 s_j + 1 taps, zeros behind them - and
    in its last column s_j^(-1/2).  psi(u) = 2 / (sqrt(3) pi^(1/4)) (1 - u^2) exp(-u^2 / 2)."""
    table = np.zeros((N_SCALES, TABLE_LD), dtype=np.float64)
    c = 2.0 / (math.sqrt(3.0) * math.pi ** 0.25)
    for j, s in enumerate(SCALES):
        u = np.arange(-8 * s, 8 * s + 1, dtype=np.float64) / float(s)
        table[j, :16 * s + 1] = c * (1.0 - u * u) * np.exp(-0.5 * u * u)
        table[j, MAX_TAPS] = float(s) ** -0.5
    return table


def check_weights(weights):
    """-> the three weights as floats; ValueError unless every one is finite and not negative."""
    w = tuple(float(v) for v in weights)
    if len(w) != 3:
        raise ValueError(f"weights holds one value per channel {CHANNELS}, got {len(w)}")
    for name, v in zip(CHANNELS, w):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"the {name} weight is {v!r}: a weight is finite and not negative")
    return w


def check_band(band):
    """-> (j_lo, j_hi); ValueError unless 0 <= j_lo <= j_hi <= 5."""
    lo, hi = band
    if isinstance(lo, bool) or isinstance(hi, bool) or int(lo) != lo or int(hi) != hi or not 0 <= lo <= hi < N_SCALES:
        raise ValueError(f"the band {tuple(band)!r} is outside 0 .. {N_SCALES - 1}: it is (j_lo, j_hi) with j_lo <= j_hi, the scales 2^(j + 1) frames")
    return int(lo), int(hi)


def check_ranges(ranges, frames, utterance, kind):
    """int32 [n, columns] of ascending, disjoint [begin, end) ranges inside [0, frames]; ValueError names the utterance and the range."""
    a = np.asarray(ranges)
    cols = 3 if kind == "phoneme" else 2
    a = a.reshape(-1, cols) if a.size else np.zeros((0, cols))
    if not np.all(a == np.floor(a)):
        raise ValueError(f"utterance {utterance}: a {kind}'s frames are whole numbers")
    a = a.astype(np.int64)
    prev = 0
    for k, row in enumerate(a):
        b, e = int(row[0]), int(row[1])
        if not 0 <= b <= e <= frames:
            raise ValueError(f"utterance {utterance}, {kind} {k} is frames [{b}, {e}), the utterance has {frames}")
        if b < prev:
            raise ValueError(f"utterance {utterance}, {kind} {k} begins at frame {b}, before the end of the one in front of it ({prev}): "
                             f"the ranges are ascending and disjoint")
        prev = e
    return np.ascontiguousarray(a, dtype=np.int32)


def check_tracks(f0, energy, phoneme_frames, units):
    """The ragged inputs of ``measure_tracks`` -> (frames per utterance, phoneme tables, unit tables), everything that can be refused
    refused: lists of unequal length, tracks of unequal length, an utterance of no frames or of more than MAX_FRAMES, a bad range."""
    B = len(f0)
    if not (len(energy) == len(phoneme_frames) == len(units) == B):
        raise ValueError(f"{B} f0 tracks, {len(energy)} energy tracks, {len(phoneme_frames)} phoneme tables and {len(units)} unit tables: one of each per utterance")
    frames, phones, unit_rows = [], [], []
    for u in range(B):
        T, Te = int(np.shape(f0[u])[0]) if np.ndim(f0[u]) else 1, int(np.shape(energy[u])[0]) if np.ndim(energy[u]) else 1
        if T != Te:
            raise ValueError(f"utterance {u}: {T} f0 values for {Te} energy values")
        if T < 1:
            raise ValueError(f"utterance {u}: no frames - an utterance needs at least one")
        if T > MAX_FRAMES:
            raise ValueError(f"utterance {u}: {T} frames are past the cap of {MAX_FRAMES} ({MAX_FRAMES / FRAME_RATE / 60:.1f} minutes)")
        frames.append(T)
        phones.append(check_ranges(phoneme_frames[u], T, u, "phoneme"))
        unit_rows.append(check_ranges(units[u], T, u, "unit"))
    return frames, phones, unit_rows


def duration_frames(durations, frames):
    """Durations per phoneme -> the cumulative sums [L + 1] clipped to ``frames``: phoneme k is frames [c[k], c[k + 1])."""
    d = durations.detach().cpu().numpy() if torch.is_tensor(durations) else np.asarray(durations)
    d = d.reshape(-1).astype(np.int64)
    if (d < 0).any():
        raise ValueError("a duration is negative")
    return np.minimum(np.concatenate([[0], np.cumsum(d)]), int(frames))


def phoneme_table(feats, cum):
    """int32 [L, 3] = (begin, end, counts for rate) from the features [L, 62] and the clipped cumulative sums of the durations."""
    feats = np.asarray(feats.detach().cpu().numpy() if torch.is_tensor(feats) else feats)
    if feats.shape[0] != len(cum) - 1:
        raise ValueError(f"{len(cum) - 1} durations for {feats.shape[0]} phonemes")
    return np.stack([cum[:-1], cum[1:], (feats[:, prosody.F_PHONEME] != 0).astype(np.int64)], axis=1).astype(np.int32)


def word_units(feats, cum):
    """int32 [words, 2]: ``prosody.word_spans(feats)`` in frames."""
    feats = np.asarray(feats.detach().cpu().numpy() if torch.is_tensor(feats) else feats)
    return np.asarray([(cum[a], cum[b]) for a, b in prosody.word_spans(feats)], dtype=np.int32).reshape(-1, 2)


def to_emphasis(feats, report, n=1, **factors):
    """The ``prosody.Span``s of the n most prominent words of a report whose units are ``prosody.word_spans(feats)`` (the default of
    ``measure``), in the order of the text - ready for ``prosody_curves=``: the emphasis a speaker gave, handed to another voice
    without cloning every duration.  factors: the keywords of ``prosody.emphasis``.  Words without a prominence (no frames) are
    never chosen; equal prominences go to the earlier word."""
    feats = np.asarray(feats.detach().cpu().numpy() if torch.is_tensor(feats) else feats)
    rows = np.asarray(report, dtype=np.float64).reshape(-1, len(COLUMNS))
    words = prosody.word_spans(feats)
    if len(rows) != len(words):
        raise ValueError(f"the report has {len(rows)} rows, the text has {len(words)} words: to_emphasis takes a report on the words")
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError(f"n is a count of words, not {n!r}")
    ranked = sorted((k for k in range(len(rows)) if not math.isnan(rows[k, 0])), key=lambda k: (-rows[k, 0], k))
    return prosody.emphasis(feats, sorted(ranked[:int(n)]), **factors)


class ProminenceMeter:
    """``measure_tracks`` on frame tracks, ``measure`` on waveforms.  extractor: an align.ProsodyExtractor to share the front end
    with (and to align recordings that come without durations); without one the meter builds its own STFT."""

    def __init__(self, device, extractor=None):
        from . import engine
        self.extractor = extractor
        self.ops = extractor.ops if extractor is not None else engine.Ops(device)
        self.ops.small_tile_blocks = 0  # one tile form at every batch size: a wave's spectrum does not depend on its batch (the aligner's own setting)
        self.lib, self.device = self.ops.lib, self.ops.device
        self.max_frames = int(self.lib.tts_prominence_max_frames())
        self.table = torch.from_numpy(wavelet_table()).to(self.device)
        self._logmel = extractor.logmel if extractor is not None else None
        self._tracker = self._resampler = None
        self.last = {}  # what the last measure() fed to measure_tracks (tests, tools)

    def _dev(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    # ---- the three launches on their own ------------------------------------------------------------------------------------
    def channels(self, f0, energy, utts, phones):
        """f0, energy: float32 [total] on the device; utts: int64 [B, 6] and phones: int32 [n, 3] on the host -> x fp64 [3, total]."""
        total = int(f0.numel())
        x = torch.zeros((3, total), dtype=torch.float64, device=self.device)
        utts_d, phones_d = self._dev(utts, np.int64), self._dev(phones.reshape(-1, 3), np.int32)
        capi.check(self.lib.tts_prominence_channels(f0.data_ptr(), energy.data_ptr(), total, utts_d.data_ptr(), utts.ctypes.data, len(utts),
                                                    phones_d.data_ptr() if len(phones) else None, phones.ctypes.data, len(phones), x.data_ptr(),
                                                    self.ops.stream()), "tts_prominence_channels")
        return x

    def cwt(self, x, utts):
        """x fp64 [3, total] -> W fp64 [3, 6, total]."""
        assert x.dtype == torch.float64 and x.dim() == 2 and x.shape[0] == 3 and x.is_contiguous() and x.device == self.device
        total = int(x.shape[1])
        w = torch.zeros((3, N_SCALES, total), dtype=torch.float64, device=self.device)
        utts_d = self._dev(utts, np.int64)
        capi.check(self.lib.tts_prominence_cwt(x.data_ptr(), total, utts_d.data_ptr(), utts.ctypes.data, len(utts), self.table.data_ptr(), w.data_ptr(),
                                               self.ops.stream()), "tts_prominence_cwt")
        return w

    def unit_rows(self, w, utts, units, weights=DEFAULT_WEIGHTS, band=DEFAULT_BAND, with_p=False):
        """W fp64 [3, 6, total] -> (rows fp64 [n_units, 8], P fp64 [total] or None) on the device."""
        assert w.dtype == torch.float64 and w.dim() == 3 and w.shape[:2] == (3, N_SCALES) and w.is_contiguous() and w.device == self.device
        total = int(w.shape[2])
        rows = torch.full((max(len(units), 1), len(COLUMNS)), math.nan, dtype=torch.float64, device=self.device)
        p = torch.zeros(total, dtype=torch.float64, device=self.device) if with_p else None
        utts_d, units_d = self._dev(utts, np.int64), self._dev(units.reshape(-1, 2), np.int32)
        capi.check(self.lib.tts_prominence_units(w.data_ptr(), total, utts_d.data_ptr(), utts.ctypes.data, len(utts),
                                                 units_d.data_ptr() if len(units) else None, units.ctypes.data, len(units), weights[0], weights[1],
                                                 weights[2], band[0], band[1], rows.data_ptr(), None if p is None else p.data_ptr(),
                                                 self.ops.stream()), "tts_prominence_units")
        return rows[:len(units)], p

    @staticmethod
    def layout(frames, phones, units):
        """-> (utts int64 [B, 6], packed phoneme rows int32 [n, 3], packed unit rows int32 [m, 2]) on the host."""
        begin = lambda v: np.concatenate([[0], np.cumsum(v)[:-1]]).astype(np.int64) if len(v) else np.zeros(0, dtype=np.int64)
        nph, nun = [len(p) for p in phones], [len(u) for u in units]
        utts = np.stack([begin(frames), np.asarray(frames, dtype=np.int64), begin(nph), np.asarray(nph, dtype=np.int64), begin(nun),
                         np.asarray(nun, dtype=np.int64)], axis=1).astype(np.int64) if len(frames) else np.zeros((0, 6), dtype=np.int64)
        cat = lambda rows, cols: np.ascontiguousarray(np.concatenate([r.reshape(-1, cols) for r in rows] + [np.zeros((0, cols), dtype=np.int32)]), dtype=np.int32)
        return np.ascontiguousarray(utts), cat(phones, 3), cat(units, 2)

    @torch.inference_mode()
    def measure_tracks(self, f0, energy, phoneme_frames, units, weights=DEFAULT_WEIGHTS, band=DEFAULT_BAND, return_scalogram=False):
        """The low-level ragged call.  Per utterance: f0 (Hz, 0 = unvoiced) and energy (> 0), one value per frame, as arrays or device
        tensors; phoneme_frames [L, 3] = (begin, end, counts for rate) and units [n, 2] = (begin, end) in frames, both ascending and
        disjoint inside the utterance, empty ranges allowed.  weights: (pitch, energy, rate), finite and not negative; band:
        (j_lo, j_hi) of the scales 2^(j + 1) frames.  -> per utterance a float64 [n, 8] array, one row of ``COLUMNS`` per unit; with
        return_scalogram also a list of dicts ``x`` [3, T] (the normalised channels), ``w`` [3, 6, T] and ``p`` [T], float64 arrays.
        Three launches for the batch; ValueError (naming the utterance and the unit) before anything runs."""
        weights, band = check_weights(weights), check_band(band)
        frames, phones, unit_rows = check_tracks(f0, energy, phoneme_frames, units)
        if not frames:
            return ([], []) if return_scalogram else []
        on = lambda tracks: torch.cat([(t.detach() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)))
                                       .to(device=self.device, dtype=torch.float32).reshape(-1) for t in tracks]).contiguous()
        utts, phones_h, units_h = self.layout(frames, phones, unit_rows)
        x = self.channels(on(f0), on(energy), utts, phones_h)
        w = self.cwt(x, utts)
        rows, p = self.unit_rows(w, utts, units_h, weights, band, with_p=return_scalogram)
        rows = rows.cpu().numpy()
        reports = [rows[b:b + n].copy() for b, n in zip(utts[:, 4], utts[:, 5])]
        if not return_scalogram:
            return reports
        x, w, p = x.cpu().numpy(), w.cpu().numpy(), p.cpu().numpy()
        return reports, [{"x": x[:, b:b + T].copy(), "w": w[:, :, b:b + T].copy(), "p": p[b:b + T].copy()} for b, T in zip(utts[:, 0], utts[:, 1])]

    # ---- waves --------------------------------------------------------------------------------------------------------------
    def front_end(self, waves16):
        """Normalised 16 kHz waves -> (f0 tracks laid onto the STFT's frames, energy per frame float32 on the device, the Ragged of the
        frames, the spectrum): the cloner's STFT with tts_frame_energy, and the tracker laid as section 16 lays its f0."""
        from . import align, pitch, style
        if self._logmel is None:
            self._logmel = style.LogMel(self.device)
        if self._tracker is None:
            self._tracker = pitch.PitchTracker(self.device)
        spec, rag = align.batched_spectra(self.ops, self._logmel, waves16)
        energy = torch.empty(rag.total_rows, dtype=torch.float32, device=self.device)
        capi.check(self.lib.tts_frame_energy(spec.data_ptr(), 2 * self._logmel.bins, self._logmel.bins, energy.data_ptr(), rag.total_rows,
                                             self.ops.stream()), "tts_frame_energy")
        f0 = [align.adjust_num_frames_centered(t, n) for t, n in zip(self._tracker.track(waves16), rag.lengths)]
        return f0, energy, rag, spec

    def aligned_durations(self, feats, spec, rag):
        """Durations per phoneme from the extractor's aligner and MAS on the STFT this meter already has."""
        from . import align
        if self.extractor is None:
            raise ValueError("durations=None needs the aligner: make the meter with ProminenceMeter(device, extractor=align.ProsodyExtractor(...))")
        al = self.extractor.aligner
        tok = [align.token_ids(np.asarray(f)) for f in feats]
        x = self.extractor.log_mel(spec, rag)
        dur, begins = al.durations(al.logits(x, rag), rag, [t[0] for t in tok], [t[1] for t in tok])
        dur = dur.cpu().numpy()
        return [dur[b:b + len(t[1])] for b, t in zip(begins, tok)]

    @torch.inference_mode()
    def measure(self, waves, sr, feats, durations=None, units=None, weights=DEFAULT_WEIGHTS, band=DEFAULT_BAND, return_scalogram=False):
        """waves: per utterance a waveform at ``sr`` (one rate or one per wave; several channels are averaged); feats: its [L, 62]
        features.  Every wave goes mono, to 16 kHz on the device and is divided by its peak (compare.waves_to_16k), then through the
        STFT, tts_frame_energy and the pitch tracker: 1 + n // 256 frames.  durations: per utterance one value per phoneme, in
        frames (``tts.last_durations``) - their cumulative sums are clipped to the frames the front end has -, or None: the
        extractor's aligner and MAS provide them.  units: per utterance [n, 2] frame ranges; default: the words
        (``prosody.word_spans(feats)``) mapped through the durations.  -> as ``measure_tracks``.  ValueError for what
        ``waves_to_16k`` refuses (a sample that is not finite, a wave shorter than the tracker's 1200 samples, one past the cap)."""
        from . import compare
        weights, band = check_weights(weights), check_band(band)
        B = len(waves)
        if len(feats) != B or (durations is not None and len(durations) != B) or (units is not None and len(units) != B):
            raise ValueError(f"{B} waves: feats, durations and units hold one entry per wave")
        if B == 0:
            return ([], []) if return_scalogram else []
        srs = [int(s) for s in sr] if isinstance(sr, (list, tuple)) else [int(sr)] * B
        feats = [np.asarray(f.detach().float().cpu().numpy() if torch.is_tensor(f) else f, dtype=np.float32) for f in feats]
        waves16 = compare.waves_to_16k(self, waves, srs, [f"utterance {u}" for u in range(B)], tracked=True)
        f0, energy, rag, spec = self.front_end(waves16)
        if durations is None:
            durations = self.aligned_durations(feats, spec, rag)
        cums = [duration_frames(d, n) for d, n in zip(durations, rag.lengths)]
        phones = [phoneme_table(f, c) for f, c in zip(feats, cums)]
        if units is None:
            units = [word_units(f, c) for f, c in zip(feats, cums)]
        energy_u = [energy[b:b + n] for b, n in zip(rag.begins, rag.lengths)]
        self.last = dict(f0=f0, energy=energy_u, phoneme_frames=phones, units=units, waves16=waves16)
        return self.measure_tracks(f0, energy_u, phones, units, weights, band, return_scalogram)
