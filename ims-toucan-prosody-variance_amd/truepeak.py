"""What a delivery specification asks of a waveform beyond its integrated loudness, on the GPU (csrc/truepeak.hip,
include/toucan_truepeak.h) for a ragged batch: the true peak after ITU-R BS.1770-4 Annex 2 (the utterance oversampled 4x by the
resampler's own interpolator, never written to memory), the largest short-term loudness and the loudness range after EBU Tech
3341 / 3342 (3 s blocks every 100 ms from the loudness meter's segment energies, gates at -70 LUFS and 20 LU below the mean, the
10th and 95th percentile by an exact selection), the one gain per utterance that brings it to a target loudness with the TRUE
peak under a ceiling as well as the sample peak, and - opt-in - a look-ahead limiter for the utterances whose peaks keep that gain
from reaching the target.  include/toucan_truepeak.h holds the definition, DESIGN.md section 20 the
decisions, tests/truepeak_ref.py the float64 restatement.

A batch returns bit for bit what its utterances return alone: every oversampled value is one fixed chain, maxima and counts do not
depend on order, sums run in index order per utterance.
"""
import math

import numpy as np
import torch

from . import capi, resample, segments
from .loudness import LoudnessMeter
from .segments import SegmentMeter, segment_samples

DELIVERY_COLUMNS = ("true_peak", "true_peak_dbtp", "sample_peak", "short_term_max_lufs", "lra", "lra_low_lufs", "lra_high_lufs", "short_term_kept")
# the rows as tts_loudness_range writes them: the eight above, then what the tests pin the selection with
RANGE_COLUMNS = DELIVERY_COLUMNS + ("short_term_blocks", "short_term_abs", "lra_low_z", "lra_high_z")
# the rows of tts_limit_true_peak: the gain in front of the limiter, the ceiling as a factor, the larger of true peak and sample peak
# before the trim and how far over the ceiling it was, whether the trim was applied, the window in samples, the trim and the trim in dB
LIMITER_COLUMNS = ("g0", "ceiling", "peak_before_trim", "over_db", "trimmed", "window", "trim", "trim_db")


def oversampling(sr):
    """F: 4 below 96 kHz, 2 below 192 kHz, 1 at 192 kHz (BS.1770-4 Annex 2)."""
    segment_samples(sr)
    return 4 if sr < 96000 else 2 if sr < 192000 else 1


def interpolator(sr):
    """(F, w, table float32 [F, K]): the resampler's table for sr -> F sr; w = 7 and K = 15 for F > 1, [[1]] for F = 1."""
    F = oversampling(sr)
    orig, new, w, table = resample.kernel_table(int(sr), F * int(sr))
    assert (orig, new) == (1, F) and table.shape == (F, 2 * w + 1) and w == (capi.TRUEPEAK_HALF_WIDTH if F > 1 else 0)
    return F, w, table


def kernel_table(sr):
    """float32 [K, F]: the transposed layout the kernels read."""
    return np.ascontiguousarray(interpolator(sr)[2].T)


def check_ceiling(true_peak_ceiling_dbtp):
    v = true_peak_ceiling_dbtp
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"the true-peak ceiling must be a finite number, not {v!r}")
    if v > 0:
        raise ValueError(f"the true-peak ceiling {v!r} dBTP is above full scale (0 dBTP)")


class DeliveryMeter(SegmentMeter):
    """``measure(packed_wave, spans, sr)`` and ``normalize(packed_wave, spans, sr, target_lufs, peak_ceiling_dbfs,
    true_peak_ceiling_dbtp, limiter)`` for a ragged batch on the device.  ``loudness_meter``: a LoudnessMeter of the same device to borrow
    for the segment energies (its own otherwise).  ``last_range``: float64 [B, 12] on the device (``RANGE_COLUMNS``) and
    ``last_steps``: int32 [B], the steps the gain of the last ``normalize`` took towards zero."""

    def __init__(self, device, loudness_meter=None):
        super().__init__(device, "delivery meter", kernel_table, "tts_truepeak_tile_samples")
        self.tile_samples = self.tile_segments
        self.loudness = loudness_meter if loudness_meter is not None else LoudnessMeter(self.device)
        assert self.loudness.device == self.device
        self.last_range = self.last_steps = self.last_limiter = self.last_limiter_gain = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _true_peak(self, wave, rows, rows_d, sr, loudness_stats=None):
        """float32 [B]: the true peak of every utterance, scaled by the gain of its loudness row where rows are given."""
        tp = torch.empty(len(rows), dtype=torch.float32, device=self.device)
        if len(rows):
            capi.check(self.lib.tts_true_peak(wave.data_ptr(), wave.numel(), rows_d.data_ptr(), rows.ctypes.data, len(rows), int(rows[:, 1].max()),
                                              self.table(sr).data_ptr(), oversampling(sr), None if loudness_stats is None else loudness_stats.data_ptr(),
                                              tp.data_ptr(), self._stream()), "tts_true_peak")
        return tp

    def _measure(self, wave, rows, rows_d, sr, gate=False):
        """energies + true peak + range on the current stream -> rows [B, 12] float64 on the device; with ``gate`` also the
        loudness rows [B, 8] of the same energies (measured only: gain 1)."""
        S, B = segment_samples(sr), len(rows)
        stats = torch.empty((B, len(RANGE_COLUMNS)), dtype=torch.float64, device=self.device)
        gated = torch.empty((B, capi.LOUDNESS_N_COLUMNS), dtype=torch.float64, device=self.device) if gate else None
        self.last_range = stats
        if B == 0:
            return (stats, gated) if gate else stats
        max_segments = self._max_segments(rows, S)
        state = torch.empty((B, max_segments, 4), dtype=torch.float64, device=self.device)
        energy = torch.empty((B, max_segments), dtype=torch.float64, device=self.device)
        peak = torch.empty((B, max_segments), dtype=torch.float32, device=self.device)
        capi.check(self.lib.tts_kweight_energy(wave.data_ptr(), wave.numel(), rows_d.data_ptr(), rows.ctypes.data, B, S,
                                               self.loudness.table(sr).data_ptr(), max_segments, state.data_ptr(), energy.data_ptr(), peak.data_ptr(),
                                               self._stream()), "tts_kweight_energy")
        tp = self._true_peak(wave, rows, rows_d, sr)
        capi.check(self.lib.tts_loudness_range(energy.data_ptr(), peak.data_ptr(), tp.data_ptr(), wave.numel(), rows_d.data_ptr(), B, S, max_segments,
                                               None, stats.data_ptr(), self._stream()), "tts_loudness_range")
        if gate:
            capi.check(self.lib.tts_loudness_gate(energy.data_ptr(), peak.data_ptr(), wave.numel(), rows_d.data_ptr(), B, S, max_segments,
                                                  float("nan"), 0.0, gated.data_ptr(), self._stream()), "tts_loudness_gate")
        self.last_segments = (energy, peak)
        return (stats, gated) if gate else stats

    @torch.inference_mode()
    def measure(self, packed_wave, spans, sr):
        """packed_wave: float32 [N] on the device; spans: [(first sample, sample count)] per utterance -> float64 [B, 8] on the
        device, columns ``DELIVERY_COLUMNS``.  On the current stream, without a synchronisation."""
        segment_samples(sr)
        rows, rows_d = self._rows(packed_wave, spans)
        return self._measure(packed_wave, rows, rows_d, sr)[:, :len(DELIVERY_COLUMNS)]

    def _out_like(self, packed_wave, rows, out):
        """``out`` as the meters' normalize takes it, for a kernel that writes the spans only."""
        if out is None:
            tiled = len(rows) > 0 and int(rows[0, 0]) == 0 and int(rows[-1].sum()) == packed_wave.numel() and \
                bool((rows[1:, 0] == rows[:-1].sum(axis=1)).all())
            out = torch.empty_like(packed_wave) if tiled else packed_wave.clone()
        assert out.dtype == torch.float32 and out.shape == packed_wave.shape and out.device == self.device and out.is_contiguous()
        return out

    @torch.inference_mode()
    def normalize(self, packed_wave, spans, sr, target_lufs=-23.0, peak_ceiling_dbfs=-1.0, true_peak_ceiling_dbtp=-1.0, limiter=False, out=None):
        """-> (wave, loudness_stats [B, 8], delivery_stats [B, 8]).  Without ``limiter``: every utterance times the one float32
        gain that brings its integrated loudness to ``target_lufs``, or as close as the sample-peak ceiling and the true-peak
        ceiling allow - the meter's own reading of the result is at or under ``true_peak_ceiling_dbtp``.  With ``limiter``: every
        utterance times the gain to the target, whatever its peaks, then through a look-ahead limiter (2 ms, feed-forward) that
        holds samples and true peak under the lower of the two ceilings; the loudness reached is measured again.  An utterance
        without a loudness keeps its bits either way.  ``out`` as ``LoudnessMeter.normalize`` takes it.  loudness_stats:
        ``loudness.LOUDNESS_COLUMNS`` - the gain applied (with ``limiter``: the gain in front of the limiter) and the loudness
        reached; delivery_stats: ``DELIVERY_COLUMNS`` of the OUTPUT.  ``last_steps`` (pure gain) or ``last_limiter`` (float64
        [B, 8], ``LIMITER_COLUMNS``; ``last_limiter_gain`` the per-sample gain) tell what it took.  Nothing returns to the host in
        between."""
        segment_samples(sr)
        segments.check_target("loudness", target_lufs, peak_ceiling_dbfs)
        check_ceiling(true_peak_ceiling_dbtp)
        rows, rows_d = self._rows(packed_wave, spans)
        B, F = len(rows), oversampling(sr)
        stats = self.loudness._measure(packed_wave, rows, rows_d, sr, target_lufs, peak_ceiling_dbfs)
        if not limiter:
            self.last_steps = torch.zeros(B, dtype=torch.int32, device=self.device)
            if B:
                tp = self._true_peak(packed_wave, rows, rows_d, sr)
                work = torch.empty((2, B), dtype=torch.int32, device=self.device)
                capi.check(self.lib.tts_truepeak_gain(packed_wave.data_ptr(), packed_wave.numel(), rows_d.data_ptr(), rows.ctypes.data, B,
                                                      self.table(sr).data_ptr(), F, tp.data_ptr(), float(true_peak_ceiling_dbtp),
                                                      stats.data_ptr(), self.last_steps.data_ptr(), work.data_ptr(), self._stream()), "tts_truepeak_gain")
            y = self._apply_gain(packed_wave, rows, rows_d, stats, out)
            return y, stats, self._measure(y, rows, rows_d, sr)[:, :len(DELIVERY_COLUMNS)]
        y = self._out_like(packed_wave, rows, out)
        self.last_limiter = torch.empty((B, len(LIMITER_COLUMNS)), dtype=torch.float64, device=self.device)
        m = torch.empty_like(packed_wave)
        self.last_limiter_gain = torch.ones(packed_wave.shape, dtype=torch.float64, device=self.device)
        if B == 0:
            return y, stats, self._measure(y, rows, rows_d, sr)[:, :len(DELIVERY_COLUMNS)]
        tp = torch.empty(B, dtype=torch.float32, device=self.device)
        capi.check(self.lib.tts_limit_true_peak(packed_wave.data_ptr(), packed_wave.numel(), rows_d.data_ptr(), rows.ctypes.data, B, int(rows[:, 1].max()),
                                                segment_samples(sr), self.table(sr).data_ptr(), F, stats.data_ptr(), float(target_lufs),
                                                float(peak_ceiling_dbfs), float(true_peak_ceiling_dbtp), m.data_ptr(), self.last_limiter_gain.data_ptr(),
                                                tp.data_ptr(), self.last_limiter.data_ptr(), y.data_ptr(), self._stream()), "tts_limit_true_peak")
        delivery, after = self._measure(y, rows, rows_d, sr, gate=True)
        stats[:, 6] = self.last_limiter[:, 0]
        stats[:, 7] = after[:, 0]
        return y, stats, delivery[:, :len(DELIVERY_COLUMNS)]
