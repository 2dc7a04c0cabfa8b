"""Integrated loudness after ITU-R BS.1770-4 and loudness normalisation on the GPU (csrc/loudness.hip, include/toucan_loudness.h)
for a ragged batch of waveforms: K-weighting, 400 ms blocks with 75 % overlap, the absolute gate at -70 LUFS and the relative gate
10 LU below the mean of what the absolute gate keeps; then one gain per utterance that brings it to a target, limited by a
SAMPLE-peak ceiling (max |x|; not a 4x oversampled true peak: truepeak.py has that one, as ``true_peak_ceiling=`` /
``limiter=`` beside ``loudness=``).  include/toucan_loudness.h holds the definition, DESIGN.md section
17 the decisions, tests/loudness_ref.py the float64 restatement.

The coefficients are the bilinear transforms of the analogue prototypes, in float64 on the host once per rate; at 48 kHz they are
the table printed in BS.1770-4 and a full-scale 997 Hz sine reads -3.01 LKFS.  Everything is fp64 in a fixed order per utterance:
a batch returns bit for bit what its utterances return alone.
"""
import math

import numpy as np
import torch

from . import capi, segments
from .segments import MAX_RATE, MIN_RATE, SegmentMeter, segment_samples  # noqa: F401  (the rates are part of this module's surface)

LOUDNESS_COLUMNS = ("lufs", "peak", "blocks", "blocks_abs", "blocks_both", "momentary_max_lufs", "gain", "lufs_after")

SHELF_F0, SHELF_GAIN_DB, SHELF_Q, SHELF_VB_EXPONENT = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773


def k_weighting(sr):
    """((b, a), (b, a)): the shelf and the high-pass of the K-weighting at ``sr``, float64 arrays of three."""
    segment_samples(sr)
    K = math.tan(math.pi * SHELF_F0 / sr)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXPONENT
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = (np.array([(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]))
    K = math.tan(math.pi * HIGHPASS_F0 / sr)
    d = 1.0 + K / HIGHPASS_Q + K * K
    high = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / HIGHPASS_Q + K * K) / d]))
    return shelf, high


def transition(sr):
    """M, float64 [4, 4]: the zero-input transition of the cascade's state (s1, s2, s3, s4; direct form II transposed) over one
    segment - column i is the state ``sr / 10`` samples after the unit state i, by the recurrence run on x = 0."""
    (b, a), (_, c) = k_weighting(sr)
    s1, s2, s3, s4 = (np.eye(4)[i].copy() for i in range(4))  # the four unit states side by side
    for _ in range(segment_samples(sr)):
        y1 = s1
        s1, s2 = s2 - a[1] * y1, -a[2] * y1
        y2 = y1 + s3
        s3, s4 = (s4 - 2.0 * y1) - c[1] * y2, y1 - c[2] * y2
    return np.stack([s1, s2, s3, s4])


def kernel_table(sr):
    """float64 [24]: what tts_kweight_energy reads - shelf b0 b1 b2 a1 a2, high-pass a1 a2, 0, M row-major."""
    (b, a), (_, c) = k_weighting(sr)
    return np.concatenate([b, a[1:], c[1:], [0.0], transition(sr).reshape(-1)])


def check_target(target_lufs, peak_ceiling_dbfs):
    segments.check_target("loudness", target_lufs, peak_ceiling_dbfs)


class LoudnessMeter(SegmentMeter):
    """``measure(packed_wave, spans, sr)`` and ``normalize(packed_wave, spans, sr, target_lufs, peak_ceiling_dbfs)`` for a ragged
    batch on the device.  The tables (coefficients and M) are uploaded once per rate and kept.  ``last_segments``: (e_k float64,
    max |x| float32), each [B, most segments of an utterance] on the device, of the last call."""

    def __init__(self, device):
        super().__init__(device, "loudness meter", kernel_table, "tts_loudness_tile_segments")

    def _measure(self, wave, rows, rows_d, sr, target, ceiling):
        """kweight + gate on the current stream -> stats [B, 8] float64 on the device."""
        S, B = segment_samples(sr), len(rows)
        stats = torch.empty((B, len(LOUDNESS_COLUMNS)), dtype=torch.float64, device=self.device)
        if B == 0:
            return stats
        max_segments = self._max_segments(rows, S)
        state = torch.empty((B, max_segments, 4), dtype=torch.float64, device=self.device)
        energy = torch.empty((B, max_segments), dtype=torch.float64, device=self.device)
        peak = torch.empty((B, max_segments), dtype=torch.float32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.tts_kweight_energy(wave.data_ptr(), wave.numel(), rows_d.data_ptr(), rows.ctypes.data, B, S, self.table(sr).data_ptr(),
                                               max_segments, state.data_ptr(), energy.data_ptr(), peak.data_ptr(), st), "tts_kweight_energy")
        capi.check(self.lib.tts_loudness_gate(energy.data_ptr(), peak.data_ptr(), wave.numel(), rows_d.data_ptr(), B, S, max_segments,
                                              float(target), float(ceiling), stats.data_ptr(), st), "tts_loudness_gate")
        self.last_segments = (energy, peak)  # [B, max_segments] each: e_k and max |x| per segment of the last call
        return stats

    @torch.inference_mode()
    def measure(self, packed_wave, spans, sr):
        """packed_wave: float32 [N] on the device; spans: [(first sample, sample count)] per utterance -> float64 [B, 8] on the
        device, columns ``LOUDNESS_COLUMNS`` (gain = 1, lufs_after = lufs).  On the current stream, without a synchronisation."""
        segment_samples(sr)
        rows, rows_d = self._rows(packed_wave, spans)
        return self._measure(packed_wave, rows, rows_d, sr, float("nan"), 0.0)

    @torch.inference_mode()
    def normalize(self, packed_wave, spans, sr, target_lufs=-23.0, peak_ceiling_dbfs=-1.0, out=None):
        """-> (wave, stats): every utterance times the one float32 gain that brings its integrated loudness to ``target_lufs``, or
        as close as the sample-peak ceiling allows; an utterance without a loudness (shorter than 400 ms, or nothing above
        -70 LUFS) keeps its bits.  ``out``: None for a new tensor (samples outside every span are copied), ``packed_wave`` itself
        for in place, or another float32 tensor of its length, of which only the spans are written.  stats as ``measure``
        returns them, with the gain applied and the loudness reached.  Nothing returns to the host in between."""
        segment_samples(sr)
        check_target(target_lufs, peak_ceiling_dbfs)
        rows, rows_d = self._rows(packed_wave, spans)
        stats = self._measure(packed_wave, rows, rows_d, sr, target_lufs, peak_ceiling_dbfs)
        return self._apply_gain(packed_wave, rows, rows_d, stats, out), stats
