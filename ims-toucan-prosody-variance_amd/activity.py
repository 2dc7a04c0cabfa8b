"""Where the speech in a waveform is, on the GPU (csrc/activity.hip, include/toucan_activity.h): the active speech level of ITU-T
Recommendation P.56, method B, for a ragged batch of waveforms - a two-stage exponential envelope, a ladder of thresholds 6.02 dB
apart with a 200 ms hangover, the level read where it stands 15.9 dB above its threshold - and, from the envelope against that
final threshold, the runs of speech, their bounds and the pauses between them; then one gain per utterance that brings the active
level to a target (-26 dB re full scale is the convention of listening tests), limited by a SAMPLE-peak ceiling.
include/toucan_activity.h holds the definition, DESIGN.md section 18 the decisions, tests/activity_ref.py the float64 restatement.

The method is restated from its publication.  Agreement with the ITU Software Tool Library's sv56 is unpinned: nobody has measured
it (sv56 bisects where the Recommendation's text, and this module, interpolate linearly in dB).  It is no silero either: it is the
substitute for the voice-activity trim of the reference that needs no model.

Everything is fp64 in a fixed order per utterance: a batch returns bit for bit what its utterances return alone.
"""
import math

import numpy as np
import torch

from . import capi, segments
from .segments import SegmentMeter, segment_samples

ACTIVITY_COLUMNS = ("active_db", "long_term_db", "activity", "threshold_db", "speech_begin", "speech_end", "gain", "active_db_after")
MIN_RATE, MAX_RATE = capi.ACTIVITY_MIN_RATE, capi.ACTIVITY_MAX_RATE
THRESHOLDS = capi.ACTIVITY_THRESHOLDS
TIME_CONSTANT, MARGIN_DB = 0.03, 15.9
DEFAULT_LEAD_MS = 30  # silero's speech_pad_ms: the envelope crosses the threshold about 20 ms after an onset


def coefficient(sr):
    """g = exp(-1 / (0.03 sr)) of both envelope stages.  ValueError for a rate the meter does not take (the loudness meter's rule)."""
    return math.exp(-1.0 / (TIME_CONSTANT * segment_samples(sr) * 10))


def transition(sr):
    """T, float64 [2, 2]: the zero-input transition of the envelope's state (p, q) over one segment - column i is the state
    ``sr / 10`` samples after the unit state i, by the recurrence run on x = 0."""
    g = coefficient(sr)
    h = 1.0 - g
    p, q = np.array([1.0, 0.0]), np.array([0.0, 1.0])  # the two unit states side by side
    for _ in range(segment_samples(sr)):
        p = g * p
        q = g * q + h * p
    return np.stack([p, q])


def kernel_table(sr):
    """float64 [6]: what tts_activity_envelope reads - g, h = 1 - g, T row-major."""
    g = coefficient(sr)
    return np.concatenate([[g, 1.0 - g], transition(sr).reshape(-1)])


def check_target(target_db, peak_ceiling_dbfs):
    segments.check_target("speech level", target_db, peak_ceiling_dbfs)


def bounds(stats, lead):
    """Host helper.  stats: [B, 8] (tensor or array, ``ACTIVITY_COLUMNS``) -> per utterance ``(max(0, speech_begin - lead),
    speech_end)`` in samples, or None for an utterance without speech.  ``lead`` (samples) answers the envelope's rise time: the
    threshold is crossed about 20 ms after an onset, so the begin is moved back; nothing is added at the end (the envelope falls
    under the threshold about 100 ms after an offset)."""
    rows = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    lead = int(lead)
    if lead < 0:
        raise ValueError(f"the lead {lead} is negative")
    out = []
    for row in rows.reshape(-1, len(ACTIVITY_COLUMNS)):
        b, e = int(row[4]), int(row[5])
        out.append((max(0, b - lead), e) if e > b else None)
    return out


def pauses(runs, count):
    """Host helper.  runs: [R, 2] (begin, end) of one utterance, ``count`` of them valid -> the gaps between consecutive runs as
    [(begin, end)]."""
    rows = runs.detach().cpu().numpy() if isinstance(runs, torch.Tensor) else np.asarray(runs)
    rows = rows.reshape(-1, 2)[:min(int(count), len(rows))]
    return [(int(rows[i][1]), int(rows[i + 1][0])) for i in range(len(rows) - 1)]


class SpeechActivity(SegmentMeter):
    """``measure(packed_wave, spans, sr)`` and ``normalize(packed_wave, spans, sr, target_db, peak_ceiling_dbfs)`` for a ragged
    batch on the device.  The tables (g, h and T) are uploaded once per rate and kept.  Of the last call: ``last_counts`` int64
    [B, 16] (a_0 .. a_14, the number of runs), ``last_runs`` int64 [B, max_runs, 2] (rows past the count hold 0), ``last_sums``
    float64 [B, 2] (sum of x^2, max |x|), ``last_states`` float64 [B, most segments, 2] (p, q at every segment's start)."""

    def __init__(self, device):
        super().__init__(device, "speech-activity meter", kernel_table, "tts_activity_tile_segments")
        self.last_counts = self.last_runs = self.last_sums = self.last_states = None

    def _measure(self, wave, rows, rows_d, sr, target, ceiling, max_runs, level_only=False):
        """The five passes on the current stream -> stats [B, 8] float64 on the device.  ``level_only``: passes 1 to 4 alone, and
        the ``last_*`` of the call before stay."""
        S, B, max_runs = segment_samples(sr), len(rows), int(max_runs)
        if max_runs < 0:
            raise ValueError(f"max_runs {max_runs} is negative")
        dev = self.device
        stats = torch.empty((B, len(ACTIVITY_COLUMNS)), dtype=torch.float64, device=dev)
        max_segments = self._max_segments(rows, S)
        counts = torch.zeros((B, capi.ACTIVITY_COUNTS), dtype=torch.int64, device=dev)
        runs = torch.zeros((B, max_runs, 2), dtype=torch.int64, device=dev)
        sums = torch.zeros((B, 2), dtype=torch.float64, device=dev)
        state = torch.zeros((B, max_segments, 2), dtype=torch.float64, device=dev)
        if not level_only:
            self.last_counts, self.last_runs, self.last_sums, self.last_states = counts, runs, sums, state
        if B == 0:
            return stats
        sq = torch.empty((B, max_segments), dtype=torch.float64, device=dev)
        peak = torch.empty((B, max_segments), dtype=torch.float32, device=dev)
        pos = torch.empty((B, max_segments, 16, 2), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        n, table = wave.numel(), self.table(sr).data_ptr()
        capi.check(self.lib.tts_activity_envelope(wave.data_ptr(), n, rows_d.data_ptr(), rows.ctypes.data, B, S, table, max_segments,
                                                  state.data_ptr(), sq.data_ptr(), peak.data_ptr(), pos.data_ptr(), st), "tts_activity_envelope")
        capi.check(self.lib.tts_activity_level(sq.data_ptr(), peak.data_ptr(), pos.data_ptr(), n, rows_d.data_ptr(), B, S, max_segments,
                                               float(target), float(ceiling), counts.data_ptr(), sums.data_ptr(), stats.data_ptr(), st),
                   "tts_activity_level")
        if level_only:
            return stats
        capi.check(self.lib.tts_activity_runs(wave.data_ptr(), n, rows_d.data_ptr(), rows.ctypes.data, B, S, table, max_segments,
                                              state.data_ptr(), pos.data_ptr(), max_runs, runs.data_ptr() if max_runs else None,
                                              counts.data_ptr(), stats.data_ptr(), st), "tts_activity_runs")
        return stats

    @torch.inference_mode()
    def measure(self, packed_wave, spans, sr, max_runs=64):
        """packed_wave: float32 [N] on the device; spans: [(first sample, sample count)] per utterance -> float64 [B, 8] on the
        device, columns ``ACTIVITY_COLUMNS`` (gain = 1, active_db_after = active_db).  ``last_runs`` keeps the first ``max_runs``
        runs of every utterance, ``last_counts[:, 15]`` their true number.  On the current stream, without a synchronisation."""
        segment_samples(sr)
        rows, rows_d = self._rows(packed_wave, spans)
        return self._measure(packed_wave, rows, rows_d, sr, float("nan"), 0.0, max_runs)

    @torch.inference_mode()
    def normalize(self, packed_wave, spans, sr, target_db=-26.0, peak_ceiling_dbfs=-1.0, out=None, max_runs=64):
        """-> (wave, stats): every utterance times the one float32 gain that brings its active speech level to ``target_db``, or
        as close as the sample-peak ceiling allows; an utterance without a level (nothing, silence, or an envelope that never
        reaches the lowest threshold) keeps its bits.  ``out``: None for a new tensor (samples outside every span are copied),
        ``packed_wave`` itself for in place, or another float32 tensor of its length, of which only the spans are written.  The
        gain is applied by the loudness meter's gain kernel, from the device row: nothing returns to the host in between.
        ``active_db_after`` is the level of the scaled wave MEASURED again (passes 1 to 4 on the output), not active_db +
        20 log10 gain: the ladder of thresholds stays where it is when the signal is scaled, so the method follows a gain that is
        no power of two only to its interpolation error (hundredths of a dB on speech, more where few thresholds are reached).
        The bounds, runs and counts are those of the input wave."""
        segment_samples(sr)
        check_target(target_db, peak_ceiling_dbfs)
        rows, rows_d = self._rows(packed_wave, spans)
        stats = self._measure(packed_wave, rows, rows_d, sr, target_db, peak_ceiling_dbfs, max_runs)
        out = self._apply_gain(packed_wave, rows, rows_d, stats, out)
        if len(rows):
            again = self._measure(out, rows, rows_d, sr, float("nan"), 0.0, 0, level_only=True)
            stats[:, ACTIVITY_COLUMNS.index("active_db_after")] = again[:, 0]
        return out, stats
