"""Pitch tracking on the GPU for the prosody cloner: what the reference gets from Praat (Preprocessing/PitchCalculator.py:64-67,
``snd.to_pitch(time_step=256/16000, pitch_floor=40, pitch_ceiling=600)``) - the autocorrelation method of Boersma (1993) with
Praat's documented defaults - for a ragged batch of normalised 16 kHz waves, on csrc/pitch.hip (include/toucan_pitch.h).

PARITY UNPINNED: the algorithm is restated from its publication and Praat's documentation (DESIGN.md section 12 holds the
definition); parselmouth is not available to compare against, so the yardsticks are the float64 restatement in tests/pitch_ref.py
and the analytic frequency of synthetic signals.  This is why the tracker is opt-in (``f0="track"``, ``track_pitch=True``).

Every launch computes an utterance in an order that depends on that utterance alone: a batch returns bit for bit what its
utterances return one by one.
"""
import numpy as np
import torch

from . import capi, engine

SR, HOP = 16000, 256
N_CAND, N_LAGS, N_WIN, MIN_SAMPLES = capi.PITCH_CANDIDATES, capi.PITCH_LAGS, capi.PITCH_WINDOW, capi.PITCH_MIN_SAMPLES
PATH_ROW = 16  # bytes of back-pointers per frame
TRACK = "track"  # the value of the f0 keyword that asks for the tracker


def frame_count(n):
    """Frames of a wave of n samples: floor((n / 16000 - 0.075) / (256 / 16000)) + 1, in integers."""
    n = int(n)
    if n < MIN_SAMPLES:
        raise ValueError(f"a wave of {n} samples is shorter than the analysis window (three periods of 40 Hz: {MIN_SAMPLES} samples)")
    return (n - MIN_SAMPLES) // HOP + 1


def frame_times(n):
    """Centre of every frame in seconds: t = 0.5 n dx - 0.5 nfr dt + 0.5 dt + f dt."""
    nfr = frame_count(n)
    dx, dt = 1.0 / SR, HOP / SR
    return 0.5 * n * dx - 0.5 * nfr * dt + 0.5 * dt + np.arange(nfr) * dt


def window_tables():
    """(win [1198] float32, wr [600] float64): the Hanning window win[j] = 0.5 - 0.5 cos(2 pi (j + 1) / (nw + 1)) and its
    autocorrelation normalised to wr[0] = 1, both computed in float64."""
    j = np.arange(N_WIN, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * (j + 1.0) / (N_WIN + 1.0))
    wr = np.correlate(np.concatenate([win, np.zeros(N_LAGS - 1)]), win, "valid")
    return win.astype(np.float32), wr / wr[0]


class PitchTracker:
    """``track(waves16)``: f0 per frame (Hz, 0 = voiceless) for every wave of a ragged batch."""

    def __init__(self, device):
        self.ops = engine.Ops(device)
        self.device = self.ops.device
        win, wr = window_tables()
        self.win = torch.from_numpy(win).to(self.device)
        self.wr = torch.from_numpy(wr).to(self.device)

    def layout(self, waves16):
        """The packed batch on the device: the waves end to end, where each begins, its samples and frames, and the rows of its
        frames in the per-frame arrays."""
        waves = [np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1)) for w in waves16]
        n = [len(w) for w in waves]
        frames = [frame_count(k) for k in n]
        assert sum(n) < 2 ** 31, "a batch holds fewer than 2^31 samples"
        ti = lambda a, dt=np.int32: torch.from_numpy(np.asarray(a, dtype=dt)).to(self.device)
        begins = lambda v: np.concatenate([[0], np.cumsum(v)[:-1]])
        return {"n": n, "frames": frames, "frame_begin": [int(b) for b in begins(frames)], "rows": int(sum(frames)),
                "wave": torch.from_numpy(np.concatenate(waves)).to(self.device), "wave_begin": ti(begins(n)), "n_samples": ti(n),
                "frame_begin_d": ti(begins(frames)), "n_frames": ti(frames)}

    def candidates(self, lay, with_r=False):
        """-> (freq [rows, 15], strength [rows, 15], n_cand [rows], r [rows, 600] or None) on the device."""
        ops, B, rows = self.ops, len(lay["n"]), lay["rows"]
        stats = ops.empty(B, 2)
        capi.check(ops.lib.tts_wave_stats(lay["wave"].data_ptr(), lay["wave_begin"].data_ptr(), lay["n_samples"].data_ptr(), B, stats.data_ptr(),
                                          ops.stream()), "tts_wave_stats")
        freq, strength = ops.empty(rows, N_CAND), ops.empty(rows, N_CAND)
        n_cand = ops.empty(rows, dtype=torch.int32)
        r = ops.empty(rows, N_LAGS) if with_r else None
        capi.check(ops.lib.tts_pitch_candidates(lay["wave"].data_ptr(), lay["wave_begin"].data_ptr(), lay["n_samples"].data_ptr(), stats.data_ptr(),
                                                lay["frame_begin_d"].data_ptr(), lay["n_frames"].data_ptr(), B, max(lay["frames"]),
                                                self.win.data_ptr(), self.wr.data_ptr(), freq.data_ptr(), strength.data_ptr(), n_cand.data_ptr(),
                                                None if r is None else r.data_ptr(), ops.stream()), "tts_pitch_candidates")
        return freq, strength, n_cand, r

    def path(self, freq, strength, n_cand, frames, force_scratch=False):
        """Candidates [rows, 15] of utterances with `frames` frames each (packed) -> f0 [rows] on the device."""
        ops, B = self.ops, len(frames)
        ti = lambda a, dt=np.int32: torch.from_numpy(np.asarray(a, dtype=dt)).to(self.device)
        off, total = np.full(B, -1, dtype=np.int64), 0
        for b, T in enumerate(frames):
            if force_scratch or T > capi.PITCH_PATH_LDS_FRAMES:
                off[b], total = total, total + T * PATH_ROW
        lds_frames = 0 if force_scratch else min(capi.PITCH_PATH_LDS_FRAMES, max(frames))
        scratch = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        fb, nf, offd = ti(np.concatenate([[0], np.cumsum(frames)[:-1]])), ti(frames), ti(off, np.int64)
        f0 = ops.empty(int(sum(frames)))
        capi.check(ops.lib.tts_pitch_path(freq.data_ptr(), strength.data_ptr(), n_cand.data_ptr(), fb.data_ptr(), nf.data_ptr(), offd.data_ptr(),
                                          scratch.data_ptr(), B, lds_frames, f0.data_ptr(), ops.stream()), "tts_pitch_path")
        return f0

    @torch.inference_mode()
    def track(self, waves16, force_scratch=False):
        """waves16: normalised mono waves at 16 kHz, at least 1200 samples each (ValueError otherwise, as Praat refuses them).
        -> list of float32 arrays, one f0 value (Hz, 0 = voiceless) per frame of ``frame_times(len(wave))``."""
        if len(waves16) == 0:
            return []
        lay = self.layout(waves16)
        freq, strength, n_cand, _ = self.candidates(lay)
        f0 = self.path(freq, strength, n_cand, lay["frames"], force_scratch).cpu().numpy()
        if (f0 < 0).any():
            raise capi.ToucanHipError("tts_pitch_path reported an utterance it could not lay out")
        return [f0[b:b + T].copy() for b, T in zip(lay["frame_begin"], lay["frames"])]
