"""How intelligible a generated waveform is next to the recording it is time-aligned with, on the GPU (csrc/intelligibility.hip,
include/toucan_intelligibility.h) for ragged batches of pairs: STOI (Taal et al. 2011) and ESTOI (Jensen and Taal 2016), restated
from the two publications - parity with any toolkit is not pinned.  include/toucan_intelligibility.h holds the definition,
DESIGN.md section 23 the decisions, tests/intelligibility_ref.py the float64 restatement.

Both signals go to 10 kHz (resample.Resampler) and are cut to the shorter.  The frames of the recording quieter than 40 dB under
its loudest are dropped from both (tts_stoi_frame_energy, tts_stoi_select); the windowed frames of the two compacted signals are
written from the wave and the kept list alone (tts_stoi_gather), go through the fp32 DFT conv that fidelity.py uses, become 15
band values a frame in fp64 (tts_stoi_bands) and one STOI and one ESTOI value per segment of 30 frames (tts_stoi_segments), whose
means are the measures (tts_stoi_reduce).  Nothing comes to the host before the end; a batch returns bit for bit what its pairs
return alone.
"""
import math

import numpy as np
import torch

from . import capi, engine, packing, resample
from .capi import MODE_LINEAR
from .ragged import Ragged

SR = capi.STOI_RATE
N_FRAME, HOP, N_BINS, N_BANDS, SEGMENT = capi.STOI_FRAME, capi.STOI_HOP, capi.STOI_BINS, capi.STOI_BANDS, capi.STOI_SEGMENT
BANDS = tuple(zip(capi.STOI_BAND_EDGES[:-1], capi.STOI_BAND_EDGES[1:]))


def band_table(sr=SR, n_fft=2 * N_FRAME, n_bands=N_BANDS, first_centre=150.0):
    """The one-third-octave bands as (first bin, bin past the last): every edge at the nearest bin frequency."""
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
    centres = first_centre * 2.0 ** (np.arange(n_bands) / 3.0)
    return tuple((int(np.argmin(np.abs(f - c * 2.0 ** (-1.0 / 6.0)))), int(np.argmin(np.abs(f - c * 2.0 ** (1.0 / 6.0))))) for c in centres)


def window():
    """float32 [256]: the 258-point Hann window without its zero end points, computed in float64 and rounded once."""
    i = np.arange(N_FRAME, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * (i + 1.0) / (N_FRAME + 1.0)))).astype(np.float32)


def dft_basis():
    """float32 [1, 256, 514]: [cos | -sin] of the 512-point DFT for the 256 samples of a frame that are not padding (the window is
    in the rows already)."""
    ang = 2.0 * np.pi * np.outer(np.arange(N_FRAME, dtype=np.float64), np.arange(N_BINS, dtype=np.float64)) / (2 * N_FRAME)
    return np.concatenate([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)[None]


def frame_count(n):
    return (int(n) - N_FRAME) // HOP + 1 if n >= N_FRAME else 0


def _wave_on(device, w):
    if torch.is_tensor(w):
        t = w.detach()
    else:
        a = np.asarray(w)
        if a.ndim == 2:
            a = a.mean(axis=1)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(device=device, dtype=torch.float32).reshape(-1).contiguous()


class Intelligibility:
    """``score(recordings, generated, sr)`` for ragged lists of waveforms, ``score_packed`` for a packed 10 kHz wave; holds the
    window, the DFT basis and the ``Resampler``."""

    def __init__(self, device):
        self.ops = engine.Ops(device)
        self.lib, self.device = self.ops.lib, self.ops.device
        self.resampler = resample.Resampler(self.device)
        self.select_sweep = int(self.lib.tts_stoi_select_sweep())
        self.segments_per_group = int(self.lib.tts_stoi_segments_per_group())
        self.window_d = torch.from_numpy(window()).to(self.device)
        self.basis = packing.ConvWeights(dft_basis(), None, MODE_LINEAR, 1, 0, self.device)
        self.last = {}  # the device buffers of the last score_packed call (tests, tools)

    def _i64(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.device)

    @torch.inference_mode()
    def select(self, packed, pairs):
        """pairs: int64 [P, 3] = (first sample of the recording, of the generated signal, samples) -> (kept int32 [P, max_frames],
        counts int32 [P], max_frames, the device copy of the pairs): the frames that pass the 40 dB mask, ascending."""
        assert packed.dtype == torch.float32 and packed.dim() == 1 and packed.device == self.device and packed.is_contiguous()
        P = len(pairs)
        frames = [frame_count(n) for n in pairs[:, 2]]
        max_frames = max([1] + frames)
        pairs_d = self._i64(pairs)
        energy = torch.empty((P, max_frames), dtype=torch.float64, device=self.device)
        kept = torch.empty((P, max_frames), dtype=torch.int32, device=self.device)
        counts = torch.zeros(P, dtype=torch.int32, device=self.device)
        st = self.ops.stream()
        capi.check(self.lib.tts_stoi_frame_energy(packed.data_ptr(), packed.numel(), pairs_d.data_ptr(), pairs.ctypes.data, P, self.window_d.data_ptr(),
                                                  max_frames, energy.data_ptr(), st), "tts_stoi_frame_energy")
        capi.check(self.lib.tts_stoi_select(energy.data_ptr(), pairs_d.data_ptr(), pairs.ctypes.data, P, packed.numel(), max_frames, kept.data_ptr(),
                                            counts.data_ptr(), st), "tts_stoi_select")
        self.last.update(energy=energy)
        return kept, counts, max_frames, pairs_d

    @torch.inference_mode()
    def gather(self, packed, pairs, pairs_d, kept, counts, max_frames):
        """-> (rows float32 [total_rows, 256], row_begin int64 [P, 2] on the host): per pair F rows for the recording
        and F for the generated signal, the first K of them the windowed frames of the compacted signal, the rest zeros."""
        P = len(pairs)
        frames = np.asarray([frame_count(n) for n in pairs[:, 2]], dtype=np.int64)
        row_begin = (np.cumsum(np.repeat(frames, 2)) - np.repeat(frames, 2)).reshape(P, 2).astype(np.int64)
        total = int(2 * frames.sum())
        rows = torch.empty((total, N_FRAME), dtype=torch.float32, device=self.device)
        rb_d = self._i64(row_begin)
        capi.check(self.lib.tts_stoi_gather(packed.data_ptr(), packed.numel(), pairs_d.data_ptr(), pairs.ctypes.data, P, self.window_d.data_ptr(),
                                            max_frames, kept.data_ptr(), counts.data_ptr(), rb_d.data_ptr(), row_begin.ctypes.data, total,
                                            rows.data_ptr(), self.ops.stream()), "tts_stoi_gather")
        return rows, row_begin

    @torch.inference_mode()
    def band_values(self, rows, row_begin, frames):
        """rows [total_rows, 256] -> float64 [total_rows, 15]: one DFT launch and one band launch for every signal of the batch."""
        total = rows.shape[0]
        bands = torch.empty((total, N_BANDS), dtype=torch.float64, device=self.device)
        if total == 0:
            return bands
        lengths, begins = zip(*[(int(F), int(b)) for F, rb in zip(frames, row_begin) for b in rb if F > 0])
        rag = Ragged(list(lengths), self.device, begins=list(begins))
        spec = self.ops.conv(self.basis, rows, self.ops.empty(total, 2 * N_BINS), rag, compute=capi.COMPUTE_F32, split_k=False)
        capi.check(self.lib.tts_stoi_bands(spec.data_ptr(), int(spec.stride(0)), total, bands.data_ptr(), self.ops.stream()), "tts_stoi_bands")
        return bands

    @torch.inference_mode()
    def tail(self, bands, row_begin, frames, counts):
        """bands float64 [total_rows, 15]; row_begin [P, 2]; frames [P] (the rows a side has); counts int32 [P] on the device (the
        rows of them that are frames: M) -> (segments float64 [P, max_segments, 2] = (STOI, ESTOI) of every segment - the slots
        past a pair's M - 29 are not written -, totals float64 [P, 2]) on the device."""
        assert bands.dtype == torch.float64 and bands.dim() == 2 and bands.shape[1] == N_BANDS and bands.is_contiguous() and bands.device == self.device
        row_begin = np.ascontiguousarray(row_begin, dtype=np.int64).reshape(-1, 2)
        frames = np.ascontiguousarray(frames, dtype=np.int64)
        P = len(frames)
        max_frames = max([1] + [int(f) for f in frames])
        max_segments = max(1, max_frames - SEGMENT + 1)
        segments = torch.empty((P, max_segments, 2), dtype=torch.float64, device=self.device)
        totals = torch.empty((P, 2), dtype=torch.float64, device=self.device)
        rb_d = self._i64(row_begin)
        st = self.ops.stream()
        capi.check(self.lib.tts_stoi_segments(bands.data_ptr(), bands.shape[0], rb_d.data_ptr(), row_begin.ctypes.data, frames.ctypes.data,
                                              counts.data_ptr(), P, max_frames, segments.data_ptr(), st), "tts_stoi_segments")
        capi.check(self.lib.tts_stoi_reduce(segments.data_ptr(), counts.data_ptr(), P, max_frames, totals.data_ptr(), st), "tts_stoi_reduce")
        return segments, totals

    @torch.inference_mode()
    def score_packed(self, packed, pair_spans, keep_segments=False, lengths=None):
        """packed: float32 [S] at 10 kHz on the device; pair_spans: [(first sample of the recording, first sample of the generated
        signal, samples)] -> one record per pair (see ``score``).  Seven launches for the whole batch; the kept counts and the
        totals come to the host once, at the end."""
        pairs = np.asarray([(int(a), int(b), int(n)) for a, b, n in pair_spans], dtype=np.int64).reshape(-1, 3)
        P = len(pairs)
        if P == 0:
            return []
        frames = [frame_count(n) for n in pairs[:, 2]]
        kept, counts, max_frames, pairs_d = self.select(packed, pairs)
        rows, row_begin = self.gather(packed, pairs, pairs_d, kept, counts, max_frames)
        bands = self.band_values(rows, row_begin, frames)
        segments, totals = self.tail(bands, row_begin, frames, counts)
        self.last.update(kept=kept, counts=counts, rows=rows, row_begin=row_begin, bands=bands, segments=segments, totals=totals)
        counts_h, totals_h = counts.cpu().numpy(), totals.cpu().numpy()
        records = []
        for p, (_, _, n) in enumerate(pairs):
            K = int(counts_h[p])
            ok = K >= SEGMENT
            S = K - SEGMENT + 1 if ok else 0
            rec = {"stoi": float(totals_h[p, 0]) if ok else math.nan, "estoi": float(totals_h[p, 1]) if ok else math.nan,
                   "status": "ok" if ok else "too_short", "frames": frames[p], "kept_frames": K, "segments": S,
                   "lengths": tuple(lengths[p]) if lengths is not None else (int(n), int(n))}
            if keep_segments:
                rec["segment_stoi"], rec["segment_estoi"] = segments[p, :S, 0], segments[p, :S, 1]
                rec["kept"] = kept[p, :K]
                rec["worst_segment"] = rec["worst_segment_seconds"] = None
                if S:
                    worst = int(torch.argmin(rec["segment_estoi"]))  # (a NaN segment is the smallest)
                    rec["worst_segment"] = worst
                    rec["worst_segment_seconds"] = int(kept[p, worst]) * HOP / SR  # where its first frame begins in the signal itself
            records.append(rec)
        return records

    @torch.inference_mode()
    def score(self, waves_a, waves_b, sr_a, sr_b=None, keep_segments=False):
        """waves_a: the recordings, waves_b: the generated signals - lists of 1-D arrays or device tensors of any lengths, at sr_a
        and sr_b (default: sr_a); what is not at 10 kHz is converted on the device.  A pair is cut to its shorter signal.  -> one
        dict per pair: ``stoi``, ``estoi`` (NaN unless ``status`` is "ok"), ``status`` ("ok", or "too_short": fewer than 256 samples
        or fewer than 30 frames left after the silent ones are dropped), ``frames``, ``kept_frames``, ``segments``, ``lengths`` (the
        samples of both at 10 kHz before the cut); with keep_segments ``segment_stoi``, ``segment_estoi`` (float64 [segments] on
        the device), ``kept`` (the kept frame indices), ``worst_segment`` (the one of the smallest ESTOI value) and
        ``worst_segment_seconds``, where it begins in the original signal's time (None without segments)."""
        if len(waves_a) != len(waves_b):
            raise ValueError(f"{len(waves_a)} recordings for {len(waves_b)} generated signals")
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
        return self.score_packed(packed, pair_spans, keep_segments, lengths)
