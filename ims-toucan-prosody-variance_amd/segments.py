"""What the meters over 100 ms segments share (csrc/segment_scan.h): segment length, target check, tables, span rows, the gain kernel."""
import math

import numpy as np
import torch

from . import capi

MIN_RATE, MAX_RATE = capi.LOUDNESS_MIN_RATE, capi.LOUDNESS_MAX_RATE


def segment_samples(sr):
    """Samples of one 100 ms segment.  ValueError for a rate that is no multiple of 10 in 8 000 .. 192 000."""
    takes = f"the loudness meter takes a sample rate that is a multiple of 10 in {MIN_RATE} .. {MAX_RATE} Hz"
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) and not (isinstance(sr, float) and sr.is_integer()):
        raise ValueError(f"{takes}, not {sr!r}")
    sr = int(sr)
    if sr % 10 or not MIN_RATE <= sr <= MAX_RATE:
        raise ValueError(f"{takes} (100 ms segments of a whole number of samples), not {sr}")
    return sr // 10


def check_target(what, target, ceiling):
    for name, v in (("target", target), ("peak ceiling", ceiling)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"the {what} {name} must be a finite number, not {v!r}")
    if ceiling > 0:
        raise ValueError(f"the peak ceiling {ceiling!r} dBFS is above full scale (0 dBFS)")


class SegmentMeter:
    """A meter on one device: ``kernel_table(sr)`` (float64, uploaded once per rate and kept), ``tile_entry`` (segments per workgroup)."""

    def __init__(self, device, name, kernel_table, tile_entry):
        self.lib = capi.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise capi.ToucanHipError(f"device {str(self.device)!r}: the {name} runs on the GPU only")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tile_segments = int(getattr(self.lib, tile_entry)())
        self._kernel_table, self._tables = kernel_table, {}

    def table(self, sr):
        if int(sr) not in self._tables:
            self._tables[int(sr)] = torch.from_numpy(self._kernel_table(sr)).to(self.device)
        return self._tables[int(sr)]

    def _rows(self, wave, spans):
        assert wave.dtype == torch.float32 and wave.dim() == 1 and wave.device == self.device and wave.is_contiguous()
        rows = np.ascontiguousarray(np.asarray([(int(b), int(n)) for b, n in spans], dtype=np.int64).reshape(-1, 2))
        # from pinned memory, so that the copy queues behind the work already on the stream instead of waiting for it
        return rows, torch.from_numpy(rows).pin_memory().to(self.device, non_blocking=True)

    @staticmethod
    def _max_segments(rows, S):
        return max(1, int(-(-rows[:, 1].max() // S))) if len(rows) else 1

    def _apply_gain(self, packed_wave, rows, rows_d, stats, out):
        """-> out: every span of ``packed_wave`` times the gain in its row of ``stats``; ``out`` as the meters' normalize takes it."""
        if out is None:
            tiled = len(rows) > 0 and int(rows[0, 0]) == 0 and int(rows[-1].sum()) == packed_wave.numel() and \
                bool((rows[1:, 0] == rows[:-1].sum(axis=1)).all())
            out = torch.empty_like(packed_wave) if tiled else packed_wave.clone()
        assert out.dtype == torch.float32 and out.shape == packed_wave.shape and out.device == self.device and out.is_contiguous()
        if len(rows):
            capi.check(self.lib.tts_apply_gain(packed_wave.data_ptr(), packed_wave.numel(), rows_d.data_ptr(), rows.ctypes.data, len(rows),
                                               int(rows[:, 1].max()), stats.data_ptr(), out.data_ptr(),
                                               torch.cuda.current_stream(self.device).cuda_stream), "tts_apply_gain")
        return out
