"""Sample-rate conversion on the GPU (csrc/resample.hip, include/toucan_resample.h): any rational factor, float32 or PCM16 out,
for a ragged batch of waveforms or for one waveform that arrives in pieces.

The filter is the one ``style.resample_sinc`` restates in float64 - torchaudio.transforms.Resample's defaults (Hann window,
lowpass_filter_width 6, rolloff 0.99), third party, PARITY UNPINNED - as a polyphase table computed once per pair of rates on the
host in float64 and rounded to float32.  With ``g = gcd(sr_in, sr_out)``, ``orig = sr_in / g``, ``new = sr_out / g``, output
``m = i new + p`` of an utterance is ``sum_j k[p][j] x[i orig + j - w]`` over ``K = 2 w + orig`` samples, x taken as 0 outside the
utterance; there are ``ceil(new n / orig)`` outputs.  DESIGN.md section 13 holds the definition and the decisions.

Every output is one chain of K fused multiply-adds in a fixed order on its table row and its K samples: a batch returns bit for bit
what its utterances return alone, and a streamed utterance (``Resampler.streamer``) what the whole one returns.
"""
import math

import numpy as np
import torch

from . import capi

WIDTH, ROLLOFF = 6, 0.99  # torchaudio's lowpass_filter_width and rolloff
MAX_FACTOR = capi.RESAMPLE_MAX_FACTOR


def ratio(sr_in, sr_out):
    """(orig, new): the rates over their greatest common divisor.  ValueError for rates that are no positive integers or whose
    reduced ratio is past the kernel's limit."""
    if isinstance(sr_in, bool) or isinstance(sr_out, bool) or int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f"sample rates are positive integers, not {sr_in!r} -> {sr_out!r}")
    g = math.gcd(int(sr_in), int(sr_out))
    orig, new = int(sr_in) // g, int(sr_out) // g
    if max(orig, new) > MAX_FACTOR:
        raise ValueError(f"{sr_in} -> {sr_out} Hz reduces to {orig} -> {new}: past the resampler's limit of {MAX_FACTOR} "
                         f"(TTS_RESAMPLE_MAX_FACTOR) for either side of the reduced ratio")
    return orig, new


def kernel_table(sr_in, sr_out):
    """(orig, new, w, table float32 [new, K]), K = 2 w + orig: the coefficients style.resample_sinc applies, computed in float64
    and rounded once.  Equal rates give the identity (orig = new = 1, w = 0, table [[1]])."""
    orig, new = ratio(sr_in, sr_out)
    if orig == new:
        return 1, 1, 0, np.ones((1, 1), dtype=np.float32)
    base = min(orig, new) * ROLLOFF
    w = int(math.ceil(WIDTH * orig / base))
    idx = np.arange(-w, w + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -WIDTH, WIDTH)
    window = np.cos(t * np.pi / WIDTH / 2.0) ** 2
    t = t * np.pi
    kern = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)
    return orig, new, w, kern.astype(np.float32)


def out_length(n, sr_in, sr_out):
    """Samples n samples at sr_in become at sr_out: ceil(new n / orig)."""
    orig, new = ratio(sr_in, sr_out)
    return -((-new * int(n)) // orig)


class Streamer:
    """The bookkeeping of a waveform that arrives in pieces of any length.  ``launch(buffer, pos0, out_first, out_count)`` returns
    the outputs out_first .. out_first + out_count - 1 of the utterance whose samples pos0 .. pos0 + len(buffer) - 1 the buffer
    holds (every other sample counting as 0) - Resampler.streamer binds it to the kernel.  ``push(piece)`` returns exactly the
    outputs whose K samples have all arrived (possibly none), ``finish()`` the rest, computed against zeros; ``cat`` joins
    buffers and ``empty()`` makes the result of a push that completes nothing."""

    def __init__(self, launch, orig, new, w, cat, empty):
        self.launch, self.orig, self.new, self.w, self.cat, self.empty = launch, orig, new, w, cat, empty
        self.received = 0    # samples pushed so far
        self.emitted = 0     # outputs returned so far: always a whole number of blocks of `new`
        self.tail = None     # the samples tail_pos .. received - 1, which later outputs still read
        self.tail_pos = 0
        self.finished = False

    def _emit(self, buf, upto):
        count = upto - self.emitted
        if count <= 0:
            return self.empty()
        out = self.launch(buf, self.tail_pos, self.emitted, count)
        self.emitted = upto
        return out

    def push(self, piece):
        assert not self.finished, "push() after finish()"
        if len(piece) == 0:
            return self.empty()
        buf = piece if self.tail is None or len(self.tail) == 0 else self.cat([self.tail, piece])
        self.received += len(piece)
        # block i reads the samples up to i orig + w + orig - 1: complete while (i + 1) orig + w <= received
        blocks = max(0, (self.received - self.w) // self.orig)
        out = self._emit(buf, max(self.emitted, blocks * self.new))
        # the next block starts at emitted / new and reads from emitted / new * orig - w on
        keep_from = max(self.tail_pos, self.emitted // self.new * self.orig - self.w)
        self.tail, self.tail_pos = buf[keep_from - self.tail_pos:], keep_from
        return out

    def finish(self):
        assert not self.finished, "finish() twice"
        self.finished = True
        total = -((-self.new * self.received) // self.orig)
        if self.tail is None or total <= self.emitted:
            return self.empty()
        return self._emit(self.tail, total)


class Resampler:
    """``resample(packed_wave, spans, sr_in, sr_out, pcm16=False)`` for a ragged batch on the device, ``streamer(sr_in, sr_out,
    pcm16=False)`` for one waveform in pieces.  Tables are uploaded once per pair of rates and kept."""

    def __init__(self, device):
        self.lib = capi.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise capi.ToucanHipError(f"device {str(self.device)!r}: the resampler runs on the GPU only")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.tile_outputs = int(self.lib.tts_resample_tile_outputs())
        self._tables = {}

    def table(self, sr_in, sr_out):
        """(orig, new, w, device table [K, new]: the transposed layout the kernel reads)."""
        key = ratio(sr_in, sr_out)
        if key not in self._tables:
            orig, new, w, tab = kernel_table(sr_in, sr_out)
            self._tables[key] = (orig, new, w, torch.from_numpy(np.ascontiguousarray(tab.T)).to(self.device))
        return self._tables[key]

    def launch(self, wave, rows, sr_in, sr_out, pcm16=False):
        """rows: [(in_begin, n_held, pos0, out_first, out_count)] per utterance -> (packed output, [out_begin]).  On the current
        stream of the device, without a synchronisation."""
        assert wave.dtype == torch.float32 and wave.dim() == 1 and wave.device == self.device and wave.is_contiguous()
        orig, new, w, tab = self.table(sr_in, sr_out)
        spans = np.zeros((len(rows), 6), dtype=np.int64)
        at = 0
        for r, (in_begin, n_held, pos0, out_first, out_count) in enumerate(rows):
            assert 0 <= in_begin and 0 <= n_held and in_begin + n_held <= wave.numel() and pos0 >= 0 and out_first >= 0 and out_count >= 0
            spans[r] = (in_begin, n_held, pos0, out_first, out_count, at)
            at += out_count
        y = torch.empty(at, dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
        if at:
            # from pinned memory, so that the copy queues behind the work already on the stream instead of waiting for it
            spans_d = torch.from_numpy(spans).pin_memory().to(self.device, non_blocking=True)
            capi.check(self.lib.tts_resample(wave.data_ptr(), tab.data_ptr(), spans_d.data_ptr(), len(rows), int(spans[:, 4].max()), orig, new, w,
                                             int(bool(pcm16)), y.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "tts_resample")
        return y, [int(b) for b in spans[:, 5]]

    @torch.inference_mode()
    def resample(self, packed_wave, spans, sr_in, sr_out, pcm16=False):
        """packed_wave: float32 [S] on the device; spans: [(first sample, sample count)] per utterance -> (packed output, spans of
        the output), every utterance converted on its own."""
        orig, new = ratio(sr_in, sr_out)
        counts = [-((-new * int(n)) // orig) for _, n in spans]
        y, begins = self.launch(packed_wave, [(int(b), int(n), 0, 0, c) for (b, n), c in zip(spans, counts)], sr_in, sr_out, pcm16)
        return y, list(zip(begins, counts))

    def streamer(self, sr_in, sr_out, pcm16=False):
        """An object with ``push(piece)`` and ``finish()`` (Streamer) for one waveform at sr_in that arrives as 1-D float32 device
        tensors of any lengths; the pieces returned, concatenated, equal ``resample`` of the whole, bit for bit."""
        orig, new, w, _ = self.table(sr_in, sr_out)
        dtype = torch.int16 if pcm16 else torch.float32

        def launch(buf, pos0, out_first, out_count):
            return self.launch(buf.contiguous(), [(0, buf.numel(), pos0, out_first, out_count)], sr_in, sr_out, pcm16)[0]

        return Streamer(launch, orig, new, w, torch.cat, lambda: torch.empty(0, dtype=dtype, device=self.device))
