"""A stand-in kernel for the test of the error-budget test (tests/test_error_budget_cpu.py): the rounding model of
tests/abi_emulator.py with the arithmetic the kernels' comments describe - fp32 accumulation in 16-channel k-steps, tap-major - for
tts_conv1d, tts_wavenet_layer and tts_resblock_step, and ways of being subtly wrong (`MUTANTS`: six that show at unit scale, and
`RANGE_MUTANTS`: two that show only away from it, tests/test_dynamic_range_cpu.py).  Host memory only.

Only what the error-budget cases use is restated: the 16-bit products, LINEAR / GLU / GATED, the three prologues, bias, pre-add,
residual, 16-bit tensors.  Anything else is an assertion error.
"""
import contextlib

import numpy as np

from ims_toucan_prosody_variance_amd import capi
from tests import abi_emulator as ae

MUTANTS = {
    "truncate": "i: every conversion to 16 bits truncates instead of rounding to nearest",
    "replicate_pad": "ii: replicate instead of zero padding at the utterance ends of a conv",
    "drop_outer_tap": "iii: the outermost up-sampler tap dropped in the first and the last output frame of an utterance (not folded onto the edge sample)",
    "bias_block": "iv: the bias of one 32-channel block (channels 32 to 63; 0 to 31 of a 32-channel conv) scaled by 0.9",
    "halo_neighbour": "v: the two halo rows (one where the halo is one row) in front of an utterance's first tile taken from the rows in front of it in the packed layout",
    "gate_twice": "vi: the gate rounded to 16 bits twice: sigmoid -> 16 bits, then tanh x sigmoid -> 16 bits",
}
# Wrong only away from unit scale: the levels of tests/dynamic_range.py are there to see them.
RANGE_MUTANTS = {
    "flush_subnormals": "vii: every conversion to fp16 flushes what lies below fp16's smallest normal number (2^-14) to zero - the fp16 formats, and the "
                        "fp16 images of the matrix-core snake's model in either format",
    "phase_from_16bit": "viii: the snake's phase sin(u e^alpha) taken from u rounded to 16 bits; the model takes the fp32 u",
}
F16_MIN_NORMAL = np.float32(2.0 ** -14)


def _flush16(a):
    """round-to-nearest-even to fp16 with subnormal results flushed to zero, as float32."""
    h = np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)
    return np.where(np.abs(h) < F16_MIN_NORMAL, np.float32(0.0) * h, h)


@contextlib.contextmanager
def _model_flushes_fp16():
    """The rounding model's own conversions to fp16 flush, for as long as the block lasts."""
    orig = ae._round16
    ae._round16 = lambda a, f16: _flush16(a) if f16 else orig(a, f16)
    try:
        yield
    finally:
        ae._round16 = orig


def _truncate16(a, f16):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not f16:
        return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = a.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


class StandIn(ae.Emulator):
    def __init__(self, mutant=None, **kw):
        super().__init__(**kw)
        assert mutant is None or mutant in MUTANTS or mutant in RANGE_MUTANTS
        self.mutant = mutant

    # ---- shared pieces ---------------------------------------------------------------------------------------------------------
    def r16(self, a, f16):
        a = np.asarray(a, dtype=np.float32)
        if self.mutant == "flush_subnormals" and f16:
            return _flush16(a)
        return _truncate16(a, f16) if self.mutant == "truncate" else ae._round16(a, f16)

    def bias(self, ptr, n):
        b = ae._arr(ptr, n).astype(np.float32).copy()
        if self.mutant == "bias_block":
            lo = 32 if n >= 64 else 0
            b[lo:lo + 32] *= np.float32(0.9)
        return b

    def conv32(self, x, w, dil, pad_left, front=None):
        """x [n, cin] (16-bit values), w [taps, cin_pad, wn] -> fp32 [n, wn]: zero 'same' padding, tap-major, one fp32 add per
        16-channel k-step.  front: the two rows in front of the utterance in the packed layout (mutant v)."""
        n, cin = x.shape
        taps = w.shape[0]
        xp = np.zeros((n + (taps - 1) * dil, cin), np.float32)
        xp[pad_left:pad_left + n] = x
        if self.mutant == "replicate_pad":
            xp[:pad_left] = x[0]
            xp[pad_left + n:] = x[-1]
        if self.mutant == "halo_neighbour" and front is not None:
            m = min(2, pad_left)
            xp[pad_left - m:pad_left] = front[2 - m:]
        acc = np.zeros((n, w.shape[2]), np.float32)
        for j in range(taps):
            rows = xp[j * dil:j * dil + n].astype(np.float64)
            for k0 in range(0, cin, 16):
                acc += (rows[:, k0:k0 + 16] @ w[j, k0:k0 + 16].astype(np.float64)).astype(np.float32)
        return acc

    def snake(self, X, alpha, beta, filt, f16):
        """abi_emulator._snake_seq through the folded filter matrices (fp32 taps, float64 sums)."""
        T = X.shape[0]
        U, D = (m.astype(np.float64) for m in ae._snake_fir_matrices(T, filt))
        if self.mutant == "drop_outer_tap":
            U[0, 0] -= 2.0 * np.float64(filt[11])
            U[2 * T - 1, T - 1] -= 2.0 * np.float64(filt[0])
        ea = np.exp(alpha.astype(np.float64))
        ib = 1.0 / (np.exp(beta.astype(np.float64)) + 1e-9)
        u = U @ X.astype(np.float64)
        phase_u = self.r16(u, f16).astype(np.float64) if self.mutant == "phase_from_16bit" else u
        return D @ (u + ib * np.sin(phase_u * ea) ** 2)

    @staticmethod
    def weights(ptr, taps, cin_pad, wn, f16):
        raw = ae._arr(ptr, taps * cin_pad * wn, np.uint16).reshape(taps, cin_pad // 8, wn, 8)
        return ae._widen16(raw, f16).reshape(raw.shape).transpose(0, 1, 3, 2).reshape(taps, cin_pad, wn)

    # ---- tts_conv1d ------------------------------------------------------------------------------------------------------------
    def tts_conv1d(self, dref, stream):
        d = dref._obj
        assert d.compute in (capi.COMPUTE_BF16, capi.COMPUTE_F16) and d.mode != capi.MODE_COUPLING
        assert not d.seqvec and not d.accumulate and d.act == capi.ACT_NONE and d.alpha == 1.0
        f16 = d.compute == capi.COMPUTE_F16
        dual = d.mode != capi.MODE_LINEAR
        fx, fy, fr = (ae._fmt(d.io_flags & b, f16) for b in (capi.IO_X_BF16, capi.IO_Y_BF16, capi.IO_RES_BF16))
        w = self.weights(d.w, d.taps, d.cin_pad, d.wn, f16)
        bias = self.bias(d.bias, d.cout * (2 if dual else 1))

        def staged(x):  # the conv's 16-bit operand from rows of one utterance
            if d.pre_act == capi.PRE_LRELU:
                x = np.where(x > 0, x, x * np.float32(d.pre_slope))
            elif d.pre_act == capi.PRE_SNAKE:
                x = self.snake(x, ae._arr(d.snake_alpha, d.cin), ae._arr(d.snake_beta, d.cin), ae._arr(d.snake_filt, 12), f16).astype(np.float32)
            return self.r16(x, f16)

        for sb, se, sid in ae._seqs_from_tiles(ae._tiles(d.tiles, d.n_tiles)):
            x = staged(ae._load(d.x, sb, se, d.cin, d.ldx, fx))
            front = staged(ae._load(d.x, sb - 2, sb, d.cin, d.ldx, fx)) if sb >= 2 else None
            acc = self.conv32(x, w[:, :d.cin], d.dil, d.pad_left, front)
            a = acc[:, :d.cout] + bias[:d.cout]
            if d.preadd:
                a = a + ae._mat(d.preadd, se, d.cout, d.ld_preadd)[sb:se]
            if dual:
                g = acc[:, d.half_pad:d.half_pad + d.cout] + bias[d.cout:]
                if d.preadd:
                    g = g + ae._mat(d.preadd + 4 * d.cout, se, d.cout, d.ld_preadd)[sb:se]
                sig = 1.0 / (1.0 + np.exp(-g.astype(np.float64)))
                v = a * sig if d.mode == capi.MODE_GLU else np.tanh(a.astype(np.float64)) * sig
            else:
                v = a
            v = np.asarray(v, dtype=np.float32)
            if d.res:
                v = v + np.float32(d.res_scale) * ae._load(d.res, sb, se, d.cout, d.ld_res, fr)
            if fy:
                v = self.r16(v, f16)  # (the store's own rounding is then exact)
            ae._store(d.y, sb, se, d.cout, d.ldy, v, fy)
        return 0

    # ---- tts_wavenet_layer -----------------------------------------------------------------------------------------------------
    def tts_wavenet_layer(self, dref, stream):
        d = dref._obj
        f16 = d.compute == capi.COMPUTE_F16
        H, n2 = 192, d.cout2
        w1 = self.weights(d.w1, 5, H, 384, f16)
        w2 = self.weights(d.w2, 1, H, n2, f16)
        b1, b2 = self.bias(d.b1, 384), ae._arr(d.b2, n2).astype(np.float32)
        col0 = 0 if n2 == 384 else H
        for sb, se, sid in ae._seqs_from_tiles(ae._tiles(d.tiles, d.n_tiles)):
            hs = ae._mat(d.hs_in, se, 384, d.ld_in)[sb:se].astype(np.float32)
            front = self.r16(ae._mat(d.hs_in, sb, 384, d.ld_in)[sb - 2:sb, :H], f16) if sb >= 2 else None
            acc = self.conv32(self.r16(hs[:, :H], f16), w1, 1, 2, front)
            cond = ae._mat(d.cond, se, 384, d.ld_cond)[sb:se]
            a = (acc[:, :H] + b1[:H]) + cond[:, :H]
            g = (acc[:, H:] + b1[H:]) + cond[:, H:]
            sig = 1.0 / (1.0 + np.exp(-g.astype(np.float64)))
            if self.mutant == "gate_twice":
                sig = self.r16(sig, f16).astype(np.float64)
            acts = self.r16(np.tanh(a.astype(np.float64)) * sig, f16)
            out = (self.conv32(acts, w2, 1, 0) + b2) + hs[:, col0:col0 + n2]
            ae._mat(d.hs_out, se, 384, d.ld_out)[sb:se, col0:col0 + n2] = out
        return 0

    # ---- tts_resblock_step -----------------------------------------------------------------------------------------------------
    def tts_resblock_step(self, dref, stream):
        d = dref._obj
        if self.mfma_snake:  # the matrix-core snake's model as it stands (float64 sums), its fp16 conversions flushing for mutant vii
            assert self.mutant in (None, "flush_subnormals")
            with _model_flushes_fp16() if self.mutant else contextlib.nullcontext():
                return super().tts_resblock_step(dref, stream)
        assert not d.accumulate
        C_, k = d.c, d.taps
        f16 = d.compute == capi.COMPUTE_F16
        io = ae._fmt(d.io_bf16, f16)
        w1, w2 = self.weights(d.w1, k, C_, C_, f16), self.weights(d.w2, k, C_, C_, f16)
        b1, b2 = self.bias(d.b1, C_), ae._arr(d.b2, C_).astype(np.float32)
        snake = d.act == capi.PRE_SNAKE
        filt = ae._arr(d.filt, 12) if snake else None
        h = (k - 1) // 2

        def act(v, al, be):
            if snake:
                return self.snake(v, ae._arr(al, C_), ae._arr(be, C_), filt, f16).astype(np.float32)
            return np.where(v > 0, v, v * np.float32(d.slope))

        for sb, se, sid in ae._seqs_from_tiles(ae._tiles(d.tiles, d.n_tiles)):
            x = ae._load(d.x, sb, se, C_, d.ldx, io)
            front = self.r16(act(ae._load(d.x, sb - 2, sb, C_, d.ldx, io), d.alpha1, d.beta1), f16) if sb >= 2 else None
            t = self.conv32(self.r16(act(x, d.alpha1, d.beta1), f16), w1, d.dil, h * d.dil, front) + b1
            if snake:
                t = self.r16(t, f16)
            a2 = self.r16(act(t, d.alpha2, d.beta2), f16)
            v = np.float32(d.alpha) * (self.conv32(a2, w2, 1, h) + b2) + np.float32(d.res_scale) * x
            if io:
                v = self.r16(v, f16)
            ae._store(d.y, sb, se, C_, d.ldy, v.astype(np.float32), io)
        return 0
