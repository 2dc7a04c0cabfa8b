"""Fused residual step: the index and predicate arithmetic of its staging and epilogues, on the shapes where it can go wrong.

The staging of x derives a thread's (row, channel group) once per round and steps it, builds one row predicate per 16-byte unit
and addresses x by 32-bit offsets from the tile's first fetched row.  So the batches here sit on the tile edges (BM - 1, BM, BM + 1 rows; two tiles and a few rows; utterances shorter
than the filters' reach; alignment rows between utterances), for every channel count with a matrix-core snake, the smallest and
the widest conv window, both 16-bit formats, both activations and both storage forms of x / y (16-bit and fp32).  Each case is
checked against a float64 reference (the one test_gpu_kernels_vs_float64 builds), in the plain form and in the scaled,
accumulating form of a stage mean, for untouched alignment rows, and for the batch-independence invariant (an utterance run alone
equals its rows of the batch, bit for bit).  The bf16 pack (two values, one conversion) is checked through tts_conv1d.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, packing
from ims_toucan_prosody_variance_amd.ragged import Ragged

from oracle import toucan_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {capi.COMPUTE_F16: 3e-3, capi.COMPUTE_BF16: 2e-2}  # the project's 16-bit tolerances (test_gpu_kernels_vs_float64.TOL)
PACK16 = {capi.COMPUTE_BF16: "bf16", capi.COMPUTE_F16: "f16"}
STORE16 = {capi.COMPUTE_BF16: torch.bfloat16, capi.COMPUTE_F16: torch.float16}
SLOPE = 0.1
SENTINEL = 9.0


def tile_rows(c):
    return 480 if c == 64 else 224


def batches(c):
    bm = tile_rows(c)
    return [[1], [bm - 1, bm, bm + 1], [2 * bm + 7, 9, 2], [5]]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine.Ops(DEV)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def grid16(*shape, seed):
    """Values every storage format here holds exactly (multiples of 1/16 below 4: six significant bits), so that one float64
    reference serves the bf16, fp16 and fp32 tensors alike."""
    return (rnd(*shape, seed=seed) * 16.0).round().clamp(-63.0, 63.0) / 16.0


def spans(rag):
    return list(zip(rag.begins, rag.lengths))


def close(got, want, tol, what=""):
    got, want = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, f"{what} max abs err {err:.3e} vs tol {tol * scale:.3e}"


def snake_f64(xu, alpha, beta, filt):
    return oracle.activation1d(xu.t().contiguous(), lambda v: oracle.snake_beta(v, alpha, beta), filt)


@functools.lru_cache(maxsize=None)
def problem(c, k, dil):
    """Weights, biases and snake parameters (float64 copies of fp32 values), shared by every case of a shape."""
    w1 = rnd(c, c, k, seed=1, scale=1.0 / np.sqrt(c * k)).float().double()
    w2 = rnd(c, c, k, seed=2, scale=1.0 / np.sqrt(c * k)).float().double()
    b1, b2 = rnd(c, seed=3, scale=0.1).float().double(), rnd(c, seed=4, scale=0.1).float().double()
    sn = [rnd(c, seed=s, scale=0.3).float().double() for s in (7, 8, 9, 10)]
    filt = torch.from_numpy(packing.kaiser_sinc_filter12()).double()
    return w1, w2, b1, b2, sn, filt


@functools.lru_cache(maxsize=None)
def reference(c, k, dil, act, batch_index):
    """(x, y0, [conv2(act2(conv1(act1(x_u)))) per utterance]) in float64: computed once, read by every format and storage form."""
    w1, w2, b1, b2, (a1, be1, a2, be2), filt = problem(c, k, dil)
    lengths = batches(c)[batch_index]
    rag = Ragged(lengths, "cpu", align=2)
    x = grid16(rag.total_rows, c, seed=5 + batch_index)
    y0 = grid16(rag.total_rows, c, seed=50 + batch_index)
    outs = []
    for b0, n in spans(rag):
        xu = x[b0:b0 + n]
        if act == capi.PRE_SNAKE:
            t = F.conv1d(snake_f64(xu, a1, be1, filt).unsqueeze(0), w1, b1, padding=(k - 1) // 2 * dil, dilation=dil)
            t = oracle.activation1d(t[0], lambda v: oracle.snake_beta(v, a2, be2), filt).unsqueeze(0)
        else:
            t = F.conv1d(F.leaky_relu(xu.t().unsqueeze(0), SLOPE), w1, b1, padding=(k - 1) // 2 * dil, dilation=dil)
            t = F.leaky_relu(t, SLOPE)
        outs.append(F.conv1d(t, w2, b2, padding=(k - 1) // 2)[0].t().contiguous())
    return x, y0, outs


@pytest.mark.parametrize("store", ["16bit", "fp32"])
@pytest.mark.parametrize("act", [capi.PRE_SNAKE, capi.PRE_LRELU], ids=["snake", "lrelu"])
@pytest.mark.parametrize("compute", [capi.COMPUTE_BF16, capi.COMPUTE_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("k,dil", [(3, 1), (11, 5)])
@pytest.mark.parametrize("c", [32, 64, 128])
def test_resblock_step_tile_edges(ops, c, k, dil, compute, act, store):
    w1, w2, b1, b2, (a1, be1, a2, be2), filt = problem(c, k, dil)
    c1 = packing.pack_conv(w1.float().numpy(), b1.float().numpy(), ops.device, dil=dil, bf16=PACK16[compute])
    c2 = packing.pack_conv(w2.float().numpy(), b2.float().numpy(), ops.device, dil=1, bf16=PACK16[compute])
    dt = STORE16[compute] if store == "16bit" else torch.float32
    f32 = lambda t: t.to(torch.float32).to(DEV).contiguous()
    sn1, sn2, fd = (f32(a1), f32(be1)), (f32(a2), f32(be2)), f32(filt)
    fir_tab = packing.snake_fir_table(packing.kaiser_sinc_filter12(), ops.device)
    third = 1.0 / 3.0

    def step(x, y, rag, scaled):
        kw = dict(alpha=third, res_scale=third, accumulate=True) if scaled else {}
        ops.resblock_step(c1, c2, x, y, rag, act, SLOPE, sn1, sn2, fd, fir_tab=fir_tab, **kw)

    for bi, lengths in enumerate(batches(c)):
        x64, y64, outs = reference(c, k, dil, act, bi)
        rag = Ragged(lengths, ops.device, align=2)
        x = x64.to(DEV).to(dt).contiguous()
        y0 = y64.to(DEV).to(dt).contiguous()
        live = torch.zeros(rag.total_rows, dtype=torch.bool, device=DEV)
        for b0, n in spans(rag):
            live[b0:b0 + n] = True
        # plain form into a tensor of sentinels, scaled and accumulating form (the stage-mean step) into a pre-filled y
        y_plain = torch.full((rag.total_rows, c), SENTINEL, device=DEV, dtype=dt)
        y_mean = y0.clone()
        step(x, y_plain, rag, False)
        step(x, y_mean, rag, True)
        torch.cuda.synchronize()
        what = f"C={c} k={k} lengths={lengths}"
        for (b0, n), out in zip(spans(rag), outs):
            close(y_plain[b0:b0 + n], out + x64[b0:b0 + n], TOL[compute], f"{what}: plain, {n} frames:")
            close(y_mean[b0:b0 + n], third * out + third * x64[b0:b0 + n] + y64[b0:b0 + n], TOL[compute], f"{what}: mean step, {n} frames:")
        # rows between utterances belong to nobody
        assert bool((y_plain[~live] == SENTINEL).all()), f"{what}: an alignment row was written"
        assert torch.equal(y_mean[~live], y0[~live]), f"{what}: an alignment row was accumulated into"
        # an utterance's result does not depend on the batch it is in
        if len(lengths) > 1:
            for b0, n in spans(rag):
                alone = Ragged([n], ops.device, align=2)
                ya = torch.full((n, c), SENTINEL, device=DEV, dtype=dt)
                ym = y0[b0:b0 + n].clone()
                step(x[b0:b0 + n], ya, alone, False)
                step(x[b0:b0 + n], ym, alone, True)
                torch.cuda.synchronize()
                assert torch.equal(ya, y_plain[b0:b0 + n]), f"{what}: {n} frames alone differ from the batch (plain)"
                assert torch.equal(ym, y_mean[b0:b0 + n]), f"{what}: {n} frames alone differ from the batch (mean step)"


def bits16(t):
    return t.contiguous().view(torch.int16)


def test_pack16_bf16_rounding_through_conv(ops):
    """Two values, one packed conversion: round to nearest even, NaN kept, signed zeros kept.  A 64-channel conv writes bf16 y
    that equals its own fp32 y converted by torch, bit for bit; and with fp32 x its operand staging (the pack itself) rounds x
    as torch does: the 1-tap identity conv returns exactly x.to(bfloat16)."""
    c, rows = 64, 96
    rag = Ragged([rows], ops.device)
    one, ulp = 1.0, 2.0 ** -7  # bf16 spacing at 1.0
    x = rnd(rows, c, seed=11).float()
    x[0, :] = one + 0.5 * ulp                       # ties towards the even neighbour below
    x[1, :] = one + 1.5 * ulp                       # ties towards the even neighbour above
    x[2, 0::2], x[2, 1::2] = -(one + 0.5 * ulp), -(one + 1.5 * ulp)
    x[3, :] = torch.tensor(np.nextafter(np.float32(one + 0.5 * ulp), np.float32(2.0)))  # just above a tie
    x[4, 0::2], x[4, 1::2] = 0.0, -0.0
    x[5, 7] = float("nan")
    xd = x.to(DEV)
    low = bits16(xd)[:, 0::2]  # (fp32 viewed as pairs of halves: the low half decides)
    assert int((low == -32768).sum()) >= 3 * c, "the input holds no ties"
    want16 = xd.to(torch.bfloat16)
    # the pack itself: fp32 x staged as bf16 operands of an identity conv (products and sums of one term are exact)
    eye = packing.pack_conv(np.eye(c, dtype=np.float32)[:, :, None], np.zeros(c, np.float32), ops.device, bf16="bf16")
    y32 = torch.zeros(rows, c, device=DEV)
    ops.conv(eye, xd, y32, rag, compute=capi.COMPUTE_BF16)
    torch.cuda.synchronize()
    clean = torch.ones(rows, dtype=torch.bool, device=DEV)
    clean[4] = False  # (a sum that starts from +0 returns +0 for either zero: values, not signs)
    clean[5] = False  # (the NaN meets every output channel of its row: 0 * NaN)
    got, want = bits16(y32[clean].to(torch.bfloat16)), bits16(want16[clean])
    assert torch.equal(y32[clean], want16[clean].float()) and torch.equal(got, want), f"{int((got != want).sum())} elements rounded differently"
    assert bool((y32[4] == 0.0).all()) and bool(torch.isnan(y32[5]).all())
    # a 16-bit-output conv against its own fp32 output: 3 taps, random weights, bias on a fine grid
    w = rnd(c, c, 3, seed=12, scale=1.0 / np.sqrt(3 * c)).float().numpy()
    b = rnd(c, seed=13, scale=0.1).float().numpy()
    cw = packing.pack_conv(w, b, ops.device, bf16="bf16")
    for xin in (xd, want16):
        y32 = torch.zeros(rows, c, device=DEV)
        y16 = torch.zeros(rows, c, device=DEV, dtype=torch.bfloat16)
        ops.conv(cw, xin, y32, rag, compute=capi.COMPUTE_BF16)
        ops.conv(cw, xin, y16, rag, compute=capi.COMPUTE_BF16)
        torch.cuda.synchronize()
        nan = torch.isnan(y32)
        assert bool(nan.any()) and not bool(nan.all())
        assert torch.equal(nan, torch.isnan(y16.float())), "NaN lost or made in the conversion"
        assert torch.equal(bits16(y16)[~nan], bits16(y32.to(torch.bfloat16))[~nan])
