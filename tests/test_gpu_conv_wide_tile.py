"""The wide tile of tts_conv1d (csrc/conv1d_wide.hip: 256 x 256 outputs per workgroup, both operands by LDS-DMA) against the other
forms of the SAME call: it keeps their matrix instruction, accumulation order and epilogue, so `torch.equal` must hold against
the 128 x 128 form and against the 64-row small-batch form - an index, ordering or synchronisation mistake shows up as a difference.
The ragged batch [1, 24, 255, 256, 257, 700] holds an utterance shorter than the halo, one exactly a tile long, one a row over a
tile and one of several tiles with a partial last one; 256 input channels are four channel slabs, so 3 / 7 / 11 taps run 12 / 28 /
44 steps through the two buffers.  The polyphase up-samplers are compared by value (`torch.equal` treats -0 == +0 as equal): the
wide kernel leaves the structural zero taps out, which can only change the sign of an exact zero."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, packing
from ims_toucan_prosody_variance_amd.ragged import Ragged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {capi.COMPUTE_F16: 3e-3, capi.COMPUTE_BF16: 2e-2}  # relative to the output scale: tests/test_gpu_kernels_vs_float64.py's 16-bit tolerances
FMT = {capi.COMPUTE_BF16: ("bf16", torch.bfloat16), capi.COMPUTE_F16: ("f16", torch.float16)}
RAGGED = [1, 24, 255, 256, 257, 700]
STAGE1 = [(3, 1), (7, 3), (11, 5)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine.Ops(DEV)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def run_forms(ops, cw, x, rag, compute, forms, dtype, res=None, **kw):
    """The same call on each of `forms` (tile rows); the output starts from the same seeded tensor (it is read with `accumulate`)."""
    out = {}
    for tr in forms:
        y = rnd(rag.total_rows, cw.cout, seed=9).to(dtype).to(DEV)
        ops.conv(cw, x, y, rag, res=res, compute=compute, tile_rows=tr, **kw)
        out[tr] = y
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("second", [False, True], ids=["plain", "res_accumulate"])
@pytest.mark.parametrize("compute", [capi.COMPUTE_BF16, capi.COMPUTE_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("k,dil", STAGE1)
def test_stage1_conv_equals_the_other_forms(ops, k, dil, compute, second):
    """256 -> 256 channels as in the vocoder's first stage; `second`: the second conv of a residual step of the last dilation
    (residual, alpha = res_scale = 1/3, accumulate)."""
    fmt, dt = FMT[compute]
    c = 256
    rag = Ragged(RAGGED, ops.device)
    cw = packing.pack_conv(rnd(c, c, k, seed=1, scale=1.0 / np.sqrt(c * k)).float().numpy(), rnd(c, seed=2, scale=0.1).float().numpy(), ops.device,
                           dil=dil, bf16=fmt)
    x = rnd(rag.total_rows, c, seed=3).to(dt).to(DEV)
    res = rnd(rag.total_rows, c, seed=5).to(dt).to(DEV) if second else None
    kw = dict(alpha=1.0 / 3.0, res_scale=1.0 / 3.0, accumulate=True) if second else {}
    y = run_forms(ops, cw, x, rag, compute, (256, 128, 64), dt, res=res, **kw)
    assert torch.isfinite(y[256].float()).all()
    assert torch.equal(y[256], y[128]), "wide tile != 128 x 128 tile"
    assert torch.equal(y[256], y[64]), "wide tile != 64-row form"


@pytest.mark.parametrize("compute", [capi.COMPUTE_BF16, capi.COMPUTE_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,stride", [(512, 256, 8), (256, 128, 6), (128, 64, 4)], ids=["512to2048", "256to768", "128to256"])
def test_polyphase_upsampler_equals_the_other_forms(ops, cin, cout, stride, compute):
    """Transposed convs packed as 3-tap polyphase convs (TTS_IO_POLYPHASE; only the wide kernel acts on the flag): 512 -> 2048
    skips whole steps per workgroup, 256 -> 768 per wavefront in the middle workgroup (wn / 2 = 384), 128 -> 256 per wavefront."""
    fmt, dt = FMT[compute]
    rag = Ragged([1, 130, 300], ops.device)
    w = rnd(cin, cout, 2 * stride, seed=11, scale=1.0 / np.sqrt(2 * cin)).float()
    cw = packing.pack_conv_transpose(w.numpy(), rnd(cout, seed=12, scale=0.1).float().numpy(), stride, ops.device, bf16=fmt)
    assert cw.algo_taps == 2 and cw.taps == 3 and cw.wn == stride * cout
    x = rnd(rag.total_rows, cin, seed=13).to(dt).to(DEV)
    y = run_forms(ops, cw, x, rag, compute, (256, 128, 64), dt)
    assert torch.isfinite(y[256].float()).all()
    assert torch.equal(y[256], y[128]), "wide tile != 128 x 128 tile"
    assert torch.equal(y[256], y[64]), "wide tile != 64-row form"


@pytest.mark.parametrize("compute", [capi.COMPUTE_BF16, capi.COMPUTE_F16], ids=["bf16", "f16"])
def test_wide_conv_vs_float64(ops, compute):
    """256 -> 256, 11 taps, dilation 5 against torch's float64 conv of the values the kernel sees."""
    fmt, dt = FMT[compute]
    c, k, dil = 256, 11, 5
    rag = Ragged(RAGGED, ops.device)
    w = rnd(c, c, k, seed=1, scale=1.0 / np.sqrt(c * k)).to(dt).double()
    b = rnd(c, seed=2, scale=0.1).float().double()
    x = rnd(rag.total_rows, c, seed=3).to(dt)
    cw = packing.pack_conv(w.float().numpy(), b.float().numpy(), ops.device, dil=dil, bf16=fmt)
    y = torch.zeros(rag.total_rows, c, device=DEV, dtype=dt)
    ops.conv(cw, x.to(DEV), y, rag, compute=compute, tile_rows=256)
    torch.cuda.synchronize()
    for b0, n in zip(rag.begins, rag.lengths):
        want = F.conv1d(x[b0:b0 + n].double().t().unsqueeze(0), w, b, padding=(k - 1) // 2 * dil, dilation=dil)[0].t()
        got = y[b0:b0 + n].cpu().double()
        scale = max(1.0, float(want.abs().max()))
        err = float((got - want).abs().max())
        assert err <= TOL[compute] * scale, f"{n} frames: max abs err {err:.3e} vs tol {TOL[compute] * scale:.3e}"


@pytest.mark.parametrize("case", ["fp32_x", "wn_384", "pre_activation"])
def test_ineligible_call_with_a_256_row_table_is_an_argument_error(ops, case):
    c = 256
    cout = 384 if case == "wn_384" else c
    rag = Ragged([300], ops.device)
    cw = packing.pack_conv(rnd(cout, c, 3, seed=1, scale=0.05).float().numpy(), None, ops.device, bf16="bf16")
    x = rnd(rag.total_rows, c, seed=3).to(torch.float32 if case == "fp32_x" else torch.bfloat16).to(DEV)
    y = torch.zeros(rag.total_rows, cout, device=DEV, dtype=torch.bfloat16)
    kw = dict(pre=capi.PRE_LRELU, pre_slope=0.1) if case == "pre_activation" else {}
    with pytest.raises(capi.ToucanHipError) as e:
        ops.conv(cw, x, y, rag, compute=capi.COMPUTE_BF16, tile_rows=256, **kw)
    assert "code -1" in str(e.value) and "wide tile" in str(e.value)  # TTS_E_ARG, with the reason
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0  # nothing was launched
