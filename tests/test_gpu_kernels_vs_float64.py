"""Library entry points against plain float64 restatements of the same operation (torch.nn.functional, or the oracle's own functions
in oracle/toucan_oracle.py) - never against the ABI emulator, which was written from the same reading of the model as the kernels.
The inputs are the ones gentle random data cannot stand in for: large offsets next to the spread (cancellation in the norms),
peaked / rising / position-dominated attention scores (the online-softmax rescaling, the key-split merge, the relative shift) and
anti-alias filters that are not symmetric (the order in which every snake consumer reads its taps).
Tolerances relative to the output scale: fp32 2e-5, fp16 3e-3, bf16 2e-2."""
import math
import os
import subprocess
import sys

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
TOL = {capi.COMPUTE_F32: 2e-5, capi.COMPUTE_F16: 3e-3, capi.COMPUTE_BF16: 2e-2}
PACK16 = {capi.COMPUTE_F32: True, capi.COMPUTE_BF16: "bf16", capi.COMPUTE_F16: "f16"}
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine.Ops(DEV)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def dev(t):
    return t.to(torch.float32).to(DEV).contiguous()


def close(got, want, tol, what=""):
    got, want = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= tol * scale, f"{what} max abs err {err:.3e} vs tol {tol * scale:.3e}"


def spans(rag):
    return list(zip(rag.begins, rag.lengths))


# ---------------------------------------------------------------------------------------------------------------------------
# Norms on offset inputs: x = m + s * randn (+ a per-channel offset), the reference computed from the fp32 values in float64
# ---------------------------------------------------------------------------------------------------------------------------
OFFSETS = [(0.0, False), (40.0, False), (300.0, False), (40.0, True), (300.0, True)]  # (m / s with s = 1, per-channel offsets)


def offset_input(rows, c, m, per_channel, seed):
    x = m + rnd(rows, c, seed=seed)
    if per_channel:
        x = x + rnd(c, seed=seed + 100, scale=3.0)
    return x.float().double()  # (the values the kernel sees)


@pytest.mark.parametrize("m,per_channel", OFFSETS)
@pytest.mark.parametrize("c", [192, 256])
def test_layernorm_offset_inputs(ops, m, per_channel, c):
    rows = 301
    x = offset_input(rows, c, m, per_channel, seed=1)
    g, b = 1.0 + rnd(c, seed=2, scale=0.1), rnd(c, seed=3, scale=0.1)
    got = ops.layernorm(dev(x), ops.empty(rows, c), dev(g), dev(b), rows, c)
    torch.cuda.synchronize()
    close(got, F.layer_norm(x, (c,), g.float().double(), b.float().double(), eps=1e-12), TOL[capi.COMPUTE_F32])


@pytest.mark.parametrize("m,per_channel", OFFSETS)
def test_cond_layernorm_offset_inputs(ops, m, per_channel):
    """oracle.conditional_layer_norm's body: scale * (x - mean) / var + shift (the variance, no eps: s stays at 1)."""
    c, lengths = 256, [70, 1, 129, 64]
    rag = Ragged(lengths, ops.device)
    x = offset_input(rag.total_rows, c, m, per_channel, seed=4)
    sc, sh = rnd(len(lengths), c, seed=5), rnd(len(lengths), c, seed=6)
    got = ops.cond_layernorm(dev(x), ops.empty(rag.total_rows, c), dev(sc), dev(sh), c, rag)
    torch.cuda.synchronize()
    for u, (b0, n) in enumerate(spans(rag)):
        xu = x[b0:b0 + n]
        mean = xu.mean(dim=-1, keepdim=True)
        var = ((xu - mean) ** 2).mean(dim=-1, keepdim=True)
        want = sc[u].float().double() * ((xu - mean) / var) + sh[u].float().double()
        close(got[b0:b0 + n], want, TOL[capi.COMPUTE_F32], f"utterance {u}:")


@pytest.mark.parametrize("m", [0.0, 40.0, 300.0])
@pytest.mark.parametrize("c", [64, 192])
def test_l2_normalize_offset_inputs(ops, m, c):
    x = offset_input(37, c, m, False, seed=7)
    got = ops.l2_normalize(dev(x), ops.empty(37, c))
    torch.cuda.synchronize()
    close(got, F.normalize(x, dim=1), TOL[capi.COMPUTE_F32])


@pytest.mark.parametrize("m,per_channel", OFFSETS)
@pytest.mark.parametrize("c,groups,tanh", [(256, 32, True), (80, 20, False)])
def test_groupnorm_offset_inputs(ops, m, per_channel, c, groups, tanh):
    """PostNet's two GroupNorms (+ tanh / + residual) per utterance of a ragged batch: 1 frame, one chunk short of, exactly and one
    past a 16-frame chunk, and 4000 frames (250 chunks merged)."""
    lengths = [1, 15, 16, 17, 4000, 33]
    rag = Ragged(lengths, ops.device, align=2)
    R = rag.total_rows
    x = offset_input(R, c, m, per_channel, seed=8)
    g, b = (1.0 + rnd(c, seed=9, scale=0.1)).float().double(), rnd(c, seed=10, scale=0.1).float().double()
    res = rnd(R, c, seed=11).float().double()
    got = ops.groupnorm(dev(x), ops.empty(R, c), dev(g), dev(b), c, groups, rag, tanh=tanh, res=None if tanh else dev(res))
    torch.cuda.synchronize()
    for b0, n in spans(rag):
        want = F.group_norm(x[b0:b0 + n].t().unsqueeze(0), groups, g, b, eps=1e-5)[0].t()
        want = torch.tanh(want) if tanh else want + res[b0:b0 + n]
        close(got[b0:b0 + n], want, TOL[capi.COMPUTE_F32], f"{n} frames:")


# ---------------------------------------------------------------------------------------------------------------------------
# Relative-position attention: fp32 plain, fp32 key-split (forced), fp16
# ---------------------------------------------------------------------------------------------------------------------------
HEADS, DK, HD = 4, 48, 192
PMAX = 700
ATT_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 700]  # (700 = pmax: the first and the last table row are used)
ATT_FORMS = {"plain": dict(flags=0), "key_split": dict(flags=capi.ATT_KEY_SPLIT_ALWAYS), "f16": dict(f16=True)}


def attention_f64(qkv, ptab, pmax, bias_u, bias_v, n):
    """One utterance of n rows, as oracle.rel_attention computes its scores (Attention.py:159-198): qu k^T + rel_shift(qv P^T), / sqrt(dk),
    softmax, @ v.  ptab[pmax - 1 + p] holds the projected encoding of relative position p; the oracle's table for n rows lists
    positions n-1 ... -(n-1)."""
    q, k, v = qkv[:, :HD].view(n, HEADS, DK), qkv[:, HD:2 * HD].view(n, HEADS, DK).transpose(0, 1), qkv[:, 2 * HD:].view(n, HEADS, DK).transpose(0, 1)
    pp = ptab[pmax - 1 + (n - 1) - torch.arange(2 * n - 1)].view(2 * n - 1, HEADS, DK).transpose(0, 1)
    qu = (q + bias_u.view(HEADS, DK)).transpose(0, 1)
    qv = (q + bias_v.view(HEADS, DK)).transpose(0, 1)
    ac = qu @ k.transpose(1, 2)
    bd = qv @ pp.transpose(1, 2)
    idx = (n - 1) - torch.arange(n).unsqueeze(1) + torch.arange(n).unsqueeze(0)
    bd = torch.gather(bd, 2, idx.unsqueeze(0).expand(HEADS, n, n))
    attn = torch.softmax((ac + bd) / math.sqrt(DK), dim=-1)
    return (attn @ v).transpose(0, 1).reshape(n, HD)


def on_grid(t):
    """Multiples of 1/64 below 32 in magnitude: exact in fp16, and so are the sums q + u the fp16 kernel forms - its rounding then
    touches the probabilities only, and the float64 reference is a fair yardstick for it."""
    assert float(t.abs().max()) < 31.0
    return torch.round(t * 64.0) / 64.0


def head_direction(seed):
    e = torch.sign(rnd(HD, seed=seed))
    return e  # +-1 per channel: e_h . e_h = 48 in every head


def attention_inputs(family, rag, place=None):
    """qkv [rows, 576], ptab [2 pmax - 1, 192], bias_u, bias_v of one input family (see the test)."""
    R = rag.total_rows
    q, k, v = rnd(R, HD, seed=1, scale=0.7), rnd(R, HD, seed=2, scale=0.7), rnd(R, HD, seed=3, scale=0.7)
    ptab = rnd(2 * PMAX - 1, HD, seed=4, scale=0.5)
    bu, bv = rnd(HD, seed=5, scale=0.3), rnd(HD, seed=6, scale=0.3)
    e = head_direction(7)
    if family == "peaked":
        # one key per utterance scores 30 / 40 / 50 / 60 (heads 0..3) above the others: every query attends to it alone
        amp = torch.tensor([math.sqrt(s * math.sqrt(DK) / DK) for s in (30.0, 40.0, 50.0, 60.0)]).repeat_interleave(DK)
        q = 0.25 * q / 0.7 + amp * e
        k = 0.25 * k / 0.7
        ptab, bu, bv = 0.1 * ptab, 0.1 * bu, 0.1 * bv
        for b0, n in spans(rag):
            j = {"first": min(3, n - 1), "middle": n // 2, "last": n - 1}[place]
            k[b0 + j] += amp * e
    elif family == "rising":
        # scores rise by ~30 over the keys of every utterance: the running max moves in every key tile
        amp = math.sqrt(30.0 * math.sqrt(DK) / DK)
        q = 0.25 * q / 0.7 + amp * e
        k = 0.25 * k / 0.7
        for b0, n in spans(rag):
            k[b0:b0 + n] += amp * torch.linspace(0.0, 1.0, n, dtype=torch.float64).unsqueeze(1) * e
        ptab, bu, bv = 0.1 * ptab, 0.1 * bu, 0.1 * bv
    elif family == "position":
        # bd >> ac: a bias_v along e and table rows c_p * e with a random c_p per relative position (scores spread +-15 by p alone)
        q, k = 0.1 * q, 0.1 * k
        bv = bv + 2.0 * e
        ptab = 0.1 * ptab + rnd(2 * PMAX - 1, 1, seed=8, scale=0.5) * e
    else:
        assert family == "gentle"
    qkv = on_grid(torch.cat([q, k, v], 1))
    return qkv, on_grid(ptab), on_grid(bu), on_grid(bv)


@pytest.mark.parametrize("family,place", [("gentle", None), ("peaked", "first"), ("peaked", "middle"), ("peaked", "last"), ("rising", None),
                                          ("position", None)])
@pytest.mark.parametrize("form", list(ATT_FORMS))
def test_relpos_attention_vs_float64(ops, family, place, form):
    rag = Ragged(ATT_LENGTHS, ops.device, align=2)
    qkv, ptab, bu, bv = attention_inputs(family, rag, place)
    ctx = torch.zeros(rag.total_rows, HD, device=DEV)
    ops.attention(dev(qkv), dev(ptab), PMAX, dev(bu), dev(bv), ctx, rag, 128, **ATT_FORMS[form])
    torch.cuda.synchronize()
    tol = TOL[capi.COMPUTE_F16 if form == "f16" else capi.COMPUTE_F32]
    for b0, n in spans(rag):
        close(ctx[b0:b0 + n], attention_f64(qkv[b0:b0 + n], ptab, PMAX, bu, bv, n), tol, f"{n} rows:")


# ---------------------------------------------------------------------------------------------------------------------------
# Anti-aliased snake: every consumer with filters that are not the symmetric design
# ---------------------------------------------------------------------------------------------------------------------------
def filter_asymmetric():
    f = packing.kaiser_sinc_filter12().astype(np.float64) * (1.0 + 0.3 * np.linspace(-1.0, 1.0, 12))
    return (f / f.sum()).astype(np.float32)


def filter_stored():
    """The design as a checkpoint stores it (float64 -> fp32) with last-bit perturbations on three taps."""
    f = packing.kaiser_sinc_filter12().copy()
    for i, d in ((1, np.inf), (6, -np.inf), (9, np.inf)):
        f[i] = np.nextafter(f[i], np.float32(d))
    return f


FILTERS = {"asymmetric": filter_asymmetric, "stored": filter_stored, "design": packing.kaiser_sinc_filter12}


def test_the_test_filters_are_what_they_claim():
    fa, fs, fd = filter_asymmetric(), filter_stored(), packing.kaiser_sinc_filter12()
    assert np.abs(fa - fa[::-1]).max() > 1e-2 and abs(float(fa.astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.array_equal(fd, fd[::-1]) and not np.array_equal(fs, fd) and not np.array_equal(fs, fs[::-1])


def snake_f64(xu, alpha, beta, filt):
    """oracle.activation1d(SnakeBeta) in float64 on one utterance xu [T, C] -> [C, T]."""
    return oracle.activation1d(xu.t().contiguous(), lambda v: oracle.snake_beta(v, alpha, beta), filt)


def snake_params(c, seed):
    return rnd(c, seed=seed, scale=0.3).float().double(), rnd(c, seed=seed + 1, scale=0.3).float().double()


@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("c,lengths", [(32, [1000, 9, 1]), (256, [336, 1, 2, 70])])
def test_snake_aa_vs_float64(ops, filt, c, lengths):
    f = torch.from_numpy(FILTERS[filt]()).double()
    rag = Ragged(lengths, ops.device, align=2)
    x = rnd(rag.total_rows, c, seed=1).float().double()
    al, be = snake_params(c, 2)
    y = torch.zeros(rag.total_rows, c, device=DEV)
    ops.snake_aa(dev(x), y, dev(al), dev(be), dev(f), c, rag)
    torch.cuda.synchronize()
    for b0, n in spans(rag):
        close(y[b0:b0 + n], snake_f64(x[b0:b0 + n], al, be, f).t(), TOL[capi.COMPUTE_F32], f"{n} frames:")


@pytest.mark.parametrize("filt", list(FILTERS))
def test_conv_post_snake_vs_float64(ops, filt):
    """activation_post + conv_post (7 taps, one output channel) + tanh: BigVGAN's last two ops."""
    c, lengths = 32, [251, 1, 2, 499]
    f = torch.from_numpy(FILTERS[filt]()).double()
    rag = Ragged(lengths, ops.device)
    x = rnd(rag.total_rows, c, seed=1).float().double()
    al, be = snake_params(c, 2)
    w = rnd(7, c, seed=4, scale=0.1).float().double()  # [tap, channel]
    bias = 0.05
    wav = torch.full((rag.total_rows,), 9.0, device=DEV)
    ops.conv_post_snake(dev(x), c, dev(w), bias, dev(al), dev(be), dev(f), wav, rag)
    torch.cuda.synchronize()
    for b0, n in spans(rag):
        t = snake_f64(x[b0:b0 + n], al, be, f).unsqueeze(0)
        want = torch.tanh(F.conv1d(t, w.t().unsqueeze(0), torch.tensor([bias], dtype=torch.float64), padding=3))[0, 0]
        close(wav[b0:b0 + n], want, TOL[capi.COMPUTE_F32], f"{n} frames:")


@pytest.mark.parametrize("filt", ["asymmetric", "stored"])
@pytest.mark.parametrize("compute", [capi.COMPUTE_F32, capi.COMPUTE_BF16, capi.COMPUTE_F16])
@pytest.mark.parametrize("c,k,dil,lengths", [(32, 3, 1, [1000, 9, 1]), (128, 11, 5, [260, 33]), (256, 7, 3, [130, 1, 2])])
def test_conv1d_pre_snake_vs_float64(ops, filt, compute, c, k, dil, lengths):
    """TTS_PRE_SNAKE: the conv's input staging applies Activation1d(SnakeBeta), then the conv and a residual.
    (fp32: 3e-5, the c * k products on top of the snake, as the emulator test allows.)"""
    f = torch.from_numpy(FILTERS[filt]()).double()
    w = rnd(c, c, k, seed=1, scale=1.0 / np.sqrt(c * k)).float().double()
    b = rnd(c, seed=2, scale=0.1).float().double()
    rag = Ragged(lengths, ops.device, align=2)
    R = rag.total_rows
    x, res = rnd(R, c, seed=3).float().double(), rnd(R, c, seed=5).float().double()
    al, be = snake_params(c, 6)
    cw = packing.pack_conv(w.float().numpy(), b.float().numpy(), ops.device, dil=dil, bf16=PACK16[compute])
    y = torch.zeros(R, c, device=DEV)
    ops.conv(cw, dev(x), y, rag, pre=capi.PRE_SNAKE, snake=(dev(al), dev(be), dev(f)), res=dev(res), compute=compute)
    torch.cuda.synchronize()
    for b0, n in spans(rag):
        t = snake_f64(x[b0:b0 + n], al, be, f).unsqueeze(0)
        want = F.conv1d(t, w, b, padding=(k - 1) // 2 * dil, dilation=dil)[0].t() + res[b0:b0 + n]
        close(y[b0:b0 + n], want, 3e-5 if compute == capi.COMPUTE_F32 else TOL[compute], f"{n} frames:")


RB_CASES = [(32, 11, 5, [700, 30, 1]), (64, 7, 3, [224, 449, 1]), (128, 3, 1, [500, 17]), (256, 11, 5, [130, 96, 1])]


@pytest.mark.parametrize("filt", ["asymmetric", "stored"])
@pytest.mark.parametrize("compute", [capi.COMPUTE_BF16, capi.COMPUTE_F16])
@pytest.mark.parametrize("c,k,dil,lengths", RB_CASES)
def test_resblock_step_snake_vs_float64(ops, filt, compute, c, k, dil, lengths):
    """One AMP dilation step y = c2(a2(c1(a1(x)))) + x: C <= 128 runs the snakes' FIR filters on the matrix cores (the table
    tts_snake_fir_table builds from the filter), C = 256 in the VALU form."""
    f = torch.from_numpy(FILTERS[filt]()).double()
    w1 = rnd(c, c, k, seed=1, scale=1.0 / np.sqrt(c * k)).float().double()
    w2 = rnd(c, c, k, seed=2, scale=1.0 / np.sqrt(c * k)).float().double()
    b1, b2 = rnd(c, seed=3, scale=0.1).float().double(), rnd(c, seed=4, scale=0.1).float().double()
    (a1, be1), (a2, be2) = snake_params(c, 7), snake_params(c, 9)
    rag = Ragged(lengths, ops.device, align=2)
    x = rnd(rag.total_rows, c, seed=5).float().double()
    c1 = packing.pack_conv(w1.float().numpy(), b1.float().numpy(), ops.device, dil=dil, bf16=PACK16[compute])
    c2 = packing.pack_conv(w2.float().numpy(), b2.float().numpy(), ops.device, dil=1, bf16=PACK16[compute])
    y = torch.zeros(rag.total_rows, c, device=DEV)
    fd = dev(f)
    ops.resblock_step(c1, c2, dev(x), y, rag, capi.PRE_SNAKE, 0.1, (dev(a1), dev(be1)), (dev(a2), dev(be2)), fd,
                      fir_tab=packing.snake_fir_table(FILTERS[filt](), ops.device))
    torch.cuda.synchronize()
    for b0, n in spans(rag):
        t = F.conv1d(snake_f64(x[b0:b0 + n], a1, be1, f).unsqueeze(0), w1, b1, padding=(k - 1) // 2 * dil, dilation=dil)
        t = oracle.activation1d(t[0], lambda v: oracle.snake_beta(v, a2, be2), f).unsqueeze(0)
        want = F.conv1d(t, w2, b2, padding=(k - 1) // 2)[0].t() + x[b0:b0 + n]
        close(y[b0:b0 + n], want, TOL[compute], f"{n} frames:")


def test_resblock_step_valu_snake_form_vs_float64():
    """TOUCAN_SNAKE_VALU=1 (read once per process by the library) keeps the C <= 128 residual steps on the register-streamed VALU
    snake: the same tests in a fresh child process with the variable set."""
    env = dict(os.environ, TOUCAN_SNAKE_VALU="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
           "-k", "test_resblock_step_snake_vs_float64 and not 256-"]
    r = subprocess.run(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " passed" in r.stdout and "12 passed" in r.stdout, r.stdout[-2000:]
