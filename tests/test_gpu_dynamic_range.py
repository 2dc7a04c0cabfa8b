"""The 16-bit kernels held to their rounding model over the dynamic range (tests/dynamic_range.py; DESIGN.md, "The 16-bit kernels over
the dynamic range"): tests/test_gpu_error_budget.py's comparison - g the kernel on the MI355X, e tests/abi_emulator.py with the
options the case names, r the float64 restatement - at the levels of tests/error_budget_cases.py: every additive input times
2^-22, 2^-18, 2^-14, 2^12 and one octave under the model's last finite scale, and the snakes' log alpha raised by 2 and by 4.
Checks (a) and (b) as at unit scale with the level's own margin, (c) and (d) in the model's own units, (e) the output is finite,
(f) the homogeneous bf16 kernels only scale.  The levels' conditions are checked without a GPU in tests/test_dynamic_range_cpu.py.

The fp32 snake kernels (one hardware sine of a phase reduced in fp32, csrc/snake.h) run against the float64 restatement at the same
two sharpnesses, inside a bound derived from the phase arithmetic (dynamic_range.snake_sine_bound)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import engine
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import abi_emulator, dynamic_range as dr, error_budget as eb, error_budget_cases as ec
from tests import test_gpu_kernels_vs_float64 as vs64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ops = engine.Ops("cuda:0")
    assert not isinstance(ops.lib, abi_emulator.Emulator)
    return ops


@pytest.mark.parametrize("case,fmt,level", ec.level_ids(), ids=lambda v: ec.level_id(v) if isinstance(v, tuple) else str(v))
def test_kernel_spends_its_error_budget_at_the_level(gpu, case, fmt, level):
    lengths, cls = dr.shape(case, fmt)
    eb.check_conditions(case.name, cls, case.channels, case.classes)
    inp, r, e = dr.model_run(case, fmt, level)
    assert np.isfinite(e).all(), "no GPU level lies where the model is not finite"
    g = ec.run_live(case, gpu, fmt, inp, lengths)
    rep = dr.evaluate(case, fmt, level, g, e, r, ec.level_margin(case, fmt, level))
    print(rep.line())
    assert rep.ok, "over the error budget: " + rep.message()


@pytest.mark.parametrize("name", ec.HOMOGENEOUS_CASES)
def test_homogeneous_bf16_kernel_only_scales(gpu, name):
    """(f) lrelu, the products with bf16 weights, fp32 sums and bf16 roundings all commute with a power of two: the kernel's output at
    2^-14 and at 2^12 is its unit-level output times the scale, bit for bit."""
    case = ec.BY_NAME[name]
    lengths, _ = dr.shape(case, "bf16")
    out = {k: ec.run_live(case, gpu, "bf16", case.inputs("bf16", 0, lengths, (k, 0)), lengths) for k in (0, -14, 12)}
    for k in (-14, 12):
        off = out[k] != 2.0 ** k * out[0]
        assert not off.any(), f"{name} at 2^{k}: {int(off.sum())} of {off.size} elements are not 2^{k} x the unit-level output"


# -----------------------------------------------------------------------------------------------------------------------------------
# the fp32 snake's hardware sine at sharp alphas
# -----------------------------------------------------------------------------------------------------------------------------------
def sharp_snake_inputs(rows, c, da):
    x = vs64.rnd(rows, c, seed=1).float().double()
    al, be = vs64.snake_params(c, 2)
    return x, (al + da).float().double(), be


@pytest.mark.parametrize("da", ec.LEVEL_DA)
@pytest.mark.parametrize("filt", list(vs64.FILTERS))
def test_snake_aa_sharp_alpha_vs_float64(gpu, filt, da):
    """tts_snake_aa (C = 32, lengths [1000, 9, 1]) with log alpha raised by `da` (phases of some tens and some hundreds of radians),
    element by element: |y - y_float64| <= F32_TOL max(1, max |y_float64|) + dynamic_range.snake_sine_bound, whose docstring
    derives the second term from the phase's two fp32 roundings, the fp32 error of h and a sine good to 2e-6."""
    c, lengths = 32, [1000, 9, 1]
    f = torch.from_numpy(vs64.FILTERS[filt]()).double()
    rag = Ragged(lengths, gpu.device, align=2)
    x, al, be = sharp_snake_inputs(rag.total_rows, c, da)
    y = torch.zeros(rag.total_rows, c, device=gpu.device)
    gpu.snake_aa(vs64.dev(x), y, vs64.dev(al), vs64.dev(be), vs64.dev(f), c, rag)
    torch.cuda.synchronize()
    y = y.cpu().double().numpy()
    worst = 0.0
    for b0, n in vs64.spans(rag):
        want = vs64.snake_f64(x[b0:b0 + n], al, be, f).t().numpy()
        tol = dr.F32_TOL * max(1.0, float(np.abs(want).max())) + dr.snake_sine_bound(x[b0:b0 + n].numpy(), al.numpy(), be.numpy(), f.numpy())
        worst = max(worst, float((np.abs(y[b0:b0 + n] - want) / tol).max()))
    print(f"snake_aa {filt} log alpha {da:+d}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("da", ec.LEVEL_DA)
@pytest.mark.parametrize("filt", list(vs64.FILTERS))
def test_conv_post_snake_sharp_alpha_vs_float64(gpu, filt, da):
    """tts_conv_post_snake with log alpha raised by `da`: the snake's bound (test_snake_aa_sharp_alpha_vs_float64) through the 7-tap
    conv, sum over taps and channels of |w| x bound (tanh has slope at most 1), beside F32_TOL."""
    c, lengths = 32, [251, 1, 2, 499]
    f = torch.from_numpy(vs64.FILTERS[filt]()).double()
    rag = Ragged(lengths, gpu.device)
    x, al, be = sharp_snake_inputs(rag.total_rows, c, da)
    w = vs64.rnd(7, c, seed=4, scale=0.1).float().double()  # [tap, channel]
    bias = 0.05
    wav = torch.full((rag.total_rows,), 9.0, device=gpu.device)
    gpu.conv_post_snake(vs64.dev(x), c, vs64.dev(w), bias, vs64.dev(al), vs64.dev(be), vs64.dev(f), wav, rag)
    torch.cuda.synchronize()
    wav = wav.cpu().double().numpy()
    worst = 0.0
    for b0, n in vs64.spans(rag):
        t = vs64.snake_f64(x[b0:b0 + n], al, be, f).unsqueeze(0)
        want = torch.tanh(F.conv1d(t, w.t().unsqueeze(0), torch.tensor([bias], dtype=torch.float64), padding=3))[0, 0].numpy()
        snake = torch.from_numpy(dr.snake_sine_bound(x[b0:b0 + n].numpy(), al.numpy(), be.numpy(), f.numpy()))
        through = F.conv1d(snake.t().unsqueeze(0), w.abs().t().unsqueeze(0), padding=3)[0, 0].numpy()
        worst = max(worst, float((np.abs(wav[b0:b0 + n] - want) / (dr.F32_TOL + through)).max()))
    print(f"conv_post_snake {filt} log alpha {da:+d}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
