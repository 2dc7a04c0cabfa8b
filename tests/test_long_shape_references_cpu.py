"""The yardsticks of tests/test_gpu_kernels_long_shapes.py, checked without a GPU - a loose reference must not hide a kernel error:

* the float32 MAS restatement (aligner_ref.mas, log64) scores within 1e-6 relative of the float64 Viterbi optimum on that module's shapes;
* scorer_ref.ctc_loss agrees with torch's float64 CTC within 1e-7 relative on that module's shapes;
* the duration head's fp32 reference differs from the correctly rounded float64 value only next to a half, on at most 80 of 4096 inputs;
* no duration product of the prosody-control case lies within 1e-3 of a half;
* the length-regulator and Glow references reproduce a tiny case worked out by hand.

Then the numpy ABI emulator runs the sequence kernels' cases (length regulator, prosody control, duration head, Glow mix, depthwise
conv) at the same shapes under the same assertions as the kernels: the emulator stands in for the library in the other CPU tests,
and its own loops had not run past 33 phonemes either."""
import math

import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import engine
from tests import abi_emulator
from tests import long_shape_cases as lc


@pytest.fixture(scope="module")
def emu():
    return engine.Ops("cpu", lib=abi_emulator.Emulator())


TO = lc.mover("cpu")


# ---- the references themselves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(lc.MAS_SHAPES)), ids=[f"{t}x{l}" for t, l in lc.MAS_SHAPES])
def test_mas_restatement_reaches_the_float64_optimum(i):
    c = lc.mas_case(i)
    T, L = lc.MAS_SHAPES[i]
    assert c.dur.sum() == T and len(c.dur) == L and (c.dur >= 1).all()
    gap = lc.mas_rel_gap(c.score, c.optimum)
    print(f"MAS {T} x {L}: restatement {c.score:.9f}, optimum {c.optimum:.9f}, relative gap {gap:.2e}")
    assert c.score <= c.optimum + 1e-9 * abs(c.optimum) and gap <= lc.MAS_REL


def test_viterbi_optimum_on_a_case_enumerated_by_hand():
    """T = 3, L = 2: the paths are (token 0, 0, 1) and (0, 1, 1)."""
    p = [[0.0, 9.0], [1.0, 2.0], [5.0, 0.5]]
    off = 9.0 + 1.0
    a = [[math.log(v + off) for v in row] for row in p]
    want = a[0][0] + max(a[1][0], a[1][1]) + a[2][1]
    assert abs(lc.viterbi_optimum_f64(p) - want) <= 1e-12
    assert abs(lc.ar.mas_float64_score(p, [1, 2]) - want) <= 1e-12  # (0, 1, 1) is the better one: log 12 > log 11


@pytest.mark.parametrize("i", range(len(lc.CTC_SHAPES)), ids=[f"{t}x{n}" for t, n in lc.CTC_SHAPES])
def test_ctc_restatement_against_torch_float64(i):
    c = lc.ctc_case(i)
    T, n = lc.CTC_SHAPES[i]
    if T < n:
        assert c.ref32 == 0.0 and c.ref64 == 0.0
        return
    rel = abs(c.ref32 - c.ref64) / abs(c.ref64)
    print(f"CTC {T} x {n}: restatement {c.ref32:.9f}, torch float64 {c.ref64:.9f}, relative difference {rel:.2e}")
    assert c.ref64 > 0.0 and rel <= 1e-7


def test_duration_reference_is_excused_only_next_to_a_half():
    c = lc.duration_case()
    n_near = int(c.near_half.sum())
    wrong = c.want != c.exact
    print(f"duration head: {n_near} of {lc.DUR_N} inputs lie next to a half; the fp32 reference rounds {int(wrong.sum())} of them the other way")
    assert 64 <= n_near <= lc.DUR_EXCUSED_MAX and bool(c.near_half[-64:].all())
    assert not bool((wrong & ~c.near_half).any())
    assert c.want[-67:-64].tolist() == [0, 1000000, 1000000] and int(c.want.min()) == 0  # both clamps


@pytest.mark.parametrize("scales", lc.PC_SCALES)
def test_prosody_durations_stay_clear_of_a_half(scales):
    assert lc.prosody_half_distance(scales) > 1e-3
    c = lc.prosody_case()
    assert int(((c.text[:, lc.oracle.F_SILENCE] == 1) & (c.dur > 0)).sum()) > 50  # (the pause product is exercised)


def test_length_regulator_reference_by_hand():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    enc = torch.tensor([[1.0, 10.0], [2.0, 20.0], [3.0, 30.0]], dtype=torch.float64)
    args = (enc, t(1.0, 0.0, -1.0), t(0.0, 2.0, 0.0), t(0.5, 1.0), t(0.25, 0.0), t(1.0, -1.0), t(0.0, 0.5))
    # row p: enc + (pitch * wp + bp) + (energy * we + be)
    rows = [[1.0 + 0.75 + 0.0, 10.0 + 1.0 + 0.5], [2.0 + 0.25 + 2.0, 20.0 + 0.0 - 1.5], [3.0 - 0.25 + 0.0, 30.0 - 1.0 + 0.5]]
    got = lc.length_regulate_f64(*args, torch.tensor([2, 0, 1]))
    assert got.tolist() == [rows[0], rows[0], rows[2]]
    assert lc.length_regulate_f64(*args, torch.tensor([0, 0, 0])).tolist() == rows  # all zero: all ones


def test_glow_reference_by_hand():
    """c = 8: group 0 mixes channels (0, 1, 4, 5), group 1 channels (2, 3, 6, 7)."""
    x = torch.arange(1.0, 9.0, dtype=torch.float64).reshape(1, 8)
    w = torch.tensor([1.0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 1, 1], dtype=torch.float64)
    zero = torch.zeros(8, dtype=torch.float64)
    assert lc.glow_mix_f64(x, w, zero, zero).tolist() == [[1.0, 5.0, 3.0, 7.0, 2.0, 14.0, 4.0, 22.0]]
    bias, logs = zero.clone(), zero.clone()
    bias[5], logs[5] = 1.0, math.log(2.0)
    got = lc.glow_mix_f64(x, w, bias, logs)
    assert abs(float(got[0, 5]) - 6.5) <= 1e-12 and got[0, :5].tolist() == [1.0, 5.0, 3.0, 7.0, 2.0]


# ---- the emulator at the same shapes ----------------------------------------------------------------------------------------
def test_emulator_length_regulator(emu):
    err = lc.check_length_regulate(*lc.run_length_regulate(emu, TO))
    print(f"emulator length regulator: {err:.2e}")


@pytest.mark.parametrize("scales", lc.PC_SCALES)
def test_emulator_prosody_control(emu, scales):
    err = lc.check_prosody(*lc.run_prosody(emu, TO, scales), scales)
    print(f"emulator prosody control {scales}: {err:.2e}")


@pytest.mark.filterwarnings("ignore:overflow encountered in exp")  # (exp(89) is meant to overflow: the upper clamp)
def test_emulator_duration_head(emu):
    print(f"emulator duration head: {lc.check_duration(lc.run_duration(emu, TO))} mismatches next to a half")


@pytest.mark.parametrize("rows,pad", [(77, 0), (13107, 0), (13108, 16), (14000, 0)])
def test_emulator_glow_mix(emu, rows, pad):
    print(f"emulator glow mix: {lc.check_glow(lc.run_glow(emu, TO, rows, pad), rows):.2e}")


@pytest.mark.parametrize("k,c,family", lc.DW_CASES)
def test_emulator_dwconv_swish(emu, k, c, family):
    print(f"emulator dwconv: {lc.check_dwconv(lc.run_dwconv(emu, TO, k, c, family), k, c, family):.2e}")
