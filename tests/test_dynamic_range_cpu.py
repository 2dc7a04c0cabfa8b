"""The levels of the error-budget cases (tests/error_budget_cases.py, tests/dynamic_range.py) on the CPU: nothing here trusts a table.

* The unit level (0, 0) reproduces the inputs every case had before there were levels, on one case per kernel family.
* RANGE_TABLE is what the sweep gives: k_top, k_floor, da_top, da_2x exactly, every recorded E_e / rms(r) to 1 %.
* LEVEL_SPREAD is what 8 seeds give (to 1e-3); at every GPU level the model is finite in all 8, the conditions of
  eb.check_conditions hold and every stratum has a budget (E_e > 0).
* The homogeneous bf16 cases only scale: the plain model's e at every level is 2^k x the unit-level e, bit for bit.
* Two mutants of the stand-in kernel (tests/error_budget_standin.py) that are invisible at unit scale - 16-bit conversions that
  flush fp16 subnormals, a snake phase taken from the 16-bit u - pass (a) to (c) at the unit level and fail where RANGE_MUTANT_FAILS
  says; the stand-in itself passes at every level.
* The fp32 snake of csrc/snake.h restated in fp32 numpy with an exact sine stays inside dynamic_range.snake_sine_bound without its
  sine term, at log alpha + 0, 2, 4: worst |err| / bound 0.20 (log alpha + 4, stored filter).
"""
import math

import numpy as np
import pytest
import torch

from ims_toucan_prosody_variance_amd import capi
from tests import dynamic_range as dr, error_budget as eb, error_budget_cases as ec, error_budget_standin as standin
from tests import test_gpu_kernels_vs_float64 as vs64

ids = lambda v: ec.level_id(v) if isinstance(v, tuple) else str(v)


# -----------------------------------------------------------------------------------------------------------------------------------
# the unit level is today's draw
# -----------------------------------------------------------------------------------------------------------------------------------
def _draw_before_levels(case, fmt, seed, lengths):
    """The inputs of one case per family as tests/error_budget_cases.py drew them before it knew levels, restated."""
    rnd, s, R, dt = ec.rnd, 100 * seed, ec.layout(lengths).total_rows, ec.DT16[fmt]
    if isinstance(case, ec.ConvCase):
        cin, cout = case.cin, case.cout
        out = dict(w=rnd(cout, cin, case.k, seed=1, scale=1.0 / math.sqrt(cin * case.k)).float(), b=rnd(cout, seed=2, scale=0.1).float(),
                   x=rnd(R, cin, seed=s + 3).float(), res=rnd(R, case.channels, seed=s + 5).float(),
                   preadd=rnd(R, cout, seed=s + 6, scale=0.5).float())
        assert case.preadd and not case.io16 and case.pre == capi.PRE_NONE
        return out
    if isinstance(case, ec.ResblockCase):
        c, k = case.c, case.k
        assert case.io16
        return dict(w1=rnd(c, c, k, seed=1, scale=1.0 / math.sqrt(c * k)).float(), w2=rnd(c, c, k, seed=2, scale=1.0 / math.sqrt(c * k)).float(),
                    b1=rnd(c, seed=3, scale=0.1).float(), b2=rnd(c, seed=4, scale=0.1).float(), x=rnd(R, c, seed=s + 5).to(dt),
                    a1=rnd(c, seed=7, scale=0.3).float(), be1=rnd(c, seed=8, scale=0.3).float(),
                    a2=rnd(c, seed=9, scale=0.3).float(), be2=rnd(c, seed=10, scale=0.3).float(),
                    filt=torch.from_numpy(np.ascontiguousarray(vs64.FILTERS[case.filt]())))
    if isinstance(case, ec.WavenetCase):
        H = case.H
        return dict(w_in=rnd(2 * H, H, 5, seed=1, scale=1.0 / math.sqrt(5 * H)).float(), b_in=rnd(2 * H, seed=2, scale=0.1).float(),
                    w_rs=rnd(case.cout2, H, 1, seed=3, scale=1.0 / math.sqrt(H)).float(), b_rs=rnd(case.cout2, seed=4, scale=0.1).float(),
                    hs=rnd(R, 2 * H, seed=s + 5).float(), cond=rnd(R, 8 * H, seed=s + 6, scale=0.5).float())
    if isinstance(case, ec.FfnCase):
        C, hid = 192, case.hidden
        return dict(w1=rnd(hid, C, 1, seed=1, scale=1.0 / math.sqrt(C)).float(), b1=rnd(hid, seed=2, scale=0.1).float(),
                    w2=rnd(C, hid, 1, seed=3, scale=1.0 / math.sqrt(hid)).float(), b2=rnd(C, seed=4, scale=0.1).float(),
                    x=rnd(lengths[0], C, seed=s + 5, scale=2.0).float(),
                    g=(1.0 + rnd(C, seed=6, scale=0.1)).float(), b=rnd(C, seed=7, scale=0.1).float(),
                    pg=(1.0 + rnd(C, seed=8, scale=0.1)).float(), pb=rnd(C, seed=9, scale=0.1).float())
    with ec._seeds_shifted(100 * seed):
        qkv, ptab, bu, bv = vs64.attention_inputs(case.family, ec.layout(lengths), case.place)
    return dict(qkv=qkv.float(), ptab=ptab.float(), bu=bu.float(), bv=bv.float())


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("name", ["conv small gated 192>2x192 k5 preadd", "resblock mfma snake 32 k3 16-bit stream", "wavenet layer cout2 384",
                                  "ffn 1536 post 300 rows", "attention gentle [129, 31, 33]"])
def test_unit_level_reproduces_the_inputs_bit_for_bit(name, seed):
    case = ec.BY_NAME[name]
    for fmt in case.formats:
        lengths = [5, 2, 40] if case.fixed_lengths is None else case.fixed_lengths
        want = _draw_before_levels(case, fmt, seed, lengths)
        for got in (case.inputs(fmt, seed, lengths), case.inputs(fmt, seed, lengths, ec.UNIT_LEVEL)):
            assert set(got) == set(want)
            for key in want:
                assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), (name, fmt, key)


def test_a_level_scales_the_additive_inputs_and_nothing_else():
    for name, scaled in (("conv snake 128>128 k11 d5 asymmetric", {"x", "res", "b"}), ("resblock valu snake 256 k3 16-bit stream", {"x", "b1", "b2"}),
                         ("wavenet layer cout2 384", {"hs", "cond", "b_in", "b_rs"}), ("ffn 1536 post 300 rows", {"x"})):
        case = ec.BY_NAME[name]
        lengths = [5, 2] if case.fixed_lengths is None else case.fixed_lengths
        unit, lv = case.inputs("bf16", 1, lengths), case.inputs("bf16", 1, lengths, (-3, 2))
        for key in unit:
            if key in scaled:
                assert torch.equal(lv[key].double(), unit[key].double() / 8.0), (name, key)  # (a power of two: exact in every format)
            elif key in ("alpha", "a1", "a2"):
                assert torch.allclose(lv[key], unit[key] + 2.0, atol=1e-6, rtol=0) and not torch.equal(lv[key], unit[key])
            else:
                assert torch.equal(lv[key], unit[key]), (name, key)
    att = ec.BY_NAME["attention gentle [129, 31, 33]"]
    unit, lv = att.inputs("f16", 0, [9, 4]), att.inputs("f16", 0, [9, 4], (5, 0))
    assert torch.equal(lv["qkv"][:, :2 * vs64.HD], unit["qkv"][:, :2 * vs64.HD]) and torch.equal(lv["qkv"][:, 2 * vs64.HD:], 32.0 * unit["qkv"][:, 2 * vs64.HD:])


# -----------------------------------------------------------------------------------------------------------------------------------
# the tables
# -----------------------------------------------------------------------------------------------------------------------------------
def test_the_tables_cover_the_levels_and_nothing_else():
    assert set(ec.LEVEL_SPREAD) == {(c.name, f, lv) for c, f, lv in ec.level_ids()}
    rows = {(c.name, f, "kernel") for c, f in ec.level_case_ids()} | {(c.name, f, "plain") for c, f in ec.level_case_ids() if ec.level_model(c)}
    assert set(ec.RANGE_TABLE) == rows
    assert set(ec.LEVEL_MODEL) <= set(ec.LEVEL_CASES) and set(ec.HOMOGENEOUS_CASES) <= set(ec.LEVEL_CASES)
    for c, f in ec.level_case_ids():
        lv = ec.levels(c, f)
        top = ec.RANGE_TABLE[(c.name, f, "kernel")]["k_top"]
        assert len(set(lv)) == len(lv) and {(k, 0) for k in ec.LEVEL_K} <= set(lv) and (top - 1, 0) in lv
        assert all(k < top for k, _ in lv), "every GPU level lies under the model's last finite scale"
        assert ((0, 2) in lv and (0, 4) in lv) == (c.name in ec.SNAKE_LEVEL_CASES)


@pytest.mark.parametrize("key", list(ec.RANGE_TABLE), ids=lambda k: " / ".join(k))
def test_range_table_is_what_the_sweep_gives(key):
    name, fmt, which = key
    got = dr.table_row(ec.BY_NAME[name], fmt, {} if which == "kernel" else dr.PLAIN)
    want = ec.RANGE_TABLE[key]
    print(got)
    assert set(got) == set(want)
    for field in ("k_top", "k_floor", "da_top", "da_2x"):
        assert got.get(field) == want.get(field), field
    assert set(got["rel"]) == set(want["rel"])
    for k in want["rel"]:
        assert abs(got["rel"][k] - want["rel"][k]) <= 0.01 * want["rel"][k], (k, got["rel"][k], want["rel"][k])
    for a, b in zip(got.get("rel_da", []), want.get("rel_da", [])):
        assert abs(a - b) <= 0.01 * b, (a, b)
    assert len(got.get("rel_da", [])) == len(want.get("rel_da", []))


@pytest.mark.parametrize("case,fmt,level", ec.level_ids(), ids=ids)
def test_level_spread_and_conditions(case, fmt, level):
    lengths, cls = dr.shape(case, fmt)
    eb.check_conditions(case.name, cls, case.channels, case.classes)
    s, (r, e) = dr.level_spread(case, fmt, level)  # asserts: finite in all 8 seeds, E_e > 0
    rep = dr.evaluate(case, fmt, level, e, e, r, 0.10)  # asserts E_e > 0 in every stratum
    assert rep.ok, rep.message()
    print(f"{case.name} {ec.level_id(level)} [{fmt}]: s = {s:.4f}, m = {eb.margin(s):.3f}, E_e / rms(r) = {rep.rel_budget:.3e}")
    assert abs(s - ec.LEVEL_SPREAD[(case.name, fmt, level)]) <= 1e-3, f"s = {s:.4f}, the table says {ec.LEVEL_SPREAD[(case.name, fmt, level)]:.4f}"


@pytest.mark.parametrize("name", ec.HOMOGENEOUS_CASES)
def test_the_levels_only_scale(name):
    """bf16 and fp32 roundings commute with a power of two while nothing is subnormal in fp32: the level machinery adds nothing."""
    case = ec.BY_NAME[name]
    assert not ec.level_model(case)
    unit = dr.model_run(case, "bf16", ec.UNIT_LEVEL)[2]
    for k, da in ec.levels(case, "bf16"):
        e = dr.model_run(case, "bf16", (k, da))[2]
        assert np.array_equal(e, 2.0 ** k * unit), (name, k)


# -----------------------------------------------------------------------------------------------------------------------------------
# the test of the test: mutants that only a level shows
# -----------------------------------------------------------------------------------------------------------------------------------
STEP = ec.ResblockCase("snake + conv step 32 k3 (valu model)", 32, 3, 1, capi.PRE_SNAKE)  # (tests/test_error_budget_cpu.py's third stand-in case)
MFMA_STEP = ec.BY_NAME["resblock mfma snake 32 k3 16-bit stream"]                           # (the matrix-core snake's model, its fp16 images flushing)
STANDIN_CASES = [ec.BY_NAME["conv regular linear 192>256 k5"], ec.BY_NAME["wavenet layer cout2 384"], STEP, MFMA_STEP]
STANDIN_MARGIN = 0.10
# mutant -> (the level at which it must fail, the (case, format) pairs it is tried on).  Measured E_g / E_e there:
#   flush_subnormals  2^-14: 1200 (conv, WaveNet layer, step; fp16), 184 (matrix-core step, bf16), 741 (the same, fp16); unit level 1.0000
#   phase_from_16bit  log alpha + 4: 4.1 (bf16), 15.3 (fp16); log alpha + 2: 2.5; unit level 1.044 / 1.053 (worst stratum 1.067)
RANGE_MUTANT_FAILS = {
    "flush_subnormals": ((-14, 0), [(c, "f16") for c in STANDIN_CASES] + [(MFMA_STEP, "bf16")]),
    "phase_from_16bit": ((0, 4), [(STEP, "bf16"), (STEP, "f16")]),
}


def standin_levels(case):
    return [ec.UNIT_LEVEL] + [(k, 0) for k in ec.LEVEL_K] + ([(0, da) for da in ec.LEVEL_DA] if "snake" in case.name else [])


def standin_report(case, fmt, level, mutant):
    _, r, e = dr.model_run(case, fmt, level)
    g = dr.model_run(case, fmt, level, lib_class=standin.StandIn, mutant=mutant)[2]
    return dr.evaluate(case, fmt, level, g, e, r, STANDIN_MARGIN, name=f"{case.name} {ec.level_id(level)} / {mutant or 'stand-in'}")


@pytest.mark.parametrize("fmt", ("bf16", "f16"))
@pytest.mark.parametrize("case", STANDIN_CASES, ids=str)
def test_standin_passes_at_every_level(case, fmt):
    for level in standin_levels(case):
        rep = standin_report(case, fmt, level, None)
        print(rep.line())
        assert rep.ok, rep.message()


@pytest.mark.parametrize("mutant", list(RANGE_MUTANT_FAILS))
def test_range_mutant_passes_at_unit_scale_and_fails_at_its_level(mutant):
    level, where = RANGE_MUTANT_FAILS[mutant]
    for case, fmt in where:
        unit = standin_report(case, fmt, ec.UNIT_LEVEL, mutant)
        print(unit.line())
        assert not ({"a", "b", "c"} & set(unit.failed)), unit.message()
        rep = standin_report(case, fmt, level, mutant)
        print(rep.message())
        assert "a" in rep.failed and "b" in rep.failed, f"{standin.RANGE_MUTANTS[mutant]} passes at {ec.level_id(level)}: {rep.line()}"


def test_every_range_mutant_is_tried():
    assert set(RANGE_MUTANT_FAILS) == set(standin.RANGE_MUTANTS) and not set(standin.RANGE_MUTANTS) & set(standin.MUTANTS)


# -----------------------------------------------------------------------------------------------------------------------------------
# the fp32 snake's phase arithmetic
# -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("da", (0,) + ec.LEVEL_DA)
@pytest.mark.parametrize("filt", list(vs64.FILTERS))
def test_fp32_snake_with_an_exact_sine_stays_inside_the_bound(filt, da):
    """The bound of tests/test_gpu_dynamic_range.py's sine tests without its sine term holds for csrc/snake.h's arithmetic in numpy:
    what is left for the hardware sine is the 2e-6 the bound grants it."""
    f = vs64.FILTERS[filt]()
    worst = 0.0
    for T in (1000, 9, 1):
        x = vs64.rnd(T, 32, seed=T).float().double()
        al, be = vs64.snake_params(32, 2)
        al = (al + da).float().double()
        want = vs64.snake_f64(x, al, be, torch.from_numpy(f).double()).t().numpy()
        got = dr.snake_fp32_exact_sine(x.numpy(), al.numpy(), be.numpy(), f).astype(np.float64)
        tol = dr.F32_TOL * max(1.0, float(np.abs(want).max())) + dr.snake_sine_bound(x.numpy(), al.numpy(), be.numpy(), f, sine_err=0.0)
        worst = max(worst, float((np.abs(got - want) / tol).max()))
    print(f"{filt} log alpha {da:+d}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
    with_sine = dr.snake_sine_bound(x.numpy(), al.numpy(), be.numpy(), f)
    assert (with_sine > dr.snake_sine_bound(x.numpy(), al.numpy(), be.numpy(), f, sine_err=0.0)).all()
