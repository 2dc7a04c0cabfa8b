"""The test of the error-budget test (tests/error_budget.py), on the CPU.

* A stand-in kernel (tests/error_budget_standin.py: the rounding model with fp32 accumulation in 16-channel k-steps, tap-major)
  passes checks (a) to (c) for the conv, the WaveNet layer and the snake + conv step, in both formats.
* Six mutants of it each fail the check named in MUTANT_FAILS (one of them in fp16 only: BELOW_THE_BUDGET) - and the assertion the
  16-bit kernel tests ended in until now (max |g - r| <= TOL max(1, max |r|)) accepts every one that does not put whole wrong
  samples into a sum: OLD_CHECK_REJECTS lists what it catches.
* The conditions of every GPU case (tests/error_budget_cases.py) hold: every row class and channel block holds N_MIN elements, at
  most a quarter of the cells fall below it, every stratum has a budget (E_e > 0), the lengths hold 1, 2 and both sides of a
  tile boundary, and the seed spread s is the one written in the table.
"""
import functools

import numpy as np
import pytest

from ims_toucan_prosody_variance_amd import capi
from tests import abi_emulator, error_budget as eb, error_budget_cases as ec, error_budget_standin as standin

FORMATS = ("bf16", "f16")

# The three kernels of the stand-in: two cases of the GPU table, and the snake + conv step in the form whose rounding points are the
# stand-in's (the VALU snake, which the GPU table runs at C = 256) at 32 channels.
STANDIN_CASES = [
    ec.BY_NAME["conv regular linear 192>256 k5"],
    ec.BY_NAME["wavenet layer cout2 384"],
    ec.ResblockCase("snake + conv step 32 k3 (valu model)", 32, 3, 1, capi.PRE_SNAKE),
]
BY_NAME = {c.name: c for c in STANDIN_CASES}
CONV, WAVENET, STEP = (c.name for c in STANDIN_CASES)
APPLIES = {
    CONV: ("truncate", "replicate_pad", "bias_block", "halo_neighbour"),
    WAVENET: ("truncate", "replicate_pad", "bias_block", "halo_neighbour", "gate_twice"),
    STEP: ("truncate", "replicate_pad", "drop_outer_tap", "bias_block", "halo_neighbour"),
}
STANDIN_MARGIN = 0.10  # (s of these three cases is below 0.033 in both formats: test_standin_cases_have_the_minimum_margin)

# mutant -> the check that catches it wherever it is tried (it fails others as well: the test prints them all).
#   truncate        (c): the gain moves by -4.5e-4 to -4.2e-3 (bf16) / -5.7e-5 to -5.3e-4 (fp16), 2 to 20 times 0.1 u; E_g / E_e 1.6 to 2.5
#   replicate_pad   (b): edge rows at 23 to 1900 times the budget
#   drop_outer_tap  (b): fp16, edge rows at 2.2 times the budget - see BELOW_THE_BUDGET for bf16
#   bias_block      (b): its channel block at 1.6 to 33 times the budget
#   halo_neighbour  (b): edge rows at 24 to 1250 times the budget
#   gate_twice      (b): every stratum at 1.10 to 1.14 times the budget ((a): 1.105 and 1.102, a hair over 1 + m)
MUTANT_FAILS = {"truncate": "c", "replicate_pad": "b", "drop_outer_tap": "b", "bias_block": "b", "halo_neighbour": "b", "gate_twice": "b"}
# The one (case, mutant, format) no check catches.  In bf16 the dropped tap changes the first and the last three frames of an
# utterance by about one bf16 rounding error of the output (the outer Kaiser tap is 1e-2 of the centre tap, bf16 rounds at 4e-3);
# they are 6 of the 30 edge rows of an utterance, and the edge rows' E_g / E_e is 1.019.  An rms statistic with m = 0.10 does not
# see a defect below 46 % of the rounding noise, in any stratum the issue defines; fp16 (noise 8 times smaller) does see it.
BELOW_THE_BUDGET = {(STEP, "drop_outer_tap", "bf16")}
# What the old TOL x scale assertion does with the mutants: it accepts every truncation, every doubly rounded gate, the dropped
# tap and, in bf16, the scaled bias; it rejects the two that put whole wrong samples into the halo, and the scaled bias in fp16 where
# the bias is large beside 3e-3.
OLD_CHECK_REJECTS = ({(n, m, f) for n in APPLIES for m in ("replicate_pad", "halo_neighbour") for f in FORMATS}
                     | {(CONV, "bias_block", "f16"), (STEP, "bias_block", "f16")})


@functools.lru_cache(maxsize=None)
def prepared(name, fmt):
    case = BY_NAME.get(name) or ec.BY_NAME[name]
    tile = case.tile_rows(fmt)
    lengths = case.lengths(fmt)
    cls = eb.row_classes(lengths, tile, case.reach) if case.classes == ec.ALL_CLASSES else np.full(sum(lengths), eb.INTERIOR, np.int8)
    inp = case.inputs(fmt, 0, lengths)
    r = case.ref(fmt, inp, lengths)
    e = ec.run_live(case, ec.model_ops(case), fmt, inp, lengths)
    return dict(case=case, tile=tile, lengths=lengths, cls=cls, inp=inp, r=r, e=e)


def standin_report(name, fmt, mutant, with_old=False):
    p = prepared(name, fmt)
    case = p["case"]
    g = ec.run_live(case, ec.model_ops(case, standin.StandIn, mutant=mutant), fmt, p["inp"], p["lengths"])
    rep = eb.evaluate(f"{name} / {mutant or 'stand-in'}", fmt, g, p["e"], p["r"], p["cls"], STANDIN_MARGIN, case.classes)
    return (rep, eb.old_check_passes(g, p["r"], fmt)) if with_old else rep


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", [c.name for c in STANDIN_CASES])
def test_standin_kernel_spends_the_budget_and_no_more(name, fmt):
    rep, old = standin_report(name, fmt, None, with_old=True)
    print(rep.line())
    assert rep.ok, rep.message()
    assert old
    assert abs(rep.ratio - 1.0) < 1e-2, rep.line()  # fp32 accumulation is invisible beside the 16-bit roundings


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name,mutant", [(n, m) for n in APPLIES for m in APPLIES[n]])
def test_mutant_exceeds_the_budget(name, mutant, fmt):
    rep, old = standin_report(name, fmt, mutant, with_old=True)
    print(rep.message())
    print(f"old check {'accepts' if old else 'rejects'} it")
    if (name, mutant, fmt) in BELOW_THE_BUDGET:
        assert rep.ok and old and 1.01 < rep.worst[1] < 1.0 + STANDIN_MARGIN, rep.message()
        return
    assert not rep.ok, f"{standin.MUTANTS[mutant]} passes every check: {rep.line()}"
    assert MUTANT_FAILS[mutant] in rep.failed, rep.message()
    assert old == ((name, mutant, fmt) not in OLD_CHECK_REJECTS)


def test_every_mutant_is_tried():
    assert {m for ms in APPLIES.values() for m in ms} == set(standin.MUTANTS) == set(MUTANT_FAILS)
    assert not any(m in ("truncate", "gate_twice", "drop_outer_tap") for _, m, _ in OLD_CHECK_REJECTS)


def test_snake_fir_matrices_restate_the_reference_padding():
    """The folded filter matrices (gen_up / gen_down of csrc/snake_mfma.h) against _snake_seq's explicit replicate padding, at lengths
    shorter than the filters' reach as well."""
    rng = np.random.default_rng(0)
    filt = ec.vs64.filter_asymmetric()
    al, be = rng.normal(size=8).astype(np.float32) * 0.3, rng.normal(size=8).astype(np.float32) * 0.3
    for T in (1, 2, 3, 5, 6, 7, 12, 40):
        X = rng.normal(size=(T, 8))
        U, D = (m.astype(np.float64) for m in abi_emulator._snake_fir_matrices(T, filt))
        u = U @ X
        got = D @ (u + (1.0 / (np.exp(be.astype(np.float64)) + 1e-9)) * np.sin(u * np.exp(al.astype(np.float64))) ** 2)
        want = abi_emulator._snake_seq(X, al, be, filt)
        assert np.abs(got - want).max() < 1e-6, T  # (the matrices sum the folded taps in fp32)


def test_row_classes():
    cls = eb.row_classes([1, 2, 20], 8, 1)
    assert cls[:3].tolist() == [eb.EDGE] * 3
    E, S, I = eb.EDGE, eb.SEAM, eb.INTERIOR
    #                             0  1  2  3  4  5  6  7 | 8  9 10 11 12 13 14 15 |16 17 18 19
    assert cls[3:].tolist() == [E, E, I, I, I, I, S, S, S, S, I, I, I, I, S, S, S, S, E, E]
    assert eb.row_classes([9], 8, 1).tolist() == [E, E, I, I, I, I, S, E, E]  # the last rows are edge rows, seam or not
    assert eb.row_classes([8], 8, 1).tolist() == [E, E, I, I, I, I, E, E]     # no boundary inside the utterance


def test_the_rounding_model_keeps_its_behaviour_by_default():
    assert abi_emulator.Emulator().mfma_snake is False


# -----------------------------------------------------------------------------------------------------------------------------------
# the conditions of the GPU cases
# -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,fmt", ec.case_ids(), ids=lambda v: str(v))
def test_conditions_hold_for_every_gpu_case(case, fmt):
    tile = case.tile_rows(fmt)
    lengths = case.lengths(fmt)
    if case.classes == ec.ALL_CLASSES:
        assert {1, 2, tile - 1, tile + 1} <= set(lengths)
        cls = eb.row_classes(lengths, tile, case.reach)
    else:
        cls = np.full(sum(lengths), eb.INTERIOR, np.int8)
    eb.check_conditions(case.name, cls, case.channels, case.classes)
    budgets = []
    for seed in range(eb.N_SEEDS):
        inp = case.inputs(fmt, seed, lengths)
        r = case.ref(fmt, inp, lengths)
        e = ec.run_live(case, ec.model_ops(case), fmt, inp, lengths)
        budgets.append(eb.rms(e - r))
        if seed == 0:
            rep = eb.evaluate(case.name, fmt, e, e, r, cls, 0.10, case.classes)  # asserts E_e > 0 in every stratum
            assert rep.ok and rep.rel_budget > ec.MIN_REL_BUDGET, rep.line()
    s = eb.seed_spread(budgets)
    print(f"{case.name} [{fmt}]: s = {s:.4f}, m = {eb.margin(s):.3f}, tile rows {tile}, lengths {lengths}")
    assert abs(s - ec.SEED_SPREAD[(case.name, fmt)]) <= 1e-3, f"s = {s:.4f}, the table says {ec.SEED_SPREAD[(case.name, fmt)]:.4f}"


def test_standin_cases_have_the_minimum_margin():
    for name in (CONV, WAVENET):
        for fmt in FORMATS:
            assert ec.case_margin(ec.BY_NAME[name], fmt) == STANDIN_MARGIN
