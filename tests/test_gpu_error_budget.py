"""The 16-bit kernels held to the error budget of their rounding model (tests/error_budget.py; DESIGN.md, "Error budgets of the
16-bit kernels"): g = the kernel on the MI355X, e = tests/abi_emulator.py on the same inputs (with the options the case names),
r = the plain float64 restatement.  E_g <= (1 + m) E_e over all live elements, in every row class (edge / seam / interior), every
32-channel block and every cell of N_MIN elements; |gain(g) - gain(e)| <= 0.1 u; and the max-abs check the other kernel tests end
in, as a coarse floor.  The cases, their lengths (built from the library's own tile rows), s and m: tests/error_budget_cases.py;
their conditions are checked without a GPU in tests/test_error_budget_cpu.py."""
import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import engine
from tests import abi_emulator, error_budget as eb, error_budget_cases as ec

pytestmark = pytest.mark.gpu
TOL = {"bf16": 2e-2, "f16": 3e-3}  # relative to the output scale: tests/test_gpu_kernels_vs_float64.py's 16-bit tolerances


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ops = engine.Ops("cuda:0")
    assert not isinstance(ops.lib, abi_emulator.Emulator)
    return ops


@pytest.mark.parametrize("case,fmt", ec.case_ids(), ids=lambda v: str(v))
def test_kernel_spends_its_error_budget_and_no_more(gpu, case, fmt):
    tile = case.tile_rows(fmt)
    lengths = case.lengths(fmt)
    cls = eb.row_classes(lengths, tile, case.reach) if case.classes == ec.ALL_CLASSES else np.full(sum(lengths), eb.INTERIOR, np.int8)
    eb.check_conditions(case.name, cls, case.channels, case.classes)
    inp = case.inputs(fmt, 0, lengths)
    r = case.ref(fmt, inp, lengths)
    e = ec.run_live(case, ec.model_ops(case), fmt, inp, lengths)
    g = ec.run_live(case, gpu, fmt, inp, lengths)
    rep = eb.evaluate(case.name, fmt, g, e, r, cls, ec.case_margin(case, fmt), case.classes)
    print(rep.line())
    assert rep.ok, "over the error budget: " + rep.message()
    # (d) the coarse floor, as it stands in the other kernel tests
    scale = max(1.0, float(np.abs(r).max()))
    err = float(np.abs(g - r).max())
    assert err <= TOL[fmt] * scale, f"max abs err {err:.3e} vs tol {TOL[fmt] * scale:.3e}"
