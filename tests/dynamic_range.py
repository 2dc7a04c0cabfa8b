"""The error budget (tests/error_budget.py) away from unit scale: the cases of tests/error_budget_cases.py at *levels* (k, da) -
g = 2^k on every additive input, da added to every snake log alpha - and the sweep that finds where a rounding model stops being
finite (k_top) and where its budget is still the format's (k_floor).  Pure numpy / torch on the CPU; the GPU test
(tests/test_gpu_dynamic_range.py) and the CPU test (tests/test_dynamic_range_cpu.py) share everything here.

Checks at a level L, beside (a) and (b) of tests/error_budget.py, which do not change:
    (c) |gain(g) - gain(e)| <= 0.1 u_L,  u_L = u x max(1, rel_L / rel_0),  rel = E_e / rms(r) of the model, at L and at the unit level:
        where the quantisation is coarser the sampling noise of the gain grows with it; u_L is never below u.
    (d) max |g - r| <= K max |e_L - r_L|,  K = TOL max(1, max |r_0|) / max |e_0 - r_0| at the unit level of the same case and format,
        TOL 2e-2 (bf16) / 3e-3 (fp16): the looseness of the other kernel tests' floor, in units of the model's own worst element.
    (e) g is finite (the levels lie where the model is).
"""
import functools

import numpy as np

from tests import abi_emulator, error_budget as eb, error_budget_cases as ec

TOL = {"bf16": 2e-2, "f16": 3e-3}
UNIT_LEVEL = ec.UNIT_LEVEL
# the plain-format model of a case that names model options
PLAIN = dict(mfma_snake=False, snake_offset_sum=False, fast_gate=False, f32_norms=False)


@functools.lru_cache(maxsize=None)
def shape(case, fmt):
    """-> (lengths, row class of every live row) of a case's budget lengths."""
    lengths = case.lengths(fmt)
    if case.classes == ec.ALL_CLASSES:
        cls = eb.row_classes(lengths, case.tile_rows(fmt), case.reach)
    else:
        cls = np.full(sum(lengths), eb.INTERIOR, np.int8)
    return lengths, cls


def model_run(case, fmt, level, seed=0, lib_class=None, **model_kw):
    """-> (inputs, r, e) of a case at a level: the float64 restatement and the rounding model (or `lib_class`) on the stored inputs.
    An overflowing conversion makes e infinite or NaN; it is not an error here."""
    lengths, _ = shape(case, fmt)
    inp = case.inputs(fmt, seed, lengths, level)
    r = case.ref(fmt, inp, lengths)
    ops = ec.model_ops(case, lib_class or abi_emulator.Emulator, **dict(ec.level_model(case), **model_kw))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = ec.run_live(case, ops, fmt, inp, lengths)
    return inp, r, e


def rel_budget(e, r):
    """E_e / rms(r); inf where the model is not finite."""
    return eb.rms(e - r) / eb.rms(r) if np.isfinite(e).all() else float("inf")


def rel_at(case, fmt, level, **model_kw):
    _, r, e = model_run(case, fmt, level, **model_kw)
    return rel_budget(e, r)


@functools.lru_cache(maxsize=None)
def unit_figures(case, fmt):
    """-> (rel_0, K) of a case and format from the model and the reference at the unit level, seed 0."""
    _, r, e = model_run(case, fmt, UNIT_LEVEL)
    return rel_budget(e, r), TOL[fmt] * max(1.0, float(np.abs(r).max())) / float(np.abs(e - r).max())


def evaluate(case, fmt, level, g, e, r, m, name=None):
    """Checks (a) to (e) of one case at a level.  -> eb.Report (rep.failed: check letter -> messages)."""
    _, cls = shape(case, fmt)
    name = name or f"{case.name} {ec.level_id(level)}"
    if not np.isfinite(g).all():
        rep = eb.Report(name, fmt)
        rep.fail("e", f"{int((~np.isfinite(g)).sum())} non-finite elements where the model is finite")
        return rep
    rel0, K = unit_figures(case, fmt)
    rel = rel_budget(e, r)
    rep = eb.evaluate(name, fmt, g, e, r, cls, m, case.classes, unit=eb.UNIT[fmt] * max(1.0, rel / rel0))
    err, worst_e = float(np.abs(g - r).max()), float(np.abs(e - r).max())
    if err > K * worst_e:
        rep.fail("d", f"max |g - r| {err:.3e} > K {K:.2f} x max |e - r| {worst_e:.3e}")
    return rep


# -----------------------------------------------------------------------------------------------------------------------------------
# the sweep
# -----------------------------------------------------------------------------------------------------------------------------------
def sweep(case, fmt, model_kw):
    """rel over SWEEP_K at da = 0 (and over SWEEP_DA at k = 0 for a snake case), seed 0 -> ({k: rel}, {da: rel})."""
    over_k = {k: rel_at(case, fmt, (k, 0), **model_kw) for k in ec.SWEEP_K}
    over_da = {}
    if case.name in ec.SNAKE_LEVEL_CASES:
        over_da = {da: (over_k[0] if da == 0 else rel_at(case, fmt, (0, da), **model_kw)) for da in ec.SWEEP_DA}
    return over_k, over_da


def last_finite(rel):
    """The largest key such that the model is finite at it and at every smaller key."""
    top = None
    for k in sorted(rel):
        if not np.isfinite(rel[k]):
            break
        top = k
    return top


def table_row(case, fmt, model_kw):
    """One row of ec.RANGE_TABLE, recomputed."""
    over_k, over_da = sweep(case, fmt, model_kw)
    row = dict(k_top=last_finite(over_k), k_floor=min(k for k in over_k if over_k[k] <= 2.0 * over_k[0]),
               rel={k: over_k[k] for k in ec.TABLE_K if np.isfinite(over_k[k])})
    row["rel"][row["k_top"]] = over_k[row["k_top"]]
    if over_da:
        within = [da for da in sorted(over_da) if all(over_da[d] <= 2.0 * over_da[0] for d in over_da if d <= da)]
        row.update(da_top=last_finite(over_da), da_2x=max(within), rel_da=[over_da[da] for da in sorted(over_da) if np.isfinite(over_da[da])])
    return row


def level_spread(case, fmt, level):
    """s of one (case, format, level): (max - min) / mean of E_e over the 8 input seeds, model alone; the seed-0 (r, e) with it."""
    budgets, first = [], None
    for seed in range(eb.N_SEEDS):
        _, r, e = model_run(case, fmt, level, seed)
        assert np.isfinite(e).all(), f"{case.name} [{fmt}] {level}: the model is not finite at seed {seed}"
        budgets.append(eb.rms(e - r))
        first = first or (r, e)
    return eb.seed_spread(budgets), first


# -----------------------------------------------------------------------------------------------------------------------------------
# the hardware sine of the fp32 snake (csrc/snake.h) at sharp alphas
# -----------------------------------------------------------------------------------------------------------------------------------
SINE_ABS_ERR = 2e-6   # twice the "~1e-6" csrc/snake.h claims for v_sin_f32 after v_fract_f32
F32_TOL = 2e-5        # tests/test_gpu_kernels_vs_float64.py's fp32 tolerance, relative to the output scale
EPS32 = 2.0 ** -24


def snake_sine_bound(x, alpha, beta, filt, sine_err=SINE_ABS_ERR):
    """What the phase arithmetic of csrc/snake.h may add to |y - y_float64| on one utterance x [T, C] (float64 arrays holding fp32
    values; alpha, beta the log parameters), element by element [T, C].  With u = U x the 2x-rate samples (factor 2 included),
    theta = u e^alpha the phase in radians and p = theta / 2 pi = h er the phase in revolutions the kernel forms:
        |d p|      <= |p| 2^-24 (the fp32 product h er) + |p| 2^-24 (er's own rounding) + er |d h|,
                      |d h| <= 6 x 2^-24 (|U| / 2) |x|: the six fp32 fused multiply-adds that make h = u / 2
        |d theta|  =  2 pi |d p|  =  2 |theta| 2^-24 + e^alpha 6 x 2^-24 |U| |x|
        |d sin^2|  <= |d theta| + 2 sine_err           (|d/d theta sin^2| = |sin 2 theta| <= 1; (sin + err)^2 - sin^2 <= 2 err + err^2)
        |d s|      =  |d sin^2| / (e^beta + 1e-9)
        |d y|      <= |D| |d s|                         (the 12 decimator taps, replicate padding folded in)
    The direct fp32 error of u, of the fused multiply-add that forms s and of the decimator's sum is what F32_TOL covers already."""
    T = x.shape[0]
    U, D = (m.astype(np.float64) for m in abi_emulator._snake_fir_matrices(T, np.asarray(filt, dtype=np.float32)))
    ea, ib = np.exp(alpha), 1.0 / (np.exp(beta) + 1e-9)
    theta = np.abs(U @ x) * ea
    d_theta = 2.0 * theta * EPS32 + ea * 6.0 * EPS32 * (np.abs(U) @ np.abs(x))
    return np.abs(D) @ (ib * (d_theta + 2.0 * sine_err + sine_err ** 2))


def snake_fp32_exact_sine(x, alpha, beta, filt):
    """csrc/snake.h restated in fp32 numpy, operation by operation (products and sums rounded separately where the kernel fuses
    them), with an exact sine of the fp32 phase: x [T, C] -> y [T, C] float32."""
    f32 = np.float32
    x, f = np.asarray(x, dtype=f32), np.asarray(filt, dtype=f32)
    T, C = x.shape
    er = np.exp(np.asarray(alpha, dtype=f32)) * f32(0.3183098861837907)
    hb = f32(0.5) * (f32(1.0) / (np.exp(np.asarray(beta, dtype=f32)) + f32(1e-9)))
    q = np.arange(T)
    h = np.zeros((2 * T, C), f32)
    for parity, taps in ((0, [(d, 5 - 2 * d) for d in range(-3, 3)]), (1, [(d, 6 - 2 * d) for d in range(-2, 4)])):
        acc = np.zeros((T, C), f32)
        for d, k in taps:
            acc = acc + x[np.clip(q + d, 0, T - 1)] * f[k]
        h[parity::2] = acc
    p = h * er
    sn = np.sin(2.0 * np.pi * (p - np.floor(p)).astype(np.float64)).astype(f32)
    s = hb * (sn * sn) + h
    a = np.zeros((T, C), f32)
    for k in range(12):
        a = a + s[np.clip(2 * q + k - 5, 0, 2 * T - 1)] * f[k]
    assert a.dtype == f32
    return f32(2.0) * a
