"""tests/wave_order.py and tests/wave_order_cases.py without a GPU: the emulated orders are sums, the generalised butterfly is the one
tests/test_gpu_fidelity.py used to define, the arg-best emulation is numpy's first occurrence, and every case of
tests/test_gpu_summation_orders.py still tells its order from the others (the builders assert it; here they all run)."""
import math

import numpy as np
import pytest

from tests import wave_order as wo
from tests import wave_order_cases as wc

LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
FORMS = [("butterfly 256", lambda v, dt: wo.butterfly_order_sum(v, dt, 256)), ("butterfly 64", lambda v, dt: wo.butterfly_order_sum(v, dt, 64)),
         ("tree 256", lambda v, dt: wo.tree_order_sum(v, dt, 256)), ("walk", wo.sequential_order_sum), ("reversed walk", wo.reversed_walk_sum)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_order_is_a_sum_within_the_textbook_bound(dtype):
    """Against math.fsum (the exactly rounded sum of the same values): any order of n - 1 rounded adds is within (n - 1) u sum |x|,
    u = 2^-24 or 2^-53.  The result has the dtype asked for, and signed, positive and two-column inputs are all covered."""
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    rng = np.random.default_rng(7)
    for n in LENGTHS:
        for positive in (False, True):
            v = wo.wide_values(rng, (n, 2), dtype, positive, orders_of_magnitude=12)
            assert v.dtype == dtype and (not positive or (v > 0).all())
            exact = [math.fsum(float(x) for x in v[:, c]) for c in range(2)]
            bound = [(n - 1) * u * math.fsum(abs(float(x)) for x in v[:, c]) for c in range(2)]
            for name, f in FORMS:
                got = f(v, dtype)
                assert got.dtype == dtype and got.shape == (2,), name
                for c in range(2):
                    assert abs(float(got[c]) - exact[c]) <= bound[c], (name, n, c)
            # one column as a vector is the same sum
            assert wo.bits(wo.butterfly_order_sum(v[:, 0], dtype)) == wo.bits(wo.butterfly_order_sum(v, dtype))[0]


def _butterfly_before(rows):
    """butterfly_order_sum as tests/test_gpu_fidelity.py defined it before it moved to tests/wave_order.py, kept to the letter."""
    s = np.zeros((256, rows.shape[1]))
    for f0 in range(0, len(rows), 256):
        chunk = rows[f0: f0 + 256]
        s[: len(chunk)] += chunk
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ o]
    return ((s[0] + s[64]) + s[128]) + s[192]


def test_the_generalised_butterfly_is_the_fidelity_tests_own():
    """On the very cases of test_spectral_reduce_adds_in_the_documented_order (same generator, same seed) the defaults of the
    generalised function give the bits of the function it replaces; and the orders differ there as that test demands."""
    frames = (1, 64, 65, 255, 256, 257, 1000)
    rng = np.random.default_rng(20261021)
    cases = [rng.normal(size=(F, 4)) * 2.0 ** rng.integers(-20, 21, size=(F, 4)) for F in frames]
    for F, c in zip(frames, cases):
        want = _butterfly_before(c)
        assert np.array_equal(wo.bits(wo.butterfly_order_sum(c)), wo.bits(want)), F
        assert np.array_equal(wo.bits(wo.order_sum("butterfly", c)), wo.bits(want)), F
        if F <= 64:  # up to one wavefront of partial sums the tree adds the same pairs
            assert np.array_equal(wo.bits(wo.tree_order_sum(c)), wo.bits(want)), F
            assert np.array_equal(wo.bits(wo.butterfly_order_sum(c, threads=64)), wo.bits(want)), F
        else:
            assert (wo.bits(wo.tree_order_sum(c)) != wo.bits(want)).any() and (wo.bits(wo.sequential_order_sum(c)) != wo.bits(want)).any(), F


def test_can_differ_names_the_lengths_at_which_nothing_can():
    assert not wo.can_differ("butterfly", "tree", 64) and wo.can_differ("butterfly", "tree", 65)
    assert not wo.can_differ("butterfly", "tree", 1000, threads=64)
    assert not wo.can_differ("butterfly", "sequential", 2) and wo.can_differ("butterfly", "sequential", 3)
    rng = np.random.default_rng(3)
    for n in (1, 2, 33, 64):  # where can_differ says no, the bits are indeed equal, whatever the values
        for _ in range(20):
            v = wo.wide_values(rng, (n,), np.float64)
            assert wo.bits(wo.butterfly_order_sum(v)) == wo.bits(wo.tree_order_sum(v))
            if n < 3:
                assert wo.bits(wo.butterfly_order_sum(v)) == wo.bits(wo.sequential_order_sum(v))


@pytest.mark.parametrize("width", [16, 64])
@pytest.mark.parametrize("maximum", [True, False])
def test_arg_best_is_the_first_occurrence(width, maximum):
    """Against np.argmax / np.argmin, which return the first occurrence, in every lane: random inputs with many ties, a tie between
    the last lane of one stride and lane 0 of the next, a tie between the two halves of a 16-lane group, all-equal input."""
    ref = np.argmax if maximum else np.argmin
    best = 9.0 if maximum else -9.0
    rng = np.random.default_rng(width + int(maximum))
    inputs = [rng.integers(0, 4, size=n).astype(np.float64) for n in (1, 2, width - 1, width, width + 1, 3 * width + 5) for _ in range(8)]
    for at in ((width - 1, width), (7, 8), (5, width + 5), (3, 9), (0, 2 * width)):
        v = rng.random(2 * width + 3)
        v[list(at)] = best
        inputs.append(v)
    inputs += [np.full(n, 1.5) for n in (1, width, 2 * width + 1)]
    for v in inputs:
        vals, idxs = wo.arg_best(v, width, maximum, first=11, every_lane=True)
        assert set(idxs) == {11 + int(ref(v))} and set(vals) == {v[ref(v)]}, v
    # one value a lane, the lane its index: the form of the pitch path (absent candidates are -inf and never win)
    for tie in ((3, 9), (8, 9), (0, 15)):
        v = [0.25] * 16
        v[tie[0]] = v[tie[1]] = 0.5
        v[12] = -np.inf
        _, idxs = wo.arg_best_lanes(v, range(16), 16, True)
        assert set(idxs) == {tie[0]}
    # the rule itself, and that an empty scan reports NONE
    assert wo.arg_before(1.0, 9, 0.0, 1, True) and wo.arg_before(1.0, 1, 1.0, 2, True) and not wo.arg_before(1.0, 2, 1.0, 1, True)
    assert wo.arg_before(0.0, 9, 1.0, 1, False) and not wo.arg_before(1.0, 1, 0.0, 2, False)
    assert wo.arg_best([], width, maximum) == (-np.inf if maximum else np.inf, wo.NONE)


def test_distinct_case_meets_its_own_condition_and_refuses_a_stale_seed():
    v, want, seed = wo.distinct_case(300, "butterfly", np.float64, columns=(2,))
    assert v.shape == (300, 2) and np.array_equal(wo.bits(want), wo.bits(wo.butterfly_order_sum(v)))
    for other in (wo.tree_order_sum(v), wo.sequential_order_sum(v)):
        assert (wo.bits(other) != wo.bits(want)).all()
    again = wo.distinct_case(300, "butterfly", np.float64, columns=(2,), seed=seed)
    assert np.array_equal(again[0], v) and again[2] == seed
    # a case that cannot tell the orders apart is refused when its seed is given: a post that throws the sum away
    with pytest.raises(AssertionError, match="no longer tells"):
        wo.distinct_case(300, "butterfly", np.float64, seed=seed, post=lambda s, x: s * 0.0)
    # and where nothing can differ nothing is demanded
    assert wo.distinct_case(1, "tree", np.float32)[2] == 0 and wo.distinct_case(2, "sequential", np.float64)[2] == 0


def test_every_case_of_the_gpu_tests_tells_its_order_apart():
    """Every builder of tests/wave_order_cases.py with its committed seed (each asserts its own distinctness), the table is complete,
    and a fresh search finds the same seeds: they are the first that qualify, not hand-picked."""
    found = wc.build_all()
    assert found == wc.SEEDS
    want = {("sumsq", n) for n in wc.SUMSQ_N} | {("stoi", n) for n in wc.STOI_SEGMENTS} | {("stoi_energy", n) for n in wc.STOI_ENERGY_FRAMES} | {("activity", n) for n in wc.ACTIVITY_SLOTS} | \
        {("prosody", n) for n in wc.PROSODY_ROWS} | {("units", n) for n in wc.UNIT_FRAMES}
    assert set(found) == want
    for (entry, n), seed in wc.SEEDS.items():
        if seed and entry not in ("sumsq", "stoi_energy"):
            kw = {"stoi": dict(order="butterfly", dtype=np.float64, columns=(2,), post=lambda s, v: s / np.float64(len(v))),
                  "activity": dict(order="sequential", dtype=np.float64, positive=True, also=(wc.WAVE_FORM, wc.REVERSED)),
                  "prosody": dict(order="butterfly", dtype=np.float32, post=lambda s, v: wc.prosody_model(v, s),
                                  make=lambda rng: wc.prosody_values(rng, n))}[entry]
            assert wo.distinct_case(n, **kw)[2] == seed, (entry, n)


def test_the_cases_are_what_the_entries_take():
    """Shapes, signs and the arithmetic the expected values stand on."""
    for n in wc.SUMSQ_N:
        x, partials, norm = wc.sumsq_case(n)
        assert x.dtype == np.float32 and x.shape == (n,) and norm.dtype == np.float32
        exact = math.fsum(float(v) * float(v) for v in x)
        assert abs(math.fsum(partials) - exact) <= n * 2.0 ** -53 * exact and abs(float(norm) - math.sqrt(exact)) <= 2.0 ** -23 * math.sqrt(exact)
        sq = wc.sumsq_squares(x)  # every square is exact in fp64: 24 x 24 bits
        assert all(float(a) == float(v) * float(v) for a, v in zip(sq.T.reshape(-1)[:min(n, 500)], x[:500]))
    x, partials, _ = wc.sumsq_case(200003)
    chunk = -(-200003 // 256)
    assert chunk > 3 * 256 and np.count_nonzero(partials) == -(-200003 // chunk)  # every thread adds more than one element
    for k in wc.ACTIVITY_SLOTS:
        assert (wc.activity_case(k)[0] > 0).all()
    for r in wc.PROSODY_ROWS:
        v, want = wc.prosody_case(r)
        assert v.dtype == want.dtype == np.float32 and v.shape == want.shape == (r, 2) and (want >= 0).all() and np.isfinite(want).all()
        assert r == 1 or ((v == 0).any(axis=0).all() and (v < 0).any())
    v, want = wc.prosody_exact_case()
    assert np.count_nonzero(v[:, 0]) == 7 and float(v[:, 0].sum()) == 31.75
    for maximum in (True, False):
        assert [c[2] for c in wc.plateau_cases(maximum)] == [63, 5, 0]
    assert [c[3] for c in wc.path_cases()] == [0, 3, 8, 3, 0, 8]
