"""The inputs and expected bits of tests/test_gpu_summation_orders.py, made on the host with the emulations of tests/wave_order.py.
Every builder asserts, before anything reaches the GPU, that its cases still tell the documented order from the others; the same
builders run in tests/test_wave_order_cpu.py, which needs no GPU.  ``python -m tests.wave_order_cases`` searches the seeds again
and prints the SEEDS table.

Lengths are the smallest at which an order can go wrong: 1, one wavefront, one past it, one short of a workgroup's sweep, the
sweep, one past it, and about 1000 (several sweeps)."""
import functools

import numpy as np

from tests import wave_order as wo

F32, F64 = np.float32, np.float64

# (entry, length) -> the seed distinct_case found; None: search (python -m tests.wave_order_cases prints the table)
SEEDS = {
    ('sumsq', 1): 0, ('sumsq', 256): 0, ('sumsq', 257): 0, ('sumsq', 65537): 0, ('sumsq', 200003): 0,
    ('stoi', 1): 0, ('stoi', 64): 0, ('stoi', 65): 5, ('stoi', 256): 3, ('stoi', 257): 0, ('stoi', 1000): 0,
    ('stoi_energy', 5): 0, ('stoi_energy', 2): 7,
    ('activity', 1): 0, ('activity', 63): 1, ('activity', 64): 0, ('activity', 65): 0, ('activity', 129): 0,
    ('prosody', 1): 0, ('prosody', 64): 3, ('prosody', 65): 5, ('prosody', 256): 2, ('prosody', 257): 2, ('prosody', 1000): 3,
    ('units', 1): 0, ('units', 63): 0, ('units', 64): 0, ('units', 65): 0, ('units', 200): 0,
}
SEARCH = False  # set by the seed search alone


def _case(entry, length, order, dtype, **kw):
    seed = None if SEARCH else SEEDS[(entry, length)]
    values, want, seed = wo.distinct_case(length, order, dtype, seed=seed, **kw)
    FOUND[(entry, length)] = seed
    return values, want


FOUND = {}


# ---- tts_sumsq: the 256-entry tree, per workgroup and over the partials ------------------------------------------------------------
SUMSQ_N = (1, 256, 257, 65537, 200003)
PARTIALS = 256


def sumsq_squares(x):
    """float32 [n] -> float64 [chunk, 256]: column b holds the squares (exact in fp64) workgroup b adds, chunk = ceil(n / 256) of
    them, zeros behind the end of x (adding +0 to a sum of squares changes no bit)."""
    chunk = -(-len(x) // PARTIALS)
    sq = np.zeros(chunk * PARTIALS, dtype=F64)
    sq[: len(x)] = x.astype(F64) * x.astype(F64)
    return np.ascontiguousarray(sq.reshape(PARTIALS, chunk).T)


@functools.lru_cache(maxsize=None)
def sumsq_case(n):
    """-> (x float32 [n], partials float64 [256] in the tree's order, norm float32).  The partials must differ from the butterfly's
    and the walk's in some workgroup wherever a workgroup's threads hold more than 64 sums (n > 64 * 256)."""
    chunk = -(-n // PARTIALS)
    make = lambda rng: wo.wide_values(rng, (n,), F32)
    x, _, seed = wo.distinct_case(chunk, "tree", F64, seed=None if SEARCH else SEEDS[("sumsq", n)], make=lambda rng: sumsq_squares(make(rng)),
                                  every_column=False)
    FOUND[("sumsq", n)] = seed
    x = make(np.random.default_rng([chunk, wo.ORDERS.index("tree"), seed]))
    partials = wo.tree_order_sum(sumsq_squares(x), F64)
    assert partials.shape == (PARTIALS,) and not partials[-(-n // chunk):].any()  # the workgroups past the end of x add nothing
    total = wo.tree_order_sum(partials, F64)
    return x, partials, F32(np.sqrt(total))


# ---- tts_stoi_reduce: butterfly + left fold in fp64, one-barrier form --------------------------------------------------------------
STOI_SEGMENTS = (1, 64, 65, 256, 257, 1000)
STOI_SEG = 30  # frames of a segment: a pair of M frames has S = M - 29 segments


@functools.lru_cache(maxsize=None)
def stoi_case(S):
    """-> (segment values float64 [S, 2], totals float64 [2] = the butterfly's sums / S)."""
    return _case("stoi", S, "butterfly", F64, columns=(2,), post=lambda s, v: s / F64(len(v)))


# ---- tts_stoi_frame_energy: the butterfly of one wavefront over four samples a lane ------------------------------------------------
STOI_ENERGY_FRAMES = (5, 2)  # frames of the two pairs: one more than a workgroup takes (four, a wavefront each), and fewer
STOI_N, STOI_HOP = 256, 128
SINGLE_SWEEP = (("tree over 256", lambda v, dt: wo.tree_order_sum(v, dt, 256)), ("butterfly over 256", lambda v, dt: wo.butterfly_order_sum(v, dt, 256)))


def stoi_window():
    """A float32 window with full mantissas, so that the fp32 product w x has a rounding of its own."""
    return (0.25 + 0.75 * np.random.default_rng(256).random(STOI_N)).astype(F32)


def stoi_energy_squares(x):
    """float32 [256 + 128 (F - 1)] -> float64 [256, F]: column f holds the squares (exact in fp64) of the fp32 products w[i] x[128 f
    + i] (one rounding each) that frame f adds."""
    F = (len(x) - STOI_N) // STOI_HOP + 1
    v = np.stack([(stoi_window() * x[STOI_HOP * f: STOI_HOP * f + STOI_N]).astype(F32) for f in range(F)], axis=1).astype(F64)
    return v * v


@functools.lru_cache(maxsize=None)
def stoi_energy_case(frames):
    """-> (x float32 [n], energy float64 [frames]): lane l adds the squares of samples l, l + 64, l + 128, l + 192 of the frame in
    turn, then the butterfly.  The frames overlap and a sum of 48-bit squares is often exact, so not every frame can be made to differ
    at once: the pair's energies differ in some frame from the walk's and from those of both single-sweep orders over the 256 samples."""
    # (exponents -6 .. 6: the squares still span some 30 binary orders of magnitude, and most of a frame's 256 terms reach its sum)
    make = lambda rng: wo.wide_values(rng, (STOI_N + STOI_HOP * (frames - 1),), F32, orders_of_magnitude=6)
    _, want, seed = wo.distinct_case(STOI_N, "butterfly", F64, threads=64, seed=None if SEARCH else SEEDS[("stoi_energy", frames)],
                                     make=lambda rng: stoi_energy_squares(make(rng)), also=SINGLE_SWEEP, every_column=False)
    FOUND[("stoi_energy", frames)] = seed
    return make(np.random.default_rng([STOI_N, wo.ORDERS.index("butterfly"), seed])), want


# ---- tts_activity_level: the in-order walk -----------------------------------------------------------------------------------------
ACTIVITY_SLOTS = (1, 63, 64, 65, 129)
WAVE_FORM = ("butterfly of one wavefront", lambda v, dt: wo.butterfly_order_sum(v, dt, threads=64))
REVERSED = ("reversed walk", wo.reversed_walk_sum)


@functools.lru_cache(maxsize=None)
def activity_case(slots):
    """-> (sq float64 [slots] > 0, their plain sequential sum); differs from both workgroup orders, from the one-wavefront butterfly
    and from the walk taken backwards."""
    return _case("activity", slots, "sequential", F64, positive=True, also=(WAVE_FORM, REVERSED))


# ---- tts_prosody_control: butterfly + left fold in fp32 ----------------------------------------------------------------------------
PROSODY_ROWS = (1, 64, 65, 256, 257, 1000)
PROSODY_SCALE = 2.0


def prosody_model(values, total=None):
    """The fp32 arithmetic of scale_variance (csrc/prosody.hip) around its sum for a scale of exactly 2 and no curves.  values
    float32 [n, ...], total = the sum of the columns' non-zero entries (default: butterfly order) -> the rows after the call: avg =
    total / count of the non-zero entries; every row, zeros included, becomes max(0, ((v - avg) * 2) + avg).  The doubling is exact,
    so the result is the same whether or not the multiply and the add are fused."""
    values = np.asarray(values, dtype=F32)
    total = wo.butterfly_order_sum(values, F32) if total is None else np.asarray(total, dtype=F32)
    count = (values != 0).sum(axis=0).astype(F32)  # an fp32 sum of ones: exact below 2^24 in any order
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = (total / count).astype(F32)
        out = ((values - avg).astype(F32) * F32(PROSODY_SCALE)).astype(F32) + avg
    return np.where(out < 0, F32(0), out).astype(F32)


def prosody_values(rng, rows):
    """float32 [rows, 2] (pitch, energy): signed, 40 binary orders of magnitude, about one row in eight exactly zero in either."""
    v = wo.wide_values(rng, (rows, 2), F32)
    if rows > 1:
        v[rng.random(size=(rows, 2)) < 0.125] = 0.0
        v[0][v[0] == 0] = 1.5  # (and the count never zero)
    return v


@functools.lru_cache(maxsize=None)
def prosody_case(rows):
    """-> (values float32 [rows, 2], the rows after the call float32 [rows, 2]).  What must differ between the orders is the stored
    rows, column by column: the mean shows in them only through its own bits."""
    return _case("prosody", rows, "butterfly", F32, post=lambda s, v: prosody_model(v, s), make=lambda rng: prosody_values(rng, rows))


def prosody_exact_case():
    """300 rows, seven of them non-zero powers of two in different wavefronts and sweeps: their sum is exact in any order, so the
    expected rows test the model of the arithmetic around the sum and nothing else."""
    v = np.zeros((300, 2), dtype=F32)
    at = (0, 5, 63, 64, 130, 255, 299)
    v[at, 0] = (1.0, 2.0, 4.0, 8.0, 0.5, 16.0, 0.25)
    v[at, 1] = (0.5, 0.25, 2.0, 1.0, 4.0, 0.125, 8.0)
    want = prosody_model(v)
    for other in (wo.sequential_order_sum(v, F32), wo.tree_order_sum(v, F32)):
        assert np.array_equal(wo.bits(prosody_model(v, other)), wo.bits(want))
    assert (want[list(at)] > 0).sum() >= 6 and not want[1].any()  # the mean is not representable: its rounding shows in the rows kept
    return v, want


# ---- tts_prominence_units: the wavefront layer -------------------------------------------------------------------------------------
UNIT_FRAMES = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def unit_case(frames):
    """-> (composite values float64 [frames], mean float64 = the one-wavefront butterfly's sum / frames)."""
    return _case("units", frames, "butterfly", F64, threads=64, post=lambda s, v: s / F64(len(v)))


def plateau_cases(maximum):
    """[(name, values float64 [n], index of the first best)] for a lane scan that starts at values[0]: equal best values in lanes 63
    and 0 of consecutive strides (the lower index sits in the higher lane), in one lane two strides apart, and everywhere."""
    rng = np.random.default_rng(64 + int(maximum))
    best, n = (4.0, 150) if maximum else (0.25, 150)
    base = lambda: 1.0 + rng.random(n)  # in [1, 2): strictly between the two plateau values
    cases = []
    for name, at in (("lanes 63 and 0", (63, 64)), ("lane 5 twice", (5, 69))):
        v = base()
        v[list(at)] = best
        cases.append((name, v, at[0]))
    cases.append(("all equal", np.full(n, 1.5), 0))
    for name, v, first in cases:
        assert wo.arg_best(v, 64, maximum) == (v[first], first), name
        assert first == (np.argmax(v) if maximum else np.argmin(v)), name
    return cases


# ---- tts_pitch_path: wave_arg_max<16> --------------------------------------------------------------------------------------------------
CANDIDATES, PATH_ROW, UNWRITTEN = 15, 16, 0xEE


def path_bytes(strength, n_cand):
    """The back-pointer rows of tts_pitch_path for an utterance whose candidates are all voiceless (frequency 0: every transition
    costs 0).  strength float64 [T, 15], n_cand [T] -> uint8 [T, 16]: byte c < 15 of row t >= 1 is the first best predecessor of
    candidate c (wave_arg_max<16> over delta[t - 1], -inf where a candidate is absent), byte 15 of every row the chosen candidate
    (the serial pick of the last frame keeps the first maximum, then the back-pointers are followed); row 0's other bytes are not
    written."""
    T = len(strength)
    rows = np.full((T, PATH_ROW), UNWRITTEN, dtype=np.uint8)
    local = lambda t: [strength[t][c] if c < n_cand[t] else -np.inf for c in range(PATH_ROW)]
    delta = local(0)
    for t in range(1, T):
        val, idx = wo.arg_best_lanes(delta, range(PATH_ROW), 16, True)
        assert len(set(idx)) == 1
        rows[t, :CANDIDATES] = idx[0]
        delta = [val[0] + l for l in local(t)]
    best = 0
    for k in range(1, n_cand[T - 1]):
        if delta[k] > delta[best]:
            best = k
    for t in range(T - 1, -1, -1):
        nxt = rows[t, best] if t > 0 else 0
        rows[t, 15] = best
        best = int(nxt)
    return rows


def path_cases():
    """[(name, strength float64 [T, 15], n_cand int32 [T], the byte every back-pointer and every chosen candidate must be)]: all
    strengths are small binary fractions, so every delta is exact and the ties are exact ties."""
    def utt(T, level, n_cand=None):
        s = np.tile(np.asarray(level, dtype=F64), (T, 1))
        return s, np.full(T, CANDIDATES, dtype=np.int32) if n_cand is None else np.asarray(n_cand, dtype=np.int32)

    flat = [0.5] * CANDIDATES
    two = lambda a, b: [0.125 if c == 0 else 0.5 if c in (a, b) else 0.25 for c in range(CANDIDATES)]
    cases = [("all tie", *utt(5, flat), 0), ("3 and 9 tie", *utt(6, two(3, 9)), 3), ("8 and 9 tie", *utt(4, two(8, 9)), 8),
             ("3 and 9 tie, fewer candidates", *utt(7, two(3, 9), [15, 10, 12, 15, 10, 11, 13]), 3), ("two frames", *utt(2, flat), 0),
             ("one frame", *utt(1, two(8, 9)), 8)]
    for name, s, nc, byte in cases:
        rows = path_bytes(s, nc)
        assert (rows[1:, :CANDIDATES] == byte).all() and (rows[:, 15] == byte).all() and (rows[0, :CANDIDATES] == UNWRITTEN).all(), name
    return cases


# ---- every case, for the CPU test and the seed search ------------------------------------------------------------------------------
def build_all():
    for n in SUMSQ_N:
        sumsq_case(n)
    for S in STOI_SEGMENTS:
        stoi_case(S)
    for f in STOI_ENERGY_FRAMES:
        stoi_energy_case(f)
    for k in ACTIVITY_SLOTS:
        activity_case(k)
    for r in PROSODY_ROWS:
        prosody_case(r)
    prosody_exact_case()
    for f in UNIT_FRAMES:
        unit_case(f)
    plateau_cases(True), plateau_cases(False), path_cases()
    return dict(FOUND)


if __name__ == "__main__":
    SEARCH = True
    found = build_all()
    print("SEEDS = {")
    for entry in ("sumsq", "stoi", "stoi_energy", "activity", "prosody", "units"):
        print("    " + ", ".join(f"({k[0]!r}, {k[1]}): {v}" for k, v in found.items() if k[0] == entry) + ",")
    print("}")
