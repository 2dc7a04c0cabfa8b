"""numpy emulations of the summation orders and of the tie rule of csrc/wave_ops.h, shared by the CPU and GPU
tests.  Every add is ONE rounded add in the given dtype (float32 or float64): arrays of that dtype added element-wise, never a
pairwise ``np.sum``.

A sum takes ``rows`` [n, ...]: n values per column, the trailing axes being independent columns that are added alike.  The forms:

  butterfly_order_sum(rows, dtype, threads=256)  thread t adds rows t, t + threads, ... in turn; the 64 lanes of a wavefront are
                                                 folded by the xor butterfly 32 .. 1 (wave_sum); the wavefronts left to right,
                                                 ((r0 + r1) + r2) + r3 (block_sum).  threads=64: one wavefront, the butterfly alone.
  tree_order_sum(rows, dtype, threads=256)       the same per-thread sums halved in LDS: (t, t + threads / 2), ... (0, 1)
                                                 (block_tree_fold)
  sequential_order_sum(rows, dtype)              the plain walk in index order (wave_each_in_order)

``arg_best`` is the first best of (value, index): each lane's ascending scan with a strict comparison, then the xor butterfly with
arg_before.  ``distinct_case`` makes the inputs of the bit-exact GPU tests: values for which the wanted order differs in bits from
the others, since a case that does not tell the orders apart proves nothing."""
import numpy as np

ORDERS = ("butterfly", "tree", "sequential")
WAVE = 64
NONE = 2 ** 31 - 1  # the index of a lane that holds no value (PM_NONE of prominence.hip)


def thread_sums(rows, dtype, threads):
    """[n, ...] -> [threads, ...]: thread t's sum of rows t, t + threads, ... in turn, from 0."""
    rows = np.asarray(rows, dtype=dtype)
    s = np.zeros((threads,) + rows.shape[1:], dtype=dtype)
    for f0 in range(0, len(rows), threads):
        chunk = rows[f0: f0 + threads]
        s[: len(chunk)] = s[: len(chunk)] + chunk
    return s


def butterfly_order_sum(rows, dtype=np.float64, threads=256):
    assert threads % WAVE == 0 and dtype in (np.float32, np.float64)
    s = thread_sums(rows, dtype, threads)
    lanes = np.arange(threads)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ o]
    r = s[0]
    for k in range(1, threads // WAVE):
        r = r + s[WAVE * k]
    return r


def tree_order_sum(rows, dtype=np.float64, threads=256):
    assert threads & (threads - 1) == 0 and dtype in (np.float32, np.float64)
    s = thread_sums(rows, dtype, threads)
    o = threads // 2
    while o:
        s[:o] = s[:o] + s[o: 2 * o]
        o //= 2
    return s[0]


def sequential_order_sum(rows, dtype=np.float64):
    assert dtype in (np.float32, np.float64)
    rows = np.asarray(rows, dtype=dtype)
    s = np.zeros(rows.shape[1:], dtype=dtype)
    for r in rows:
        s = s + r
    return s


def reversed_walk_sum(rows, dtype=np.float64):
    """The walk with every group of 64 taken backwards: what a reversed wave_each_in_order would add."""
    rows = np.asarray(rows, dtype=dtype)
    order = np.concatenate([np.arange(k0, min(k0 + WAVE, len(rows)))[::-1] for k0 in range(0, len(rows), WAVE)]) if len(rows) else []
    return sequential_order_sum(rows[order], dtype)


def order_sum(order, rows, dtype=np.float64, threads=256):
    if order == "butterfly":
        return butterfly_order_sum(rows, dtype, threads)
    if order == "tree":
        return tree_order_sum(rows, dtype, threads)
    assert order == "sequential", order
    return sequential_order_sum(rows, dtype)


def bits(a):
    """The bit patterns of a float32 / float64 array (or scalar) as unsigned integers."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- first best of (value, index) ------------------------------------------------------------------------------------------------
def arg_before(ov, oi, v, i, maximum):
    """wave_ops.h arg_before: (ov, oi) goes before (v, i) if ov is better, or equal and oi < i."""
    return bool((ov > v) if maximum else (ov < v)) or bool(ov == v and oi < i)


def arg_best_lanes(values, indices, width, maximum=True):
    """The xor butterfly width / 2 .. 1 of wave_arg_best over one group of ``width`` lanes -> (values, indices) of every lane."""
    v, i = list(values), list(indices)
    assert len(v) == len(i) == width and width in (16, 64)
    o = width // 2
    while o:
        nv, ni = list(v), list(i)
        for l in range(width):
            if arg_before(v[l ^ o], i[l ^ o], v[l], i[l], maximum):
                nv[l], ni[l] = v[l ^ o], i[l ^ o]
        v, i, o = nv, ni, o // 2
    return v, i


def arg_best(values, width=64, maximum=True, first=0, every_lane=False):
    """(best value, its index) as the kernels find it: lane l scans first + l, first + l + width, ... in ascending order and takes
    a value only if it is strictly better, so the first of equal values stays; a lane that met nothing holds (-+inf, NONE); then
    the butterfly.  -> lane 0's pair, or with ``every_lane`` the pairs of all lanes (they agree)."""
    worst = -np.inf if maximum else np.inf
    v, i = [worst] * width, [NONE] * width
    for k, x in enumerate(values):
        l = k % width
        if (x > v[l]) if maximum else (x < v[l]):
            v[l], i[l] = x, first + k
    v, i = arg_best_lanes(v, i, width, maximum)
    return (v, i) if every_lane else (v[0], i[0])


# ---- cases that tell the orders apart ----------------------------------------------------------------------------------------------
def can_differ(a, b, length, threads=256):
    """Whether orders a and b can give different bits at all on ``length`` values a column: two values have one sum, and the tree
    and the butterfly add the same pairs while at most 64 threads hold a non-zero partial sum."""
    if a == b or length < 3:
        return False
    if {a, b} == {"butterfly", "tree"}:
        return min(length, threads) > WAVE
    return True


def wide_values(rng, shape, dtype, positive=False, orders_of_magnitude=20):
    """Values spread over 2 * orders_of_magnitude binary orders of magnitude, exact in ``dtype``: normal deviates, or for inputs that
    must be positive a random mantissa in [1, 2), times a random power of two."""
    m = 1.0 + rng.random(size=shape) if positive else rng.normal(size=shape)
    return (m.astype(dtype) * (2.0 ** rng.integers(-orders_of_magnitude, orders_of_magnitude + 1, size=shape)).astype(dtype)).astype(dtype)


def column_differs(a, b):
    """Per column (last axis; a scalar is one column): whether any of its entries differs in bits."""
    d = np.atleast_1d(bits(np.asarray(a)) != bits(np.asarray(b)))
    return d.reshape(-1, d.shape[-1]).any(axis=0) if d.ndim > 1 else d


def told_apart(values, order, dtype, threads=256, post=None, also=(), every_column=True):
    """-> (the result in ``order``, [names of the orders it fails to differ from]).  The result is ``post(sum, values)`` (default:
    the sum): what the kernel stores, so that a division or a cast behind the sum cannot hide the difference.  Compared are the two
    other orders where they can differ at this length, and the ``also`` callables (name, f(values, dtype)); with ``every_column``
    each column (last axis) must differ, else any entry."""
    post = post or (lambda s, v: s)
    want = post(order_sum(order, values, dtype, threads), values)
    others = [(o, order_sum(o, values, dtype, threads)) for o in ORDERS if can_differ(order, o, len(values), threads)]
    others += [(name, f(values, dtype)) for name, f in also if len(values) >= 3]
    same = []
    for name, s in others:
        d = column_differs(want, post(s, values))
        if not (d.all() if every_column else d.any()):
            same.append(name)
    return want, same


def distinct_case(length, order, dtype, columns=(), threads=256, positive=False, seed=None, post=None, also=(), every_column=True,
                  make=None, tries=2000):
    """-> (values [length, *columns] in dtype, the expected result, seed).  ``seed`` None: search seeds 0, 1, ... until the result in
    ``order`` differs in bits from each other order that can differ (told_apart); a given seed is used as it is and must still meet
    the condition (AssertionError otherwise): the GPU tests pass the committed seeds.  ``make(rng)`` replaces the default values
    (wide_values)."""
    make = make or (lambda rng: wide_values(rng, (length,) + tuple(columns), dtype, positive))
    for s in ([seed] if seed is not None else range(tries)):
        values = make(np.random.default_rng([length, ORDERS.index(order), s]))
        want, same = told_apart(values, order, dtype, threads, post, also, every_column)
        if not same:
            return values, want, s
    assert seed is None, f"seed {seed} no longer tells {order} from {same} at length {length}"
    raise AssertionError(f"no seed below {tries} tells {order} from {same} at length {length}")
