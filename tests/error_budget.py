"""The error budget of a 16-bit kernel: how far its rounding model (tests/abi_emulator.py: float64 accumulation, rounded to 16 bits
exactly where the kernel says it rounds) lies from the float64 restatement of the same operation.  A correct kernel spends that
budget and no more.  Pure numpy; nothing here touches a GPU.

Over the live elements of one case (rows inside an utterance x output channels):
    g  the kernel's output        e  the rounding model's output on the same inputs        r  the float64 restatement, no rounding
    E(x) = rms(x - r), the budget is E(e);   gain(x) = <x - r, r> / <r, r>.
Every element carries a row class (edge / seam / interior, `row_classes`) and an output-channel block (32 consecutive channels,
the unit one wavefront owns in these kernels).

    (a) E(g) <= (1 + m) E(e)  over all live elements
    (b) the same in every row class, every channel block, and every row class x channel block cell of at least N_MIN elements
    (c) |gain(g) - gain(e)| <= 0.1 u,  u = 2^-9 (bf16) / 2^-12 (fp16)

m = max(0.10, 3 s), s = the relative spread (max - min) / mean of E(e) over 8 input seeds, measured from the rounding model alone
and written next to the case table (tests/error_budget_cases.py).  With m = 0.10 an independent defect is caught once its rms error
reaches sqrt(1.1^2 - 1) = 46 % of the rounding noise.  m is never raised because a kernel exceeded it.
"""
import numpy as np

N_MIN = 2048
BLOCK = 32
EDGE, SEAM, INTERIOR = 0, 1, 2
ROW_CLASSES = ("edge", "seam", "interior")
UNIT = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}
MAX_SMALL_CELLS = 0.25  # at most this share of the row class x channel block cells may hold fewer than N_MIN elements
N_SEEDS = 8


def margin(s):
    return max(0.10, 3.0 * s)


def row_classes(lengths, tile_rows, reach):
    """Row class of every live row, utterance after utterance (one int8 vector of sum(lengths) entries).
    edge: at most `reach` rows from the utterance's first or last row.  seam: at most `reach` rows from a tile boundary inside the
    utterance (the rows m * tile_rows - 1 and m * tile_rows, counted from the utterance's first row, are the boundary's two
    sides).  An edge row is an edge row even when it is near a seam.  tile_rows None: the kernel has no tiles along the rows."""
    out = []
    for n in lengths:
        t = np.arange(n)
        cls = np.full(n, INTERIOR, dtype=np.int8)
        if tile_rows:
            below = t % tile_rows                      # rows to the boundary at or below t (0: t is a tile's first row)
            above = tile_rows - 1 - below              # rows to the last row of t's tile
            near_lo = (below <= reach) & (t >= tile_rows)                         # a boundary below exists
            near_hi = (above <= reach) & (t - below + tile_rows < n)              # ... and one above
            cls[near_lo | near_hi] = SEAM
        cls[(t <= reach) | (n - 1 - t <= reach)] = EDGE
        out.append(cls)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int8)


def strata(row_class, channels, classes=(EDGE, SEAM, INTERIOR)):
    """[(name, kind, boolean mask [rows, channels])]: kind 'row', 'block' or 'cell'."""
    assert channels % BLOCK == 0, "a channel block is 32 consecutive output channels"
    rows = len(row_class)
    blocks = np.arange(channels) // BLOCK
    out = []
    for c in classes:
        out.append((ROW_CLASSES[c], "row", np.broadcast_to((row_class == c)[:, None], (rows, channels))))
    for b in range(channels // BLOCK):
        out.append((f"block {b}", "block", np.broadcast_to((blocks == b)[None, :], (rows, channels))))
    for c in classes:
        for b in range(channels // BLOCK):
            out.append((f"{ROW_CLASSES[c]} x block {b}", "cell", (row_class == c)[:, None] & (blocks == b)[None, :]))
    return out


def check_conditions(name, row_class, channels, classes=(EDGE, SEAM, INTERIOR)):
    """The conditions on a case's shape: every row class and every channel block holds N_MIN elements, and at most a quarter of the
    cells fall below it.  Returns the number of cells below N_MIN."""
    small = cells = 0
    for sname, kind, mask in strata(row_class, channels, classes):
        n = int(mask.sum())
        if kind == "cell":
            cells += 1
            small += n < N_MIN
        else:
            assert n >= N_MIN, f"{name}: stratum '{sname}' holds {n} elements, fewer than N_MIN = {N_MIN}"
    assert small <= MAX_SMALL_CELLS * cells, f"{name}: {small} of {cells} cells hold fewer than N_MIN = {N_MIN} elements"
    return small


def rms(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.mean(x * x))) if x.size else 0.0


def gain(x, r):
    x, r = np.asarray(x, dtype=np.float64).ravel(), np.asarray(r, dtype=np.float64).ravel()
    return float(np.dot(x - r, r) / np.dot(r, r))


def seed_spread(budgets):
    """s: (max - min) / mean of E(e) over the input seeds."""
    b = np.asarray(budgets, dtype=np.float64)
    assert len(b) == N_SEEDS and b.min() > 0.0
    return float((b.max() - b.min()) / b.mean())


class Report:
    """What `evaluate` found: the figures of one case and the checks it fails (a dict check letter -> messages)."""

    def __init__(self, name, fmt):
        self.name, self.fmt = name, fmt
        self.failed = {}
        self.rel_budget = self.ratio = self.gain_g = self.gain_e = float("nan")
        self.worst = ("", float("nan"))

    def fail(self, check, msg):
        self.failed.setdefault(check, []).append(msg)

    @property
    def ok(self):
        return not self.failed

    def line(self):
        return (f"{self.name} [{self.fmt}]: E_e/rms(r) {self.rel_budget:.3e}  E_g/E_e {self.ratio:.4f}  worst stratum '{self.worst[0]}' "
                f"{self.worst[1]:.4f}  gain g {self.gain_g:+.3e} e {self.gain_e:+.3e}")

    def message(self):
        return "\n".join([self.line()] + [f"  ({c}) {m}" for c in sorted(self.failed) for m in self.failed[c]])


def evaluate(name, fmt, g, e, r, row_class, m, classes=(EDGE, SEAM, INTERIOR), unit=None):
    """Checks (a) to (c) on one case; g, e, r: [live rows, channels].  Never raises for a failed check: see `check`.
    unit: the u of check (c) where it is not the format's own (tests/dynamic_range.py: never below it)."""
    g, e, r = (np.asarray(a, dtype=np.float64) for a in (g, e, r))
    assert g.shape == e.shape == r.shape and g.ndim == 2 and g.shape[0] == len(row_class)
    assert np.isfinite(g).all() and np.isfinite(e).all() and np.isfinite(r).all(), f"{name}: non-finite values"
    rep = Report(name, fmt)
    Ee, Eg = rms(e - r), rms(g - r)
    assert Ee > 0.0, f"{name}: the rounding model equals the float64 restatement: there is no budget to spend"
    rep.rel_budget, rep.ratio = Ee / rms(r), Eg / Ee
    if Eg > (1.0 + m) * Ee:
        rep.fail("a", f"all elements: E_g {Eg:.4e} > (1 + {m:.2f}) x E_e {Ee:.4e} (ratio {Eg / Ee:.4f})")
    worst = ("all", Eg / Ee)
    for sname, kind, mask in strata(row_class, g.shape[1], classes):
        n = int(mask.sum())
        if kind == "cell" and n < N_MIN:
            continue
        se, sg = rms((e - r)[mask]), rms((g - r)[mask])
        assert se > 0.0, f"{name}: stratum '{sname}' has no budget (E_e = 0)"
        if sg / se > worst[1]:
            worst = (sname, sg / se)
        if sg > (1.0 + m) * se:
            rep.fail("b", f"stratum '{sname}' ({n} elements): E_g {sg:.4e} > (1 + {m:.2f}) x E_e {se:.4e} (ratio {sg / se:.4f})")
    rep.worst = worst
    rep.gain_g, rep.gain_e = gain(g, r), gain(e, r)
    u = UNIT[fmt] if unit is None else unit
    assert u >= UNIT[fmt]
    if abs(rep.gain_g - rep.gain_e) > 0.1 * u:
        rep.fail("c", f"gain(g) {rep.gain_g:+.4e} - gain(e) {rep.gain_e:+.4e} = {rep.gain_g - rep.gain_e:+.3e}, beyond 0.1 u = {0.1 * u:.3e}")
    return rep


def check(name, fmt, g, e, r, row_class, m, classes=(EDGE, SEAM, INTERIOR)):
    """`evaluate`, raising with the case, the strata and the numbers when a check fails.  Returns the report."""
    rep = evaluate(name, fmt, g, e, r, row_class, m, classes)
    assert rep.ok, "over the error budget: " + rep.message()
    return rep


def old_check_passes(g, r, fmt):
    """The assertion every 16-bit kernel test ends in: max |g - r| <= TOL max(1, max |r|), TOL 2e-2 (bf16) / 3e-3 (fp16)."""
    tol = {"bf16": 2e-2, "f16": 3e-3}[fmt]
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.abs(g - r).max()) <= tol * max(1.0, float(np.abs(r).max()))
