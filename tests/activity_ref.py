"""Float64 restatement of the speech-activity meter (csrc/activity.hip, include/toucan_activity.h): ITU-T P.56 method B with
nothing parallel in it - the two-stage envelope sample by sample, the hangover by the definition and by the literal counter, the
segment form of the count that the kernels use, the level with its interpolation, the runs - the bound the kernel's carried
states must meet, and the seeded signals the activity tests share.  Nothing here imports the product's activity.py.

The bound on a carried state (derived, not measured).  u = 2^-53; X = max |x| of the utterance; g the envelope coefficient,
h = 1 - g.  Both p and q are convex combinations of earlier values and |x|, so neither exceeds X.  A step of p rounds h |x| and the
fma (the kernel), or h |x|, g p and their sum (this file): at most 3 u X; the error of p decays by g per step, so it stays below
3 u X / (1 - g).  A step of q adds its own 3 u X and h times the error of p, again at most 3 u X: below 6 u X / (1 - g).  The
segment-parallel form adds, per segment, the roundings of s_{k+1} = T s_k + end_k (four, each at most u X) and the error of T
itself (S steps of relative error u each on entries below 0.13: at most 0.3 S u X, which is 0.1 u X / (1 - g) since
S = 1 / (0.3 (1 - g)) to first order); T contracts (its norm is below 0.2), so these do not accumulate past 1.25 times one
segment's share.  Kernel and restatement each stay within their own error of the exact envelope:

    |p - p_ref|, |q - q_ref| <= 16 u X / (1 - g)

covers both with room (6 + 6 + 0.13 + 5 (1 - g) <= 12.2).  The recurrence contracts, so the bound does not grow with the length.
What it rules out is a wrong coefficient, transition or carry, which moves a state by parts in 10^2.  The sharp check is the
counts: with every q_t at least 1e-9 (relative) away from every threshold, they must be exact.
"""
import functools
import math

import numpy as np

from tests.loudness_ref import RATES, noise, tone  # the rates and the seeded signals of the loudness tests

U = 2.0 ** -53
MARGIN_DB, THRESHOLDS = 15.9, 15
LADDER = tuple(2.0 ** (j - 15) for j in range(THRESHOLDS))
COLUMNS = ("active_db", "long_term_db", "activity", "threshold_db", "speech_begin", "speech_end", "gain", "active_db_after")
MAX_RUNS = 2  # what the GPU test asks for: the three-burst case has more


def coefficient(sr):
    return math.exp(-1.0 / (0.03 * sr))


def envelope(x, sr, state=(0.0, 0.0)):
    """(p_t, q_t) of every sample, float64 arrays, sample by sample from ``state``."""
    g = coefficient(sr)
    h = 1.0 - g
    p, q = state
    ps, qs = [0.0] * len(x), [0.0] * len(x)
    for t, v in enumerate(np.abs(np.asarray(x, dtype=np.float64)).tolist()):
        p = g * p + h * v
        q = g * q + h * p
        ps[t], qs[t] = p, q
    return np.array(ps, dtype=np.float64), np.array(qs, dtype=np.float64)


def active_count(above, I):
    """The definition: sample t is active if some t' <= t has above[t'] and t - t' <= I."""
    t = np.arange(len(above), dtype=np.int64)
    last = np.maximum.accumulate(np.where(above, t, -(I + 1)))
    return int((t - last <= I).sum())


def active_count_literal(above, I):
    """The Recommendation's hangover counter, started as exhausted, sample by sample."""
    hang, a = I + 1, 0
    for hit in above.tolist():
        hang = 0 if hit else min(hang + 1, I + 1)
        if hang <= I:
            a += 1
    return a


def segment_positions(above, S):
    """[(S_k, first, last)] per segment slot of S samples (the last possibly partial); first = last = -1 where none is set."""
    out = []
    for k in range(-(-len(above) // S)):
        idx = np.flatnonzero(above[k * S:(k + 1) * S])
        out.append((min(S, len(above) - k * S), int(idx[0]) if idx.size else -1, int(idx[-1]) if idx.size else -1))
    return out


def active_count_segments(above, S, I):
    """The segment form the kernels use: the count from the first and last sample of every segment and an integer carry."""
    a = r = 0
    for Sk, f, l in segment_positions(above, S):
        if f < 0:
            a += min(r, Sk)
            r = max(0, r - Sk)
        else:
            tail = Sk - 1 - l
            a += min(r, f) + (l - f + 1) + min(I, tail)
            r = max(0, I - tail)
    return a


def runs_of(above, I):
    """[(first, last + 1)] of the samples set in ``above``, chained wherever two neighbours are at most I apart."""
    idx = np.flatnonzero(above)
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) > I)
    firsts = np.concatenate([[idx[0]], idx[cut + 1]])
    lasts = np.concatenate([idx[cut], [idx[-1]]])
    return [(int(b), int(e) + 1) for b, e in zip(firsts, lasts)]


def level(sq, n, a):
    """(active_db, long_term_db, activity, threshold_db) from the sum of squares, the sample count and a_0 .. a_14."""
    if n == 0 or sq == 0 or a[0] == 0:
        return -math.inf, -math.inf, 0.0, -math.inf
    long_term = 10.0 * math.log10(sq / n)
    A = C = D = None
    for j in range(THRESHOLDS):
        if a[j] == 0:
            break
        A1, C1 = 10.0 * math.log10(sq / a[j]), 20.0 * math.log10(LADDER[j])
        D1 = A1 - C1
        if D1 <= MARGIN_DB:
            if j > 0:
                w = (D - MARGIN_DB) / (D - D1)
                A1, C1 = A + w * (A1 - A), C + w * (C1 - C)
            return A1, long_term, 10.0 ** ((long_term - A1) / 10.0), C1
        A, C, D = A1, C1, D1
    return A, long_term, 10.0 ** ((long_term - A) / 10.0), C  # no threshold qualifies: the last one with active samples


def gain(active_db, peak, target, ceiling):
    """The gain of the definition before its rounding to float32, and whether the ceiling is what limits it."""
    if not math.isfinite(active_db) or peak == 0:
        return 1.0, False
    g, lim = 10.0 ** ((target - active_db) / 20.0), 10.0 ** (ceiling / 20.0) / peak
    return (lim, True) if lim < g else (g, False)


def relative_margin(q, c):
    """The least relative distance of any q_t from the threshold c."""
    return float(np.abs(q / c - 1.0).min(initial=math.inf))


def measure(x, sr):
    """Everything the meter reports about one utterance, and the two margins of the counts' exactness."""
    x = np.asarray(x, dtype=np.float32)
    S, n = sr // 10, len(x)
    I = 2 * S
    p, q = envelope(x, sr)
    a = [active_count(q >= c, I) for c in LADDER]
    sq = math.fsum((x.astype(np.float64) ** 2).tolist())
    peak = float(np.abs(x).max(initial=0.0))
    active_db, long_term_db, activity, threshold_db = level(sq, n, a)
    runs, c_star = [], math.inf
    if math.isfinite(threshold_db):
        c_star = 10.0 ** (threshold_db / 20.0)
        runs = runs_of(q >= c_star, I)
    starts = np.zeros((-(-n // S), 2))
    for k in range(1, len(starts)):
        starts[k] = (p[k * S - 1], q[k * S - 1])
    return {"n": n, "x": x, "q": q, "a": a, "sq": sq, "peak": peak, "active_db": active_db, "long_term_db": long_term_db, "activity": activity,
            "threshold_db": threshold_db, "c_star": c_star, "runs": runs, "speech_begin": runs[0][0] if runs else 0,
            "speech_end": runs[-1][1] if runs else 0, "starts": starts, "state_bound": state_bound(x, sr),
            "ladder_margin": min(relative_margin(q, c) for c in LADDER),
            "final_margin": relative_margin(q, c_star) if math.isfinite(c_star) else math.inf}


def state_bound(x, sr):
    """The bound of the module docstring on |p - p_ref| and |q - q_ref| at every segment start of the utterance x."""
    return 16.0 * U * float(np.abs(x).max(initial=0.0)) / (1.0 - coefficient(sr))


def bursts(sr, plan, amplitude=0.5):
    """plan: [(segments, on)] in units of S (fractions allowed) -> a 997 Hz tone where on, zeros elsewhere, float32."""
    S = sr // 10
    parts, at = [], 0
    for length, on in plan:
        m = int(round(length * S))
        parts.append(tone(m, sr, 20.0 * math.log10(amplitude), start=at) if on else np.zeros(m, dtype=np.float32))
        at += m
    return np.concatenate(parts)


def signals(sr, tile):
    """[(name, float32 wave)], the smallest shapes that reach every edge: nothing, one sample, the lengths around one segment,
    silence, noise too quiet for the lowest threshold, one full-scale click (no threshold qualifies), a full-scale sine, two bursts
    a short gap apart (one run), two a long gap apart (two runs, one pause), three (more runs than MAX_RUNS), speech in the
    trailing partial segment only; at 8 kHz also exactly ``tile`` segments, a burst that ends a few samples before the last
    segment of the first workgroup (the hangover is carried into the second), and 2 tile + 3 segments of noise."""
    S = sr // 10
    out = [("empty", np.zeros(0, dtype=np.float32)), ("one", np.full(1, 0.5, dtype=np.float32))]
    out += [(f"noise_{name}", noise(n, seed=20 + i)) for i, (name, n) in enumerate((("S-1", S - 1), ("S", S), ("S+1", S + 1)))]
    out.append(("zeros", np.zeros(3 * S, dtype=np.float32)))
    out.append(("too_quiet", (noise(3 * S + 7, seed=24) * np.float32(1e-6 / 0.3)).astype(np.float32)))
    click = np.zeros(6 * S, dtype=np.float32)
    click[S // 2 + 3] = 1.0
    out.append(("click", click))
    out.append(("sine", tone(7 * S + 123, sr, 0.0)))
    out.append(("bursts_close", bursts(sr, [(1, False), (3, True), (1.5, False), (3, True), (3, False)])))
    out.append(("bursts_far", bursts(sr, [(1, False), (3, True), (8, False), (3, True), (2, False)])))
    out.append(("three_runs", bursts(sr, [(0.5, False), (2, True), (5, False), (2, True), (5, False), (2, True), (1.3, False)])))
    out.append(("partial_only", bursts(sr, [(3, False), (0.5, True)])))
    if sr == 8000:
        out.append(("one_workgroup", noise(tile * S, seed=31)))
        burst_end = (tile - 1) * S - 5
        across = np.zeros((tile + 2) * S + 5, dtype=np.float32)
        across[(tile - 5) * S:burst_end] = tone(burst_end - (tile - 5) * S, sr, -6.0)
        out.append(("across_workgroups", across))
        out.append(("past_two_workgroups", noise((2 * tile + 3) * S, seed=32)))
    return out


@functools.lru_cache(maxsize=None)
def cases(sr, tile=64):
    """The shared, read-only reference of one rate: per signal what ``measure`` returns, with its name."""
    out = []
    for name, x in signals(sr, tile):
        item = dict(measure(x, sr), name=name)
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(item)
    return tuple(out)
