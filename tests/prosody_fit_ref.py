"""numpy restatement of the time-budget solver (include/toucan_prosody_fit.h) in float32 and int64: the frame
count F, the solve on the bit patterns, the repair and the report.  It shares no code with the package.  ``fixture()`` is the seeded
batch both test files solve."""
import numpy as np

F_SILENCE, F_WORD_BOUNDARY, F_PHONEME, F_VOICED = 16, 21, 15, 61
UTT_DURATION, UTT_PAUSE, SPAN = 0, 1, 2
EMPTY, EXACT, REPAIRED, NEAREST, CLAMPED_LOW, CLAMPED_HIGH = range(6)
f32 = np.float32


def bits(x):
    return int(np.array(x, dtype=np.float32).view(np.uint32))


def from_bits(b):
    return np.array(b, dtype=np.uint32).view(np.float32)[()]


def pred(x):
    return from_bits(bits(x) - 1)


def succ(x):
    return from_bits(bits(x) + 1)


def rows(text, dur, c, kind, x, s_duration, s_pause):
    """d'' of every row of a segment with its knob at x: text [n, 62], dur [n] (as predicted), c [n] float32 (curve column 0)."""
    x, s_duration, s_pause = f32(x), f32(s_duration), f32(s_pause)
    d = np.asarray(dur).astype(np.int64).copy()
    d[text[:, F_WORD_BOUNDARY] == 1] = 0
    c = np.asarray(c, dtype=np.float32)
    if kind == UTT_DURATION:
        pause, ed = s_pause, x * c
    elif kind == UTT_PAUSE:
        pause, ed = x, s_duration * c
    else:
        pause, ed = s_pause, s_duration * (c * x)
    assert ed.dtype == np.float32
    sil = text[:, F_SILENCE] == 1
    if pause != 1:
        d[sil] = np.rint(d[sil].astype(np.float32) * pause).astype(np.int64)
    m = ed != 1
    d[m] = np.rint(d[m].astype(np.float32) * ed[m]).astype(np.int64)
    return d


def frames(*a):
    return int(rows(*a).sum())


def solve_one(text, dur, c, kind, target, lo, hi, exact, s_duration=1.0, s_pause=1.0):
    """One segment -> dict(status, value, extra [n] int64, report [8] float32, x0, x1 (None unless the bisection ran))."""
    n = len(dur)
    T, lo, hi = int(target), f32(lo), f32(hi)
    F = lambda x: frames(text, dur, c, kind, x, s_duration, s_pause)
    given = f32(s_duration if kind == UTT_DURATION else s_pause if kind == UTT_PAUSE else 1.0)
    f_base, f_lo, f_hi = F(given), F(lo), F(hi)
    extra = np.zeros(n, dtype=np.int64)
    value, f_value, iterations, x0, x1 = given, f_base, 0, None, None
    if f_lo == f_hi:
        status = EMPTY
    elif f_lo > T:
        status, value, f_value = CLAMPED_LOW, lo, f_lo
    elif f_hi < T:
        status, value, f_value = CLAMPED_HIGH, hi, f_hi
    elif f_lo == T:
        status, value, f_value = EXACT, lo, f_lo
    else:
        a, b, fa, fb = bits(lo), bits(hi), f_lo, f_hi
        while b - a > 1:
            mid = a + (b - a) // 2
            fm = F(from_bits(mid))
            if fm >= T:
                b, fb = mid, fm
            else:
                a, fa = mid, fm
            iterations += 1
        x0, x1 = from_bits(a), from_bits(b)
        if fb == T:
            status, value, f_value = EXACT, x1, fb
        elif exact:
            status, value, f_value = REPAIRED, x0, fa
            k = T - fa
            delta = rows(text, dur, c, kind, x1, s_duration, s_pause) - rows(text, dur, c, kind, x0, s_duration, s_pause)
            assert (delta >= 0).all()
            total = int(delta.sum())
            assert total == fb - fa and total >= k > 0
            p = np.concatenate([[0], np.cumsum(delta)[:-1]]).astype(np.int64)
            for r in range(n):
                for t in range(int(p[r]), int(p[r] + delta[r])):
                    if ((t + 1) * k) // total > (t * k) // total:
                        extra[r] += 1
        else:
            upper = fb - T < T - fa
            status, value, f_value = NEAREST, (x1 if upper else x0), (fb if upper else fa)
    report = np.array([T, f_value + int(extra.sum()), f_value, value, status, iterations, int((extra > 0).sum()), f_base], dtype=np.float32)
    return dict(status=status, value=f32(value), extra=extra, report=report, x0=x0, x1=x1)


def fit(text, dur, lengths, segments, scales=None, curves=None):
    """The whole call: segments [n_seg, 8] (utterance, kind, begin, end, target, lo, hi, exact).  -> (scales_out [B, 4], curves_out
    [R, 5] or None, extra [R] int32, report [n_seg, 8], per-segment dicts of solve_one)."""
    B, R = len(lengths), int(sum(lengths))
    scales_out = np.ones((B, 4), dtype=np.float32) if scales is None else np.array(scales, dtype=np.float32)
    any_span = bool((np.asarray(segments)[:, 1] == SPAN).any())
    curves_out = None
    if curves is not None:
        curves_out = np.array(curves, dtype=np.float32)
    elif any_span:
        curves_out = np.tile(f32([1, 1, 1, 0, 0]), (R, 1))
    extra = np.zeros(R, dtype=np.int32)
    report = np.zeros((len(segments), 8), dtype=np.float32)
    solved = []
    for s, (u, kind, b, e, target, lo, hi, exact) in enumerate(np.asarray(segments)):
        u, kind, b, e = int(u), int(kind), int(b), int(e)
        c = np.ones(e - b, dtype=np.float32) if curves is None else np.asarray(curves, dtype=np.float32)[b:e, 0]
        sd, sp = (1.0, 1.0) if scales is None else (scales[u][0], scales[u][3])
        one = solve_one(text[b:e], dur[b:e], c, kind, target, lo, hi, bool(exact), sd, sp)
        solved.append(one)
        report[s] = one["report"]
        extra[b:e] = one["extra"]
        if one["status"] != EMPTY:
            if kind == SPAN:
                curves_out[b:e, 0] = c * one["value"]
            else:
                scales_out[u, 0 if kind == UTT_DURATION else 3] = one["value"]
    return scales_out, curves_out, extra, report, solved


def control_durations(text, dur, lengths, scales, curves):
    """The control kernel's durations for a batch with the given tables (either may be None)."""
    out = np.zeros(len(dur), dtype=np.int64)
    b = 0
    for u, n in enumerate(lengths):
        c = np.ones(n, dtype=np.float32) if curves is None else np.asarray(curves, dtype=np.float32)[b:b + n, 0]
        sd, sp = (1.0, 1.0) if scales is None else (scales[u][0], scales[u][3])
        out[b:b + n] = rows(text[b:b + n], dur[b:b + n], c, UTT_DURATION, sd, sd, sp)
        b += n
    return out


# ---- the seeded fixture -------------------------------------------------------------------------------------------------------------
# lengths: one row; less than a sweep of 256; a sweep and a tail of one; several sweeps and a tail
LENGTHS = [1, 7, 257, 1000, 7, 257, 1000, 257, 7, 1000, 257, 1000]
ALL_ZERO, NO_SILENCE, UNFITTED = 4, 5, 8  # utterances: every duration 0; no silence row (under the pause knob); no segment


def fixture():
    """text [R, 62], dur [R] int32, scales [B, 4], curves [R, 5], segments [n_seg, 8]: flags and durations drawn as in
    tests/test_gpu_prosody_scales.py; one all-zero utterance, one without silence rows under the pause knob, one without a segment;
    targets between 0.5x and 1.8x of the unscaled count, and some far outside the bounds."""
    rng = np.random.default_rng(41)
    R = sum(LENGTHS)
    begins = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(int)
    text = np.zeros((R, 62), dtype=np.float32)
    text[:, F_VOICED] = rng.random(R) < 0.6
    text[:, F_PHONEME] = rng.random(R) < 0.8
    text[:, F_WORD_BOUNDARY] = rng.random(R) < 0.15
    text[:, F_SILENCE] = rng.random(R) < 0.2
    dur = rng.integers(0, 13, R).astype(np.int32)
    sl = lambda u: slice(begins[u], begins[u + 1])
    text[0, F_WORD_BOUNDARY] = 0
    dur[0] = 5  # (the one-row utterance has frames to fit)
    dur[sl(ALL_ZERO)] = 0
    text[sl(NO_SILENCE), F_SILENCE] = 0
    scales = np.ones((len(LENGTHS), 4), dtype=np.float32)
    scales[2] = (1.7, 1.2, 0.9, 1.1)   # a pause fit under a duration scale above 1.5: one more frame of a pause becomes two
    scales[3] = (0.8, 1.0, 1.3, 0.6)   # a duration fit that starts from given scales
    scales[7] = (1.9, 1.0, 1.0, 1.0)
    curves = np.tile(f32([1, 1, 1, 0, 0]), (R, 1))
    # duration factors on one whole utterance and inside two spans; neutral elsewhere, so that tied durations stay tied there
    for u, a, b in ((1, 0, 7), (6, 0, 300), (11, 262, 999)):
        curves[begins[u] + a:begins[u] + b, 0] = (0.6 + 0.9 * rng.random(b - a)).astype(np.float32)
    curves[:, 1:3] = (0.8 + 0.4 * rng.random((R, 2))).astype(np.float32)
    base = lambda u, a=0, b=None: int(rows(text[sl(u)], dur[sl(u)], np.ones(LENGTHS[u], dtype=np.float32), UTT_DURATION, 1.0, 1.0, 1.0)[a:b].sum())
    seg = []
    add = lambda u, kind, a, b, target, lo, hi, exact: seg.append((u, kind, begins[u] + a, begins[u] + b, max(1, int(target)), lo, hi, exact))
    add(0, UTT_DURATION, 0, 1, 9, 0.25, 4.0, 1)
    add(1, UTT_DURATION, 0, 7, 1.37 * base(1), 0.25, 4.0, 0)
    add(2, UTT_PAUSE, 0, 257, 1.94 * base(2), 0.0, 8.0, 1)
    add(3, UTT_DURATION, 0, 1000, 1.23 * base(3), 0.25, 4.0, 1)
    add(ALL_ZERO, UTT_DURATION, 0, 7, 20, 0.25, 4.0, 1)
    add(NO_SILENCE, UTT_PAUSE, 0, 257, 1.2 * base(NO_SILENCE), 0.0, 8.0, 1)
    add(6, SPAN, 0, 300, 0.71 * base(6, 0, 300), 0.25, 4.0, 1)
    add(6, SPAN, 300, 301, 1, 0.25, 4.0, 1)
    add(6, SPAN, 420, 1000, 1.55 * base(6, 420, 1000), 0.25, 4.0, 0)
    add(7, UTT_PAUSE, 0, 257, 1.9 * base(7) + 0.4 * base(7), 0.5, 8.0, 0)
    add(9, UTT_DURATION, 0, 1000, 40 * base(9), 0.25, 4.0, 1)
    add(10, UTT_DURATION, 0, 257, 3, 0.5, 2.0, 1)
    add(11, SPAN, 5, 262, 1.8 * base(11, 5, 262), 0.25, 4.0, 1)
    add(11, SPAN, 262, 999, 0.5 * base(11, 262, 999), 0.25, 4.0, 1)
    return dict(text=text, dur=dur, scales=scales, curves=curves, segments=np.asarray(seg, dtype=np.float32), lengths=list(LENGTHS))
