"""Float64 restatement of the pitch tracker (Boersma 1993's autocorrelation method with Praat's documented defaults, as
PitchCalculator.py:64-67 calls it: time step 256/16000, floor 40 Hz, ceiling 600 Hz) written from the definition in DESIGN.md
section 12, and the seeded signals the pitch tests share.  Nothing here imports the product's pitch.py: the two are independent
statements of the same definition.  PARITY UNPINNED: Praat itself is not available to compare against."""
import functools
import math

import numpy as np

SR, HOP = 16000, 256
FLOOR, CEILING = 40.0, 600.0
SILENCE_T, VOICING_T, OCTAVE_COST, JUMP_COST, VUV_COST = 0.03, 0.45, 0.01, 0.35, 0.14
MAX_CAND = 15
NPER = SR // 40  # 400
HPER = NPER // 2 + 1  # 201
HW = int(math.floor(0.075 * SR)) // 2 - 1  # 599
NW = 2 * HW  # 1198
MAXLAG = NW // 3 + 2  # 401
BIX = NW // 2  # 599
MIN_SAMPLES = 1200
GOLD = (math.sqrt(5.0) - 1.0) / 2.0
GOLD_STEPS = 45  # 2 * GOLD**45 < 1e-9


def frame_count(n):
    """floor((n dx - 0.075) / dt) + 1 in exact arithmetic: floor((n - 1200) / 256) + 1."""
    if n < MIN_SAMPLES:
        raise ValueError(f"{n} samples: the analysis window of 3 periods of 40 Hz needs {MIN_SAMPLES}")
    return (n - MIN_SAMPLES) // HOP + 1


def frame_left(n):
    """Low sample of every frame centre, floor(t / dx - 0.5) with t = 0.5 n dx - 0.5 nfr dt + 0.5 dt + f dt, in exact arithmetic:
    t / dx - 0.5 = (n - 256 nfr + 255) / 2 + 256 f."""
    nfr = frame_count(n)
    return (n - HOP * nfr + HOP - 1) // 2 + HOP * np.arange(nfr, dtype=np.int64)


def frame_times(n):
    nfr = frame_count(n)
    dx, dt = 1.0 / SR, HOP / SR
    return 0.5 * n * dx - 0.5 * nfr * dt + 0.5 * dt + np.arange(nfr) * dt


@functools.lru_cache(maxsize=None)
def window():
    """(win [NW], wr [BIX + 1]): the Hanning window and its autocorrelation normalised to wr[0] = 1."""
    j = np.arange(NW, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * (j + 1.0) / (NW + 1.0))
    wr = np.array([np.dot(win[: NW - k], win[k:]) for k in range(BIX + 1)])
    return win, wr / wr[0]


def sinc_interp(R, rows, x, depth):
    """S_D(x[k]) on row rows[k] of R [F, BIX + 1]: Hann-windowed sinc interpolation of r[-BIX .. BIX] (r[-k] = r[k]) with at most
    `depth` samples either side of x, fewer where r ends.  sin(pi (x - m)) is taken as (-1)^k sin(pi frac(x)) for the k-th sample on
    either side: the same number, one sine per point instead of one per term."""
    x = np.asarray(x, dtype=np.float64)
    l = np.floor(x).astype(np.int64)
    dep = np.minimum(np.minimum(depth, l + BIX + 1), BIX - l)[:, None]
    k = np.arange(depth)[None, :]
    sign = np.where(k % 2 == 0, 1.0, -1.0)
    xc, lc = x[:, None], l[:, None]
    total = np.zeros(len(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        for m, dist, width in ((lc - k, xc - lc, xc - (lc + 1 - dep) + 1.0), (lc + 1 + k, lc + 1 - xc, (lc + dep) - xc + 1.0)):
            a = np.pi * (dist + k)  # pi |x - m|
            term = R[rows[:, None], np.minimum(np.abs(m), BIX)] * (sign * np.sin(np.pi * dist)) / a * (0.5 + 0.5 * np.cos(a / width))
            total += np.where(k < dep, term, 0.0).sum(axis=1)
    return np.where(x == l, R[rows, np.minimum(np.abs(l), BIX)], total)


def refine(R, rows, lags):
    """Maximise S70 over [i - 1, i + 1] by golden section for every (row, lag i): GOLD_STEPS steps bring the bracket under 1e-9.
    -> (x, S70(x))."""
    f = lambda x: sinc_interp(R, rows, x, 70)
    a, b = lags - 1.0, lags + 1.0
    c, d = b - GOLD * (b - a), a + GOLD * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(GOLD_STEPS):
        lo = fc >= fd  # the maximum lies in [a, d]; else in [c, b]
        a, b = np.where(lo, a, c), np.where(lo, d, b)
        c2, d2 = b - GOLD * (b - a), a + GOLD * (b - a)
        fn = f(np.where(lo, c2, d2))  # one new point per bracket
        c, d, fc, fd = c2, d2, np.where(lo, fn, fd), np.where(lo, fc, fn)
    x = 0.5 * (a + b)
    return x, f(x)


def frame_correlation(x, gpeak, left):
    """One frame of the mean-free wave x (float64): (r [BIX + 1], r[0] = 1 alone when the frame is empty; intensity)."""
    win, wr = window()
    right = left + 1
    local_mean = x[right - NPER: left + NPER + 1].mean()
    seg = (x[right - HW: right - HW + NW] - local_mean) * win
    lp = np.abs(seg[HW - HPER: HW + HPER]).max()
    intensity = min(1.0, lp / gpeak) if gpeak > 0 else 0.0
    ac = np.correlate(np.concatenate([seg, np.zeros(BIX)]), seg, "valid")  # ac[k] = sum_j seg[j] seg[j + k], k = 0 .. BIX
    if ac[0] == 0:
        return np.eye(1, BIX + 1)[0], intensity
    return ac / (ac[0] * wr), intensity


def maxima(r):
    """-> (lags i of the voiced candidates of one frame, fragile)."""
    half = 0.5 * VOICING_T
    i = np.arange(2, min(MAXLAG, BIX))
    c, lo, hi = r[i], r[i - 1], r[i + 1]
    would_be = (c > half - 1e-4) & (c > lo - 1e-5) & (c >= hi - 1e-5)
    close = (np.abs(c - half) < 1e-4) | (np.abs(c - lo) < 1e-5) | (np.abs(c - hi) < 1e-5)
    return i[(c > half) & (c > lo) & (c >= hi)], bool((would_be & close).any())


def viterbi(freq, strength, n_cand):
    """freq, strength: [F, 15]; n_cand [F].  -> (f0 [F] float64, margin [F]): the maximising path (first maximum on ties) and, per
    frame, the smallest gap between the chosen and the next best alternative among the decisions taken on the path at that frame."""
    freq, strength = np.asarray(freq, dtype=np.float64), np.asarray(strength, dtype=np.float64)
    F = len(n_cand)
    corr = OCTAVE_COST / (HOP / SR)
    unv = lambda f: f == 0.0 or f > CEILING

    def local(f, s):
        if f == 0.0:
            return s
        return 0.0 if f > CEILING else s - OCTAVE_COST * math.log2(CEILING / f)

    def cost(f1, f2):
        u1, u2 = unv(f1), unv(f2)
        if u1 and u2:
            return 0.0
        if u1 != u2:
            return VUV_COST * corr
        return JUMP_COST * corr * abs(math.log2(f1 / f2))

    delta = [local(freq[0, c], strength[0, c]) for c in range(n_cand[0])]
    back, gaps = [], []
    for t in range(1, F):
        new, bp, gap = [], [], []
        for c in range(n_cand[t]):
            vals = [delta[p] - cost(freq[t - 1, p], freq[t, c]) for p in range(n_cand[t - 1])]
            best = int(np.argmax(vals))  # the first maximum
            rest = vals[:best] + vals[best + 1:]
            gap.append(vals[best] - max(rest) if rest else np.inf)
            new.append(vals[best] + local(freq[t, c], strength[t, c]))
            bp.append(best)
        delta = new
        back.append(bp)
        gaps.append(gap)
    c = int(np.argmax(delta))
    rest = delta[:c] + delta[c + 1:]
    f0, margin = np.zeros(F), np.full(F, np.inf)
    margin[F - 1] = delta[c] - max(rest) if rest else np.inf
    for t in range(F - 1, -1, -1):
        f0[t] = 0.0 if unv(freq[t, c]) else freq[t, c]
        if t > 0:
            margin[t] = min(margin[t], gaps[t - 1][c])
            c = back[t - 1][c]
    return f0, margin


def analyse(wave):
    """The whole restatement for one float32 wave: dict of f0 [F], freq / strength / lag [F, 15] (candidates: the unvoiced one, then
    by lag), n_cand [F], fragile [F], margin [F], r [F, BIX + 1]."""
    x = np.asarray(wave, dtype=np.float64).reshape(-1)
    lefts = frame_left(len(x))
    F = len(lefts)
    x = x - x.mean()
    gpeak = np.abs(x).max()
    R, intensity, fragile = np.zeros((F, BIX + 1)), np.zeros(F), np.zeros(F, dtype=bool)
    rows, lags = [], []
    for t, left in enumerate(lefts):
        R[t], intensity[t] = frame_correlation(x, gpeak, int(left))
        i, fragile[t] = maxima(R[t])
        rows.append(np.full(len(i), t))
        lags.append(i)
    rows, lags = np.concatenate(rows), np.concatenate(lags)
    # first strength at the parabola's vertex, then the best 14 per frame by strength - octave cost (ties: the smaller lag)
    c, lo, hi = R[rows, lags], R[rows, lags - 1], R[rows, lags + 1]
    xv = lags + 0.5 * (hi - lo) / (2.0 * c - lo - hi)
    s = sinc_interp(R, rows, xv, 30)
    s = np.where(s > 1.0, 1.0 / s, s)
    score = s - OCTAVE_COST * np.log2(FLOOR / (SR / xv))
    keep = np.ones(len(rows), dtype=bool)
    for t in np.nonzero(np.bincount(rows, minlength=F) > MAX_CAND - 1)[0]:
        k = np.nonzero(rows == t)[0]
        order = sorted(k, key=lambda q: (-score[q], lags[q]))
        keep[order[MAX_CAND - 1:]] = False
    rows, lags = rows[keep], lags[keep]
    xr, sr = refine(R, rows, lags)
    sr = np.where(sr > 1.0, 1.0 / sr, sr)
    freq, strength = np.zeros((F, MAX_CAND)), np.zeros((F, MAX_CAND))
    lag, n_cand = np.zeros((F, MAX_CAND), dtype=np.int32), np.ones(F, dtype=np.int32)
    strength[:, 0] = VOICING_T + np.maximum(0.0, 2.0 - intensity / (SILENCE_T / (1.0 + VOICING_T)))
    for t, i, xx, ss in zip(rows, lags, xr, sr):  # rows and lags ascend
        freq[t, n_cand[t]], strength[t, n_cand[t]], lag[t, n_cand[t]] = SR / xx, ss, i
        n_cand[t] += 1
    f0, margin = viterbi(freq, strength, n_cand)
    return {"f0": f0, "freq": freq, "strength": strength, "lag": lag, "n_cand": n_cand, "fragile": fragile, "margin": margin, "r": R}


# ---- seeded signals ---------------------------------------------------------------------------------------------------------
def harmonic(f0_track, rng, n_harm=6, amplitude=0.1, noise=0.002):
    """Six harmonics with random amplitudes and phases on the instantaneous frequency f0_track [n] (Hz), peak `amplitude`, plus
    white noise."""
    phase = 2.0 * np.pi * np.cumsum(f0_track) / SR
    amps = rng.uniform(0.3, 1.0, n_harm) / np.arange(1, n_harm + 1)
    x = sum(a * np.sin(h * phase + th) for h, a, th in zip(range(1, n_harm + 1), amps, rng.uniform(0, 2 * np.pi, n_harm)))
    x = amplitude * x / np.abs(x).max()
    return x + noise * rng.standard_normal(len(x))


def glide(seed, seconds=1.2, gap=0.15, offset=0.0, lo=70.0, hi=400.0):
    """-> (wave float32 [n], analytic f0 [n], voiced mask [n]): f0 gliding linearly between two draws from lo .. hi Hz with a 3 Hz
    vibrato of +-8 Hz, and a silent gap (noise only) of `gap` of the length in the middle."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * SR))
    t = np.arange(n) / SR
    fa, fb = rng.uniform(lo, hi, 2)
    f0 = fa + (fb - fa) * t / seconds + 8.0 * np.sin(2.0 * np.pi * 3.0 * t)
    x = harmonic(f0, rng, noise=0.0)
    voiced = np.ones(n, dtype=bool)
    g0, g1 = int(n * (0.5 - gap / 2)), int(n * (0.5 + gap / 2))
    voiced[g0:g1] = False
    x = np.where(voiced, x, 0.0) + 0.002 * rng.standard_normal(n) + offset
    return x.astype(np.float32), f0, voiced


def steady(freq, seconds=1.2, seed=0):
    rng = np.random.default_rng(1000 + seed)
    n = int(round(seconds * SR))
    f0 = np.full(n, float(freq))
    return harmonic(f0, rng).astype(np.float32), f0, np.ones(n, dtype=bool)


def step(seed=0, seconds=1.2):
    """200 Hz, then 100 Hz from the middle on."""
    rng = np.random.default_rng(2000 + seed)
    n = int(round(seconds * SR))
    f0 = np.where(np.arange(n) < n // 2, 200.0, 100.0)
    clean = np.ones(n, dtype=bool)
    clean[n // 2] = False  # a window across the jump has no single analytic frequency: it is not "fully voiced"
    return harmonic(f0, rng).astype(np.float32), f0, clean


def window_state(n, mask):
    """Per frame: (every sample of its window is voiced, no sample of its window is voiced)."""
    lefts = frame_left(n)
    c = np.concatenate([[0], np.cumsum(mask)])
    inside = c[lefts + 1 - HW + NW] - c[lefts + 1 - HW]
    return inside == NW, inside == 0


GLIDE_SEEDS = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def signals():
    """name -> (wave, analytic f0 or None, voiced mask or None).  Ragged lengths; every one is short except `long40`."""
    s = {f"glide{k}": glide(k) for k in GLIDE_SEEDS}
    s["dc"] = glide(11, offset=0.5)
    s["low45"] = steady(45.0)
    s["high580"] = steady(580.0)
    s["step"] = step()
    s["zeros"] = (np.zeros(int(1.0 * SR), dtype=np.float32), None, None)
    w, f0, v = glide(12, seconds=0.5, gap=0.0)
    s["shortest"] = (w[:MIN_SAMPLES].copy(), f0[:MIN_SAMPLES], v[:MIN_SAMPLES])
    s["odd"] = tuple(a[:15555] for a in glide(13))
    return s


SHORT = ("glide1", "glide2", "glide3", "glide4", "dc", "low45", "high580", "step", "zeros", "shortest", "odd")


@functools.lru_cache(maxsize=None)
def long40():
    """40 s: 2496 frames, past what the path kernel keeps in LDS.  A low voice: two or three candidates per frame keep the
    restatement quick."""
    return glide(21, seconds=40.0, gap=0.1, lo=80.0, hi=120.0)


@functools.lru_cache(maxsize=None)
def analysed(name):
    """The restatement of one signal, computed once per process and shared (read-only) by the tests."""
    wave = long40()[0] if name == "long40" else signals()[name][0]
    out = analyse(wave)
    for v in out.values():
        v.setflags(write=False)
    return out
