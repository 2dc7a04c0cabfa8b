"""Float64 restatement of the delivery meter (csrc/truepeak.hip, include/toucan_truepeak.h): the true peak of ITU-R BS.1770-4
Annex 2 with the project's interpolator, the short-term loudness and the loudness range of EBU Tech 3341 / 3342, the gain under a
true-peak ceiling, and the seeded signals the true-peak tests share.  Nothing here imports the product's truepeak.py or
resample.py: the table is restated from its formula (Hann-windowed sinc, width 6, rolloff 0.99) and the CPU tests hold the two
against each other.

The bound on a true-peak reading (derived, not measured).  Every oversampled value of the kernel is one chain of K = 15 fp32
fused multiply-adds on float32 coefficients and samples; against the exact sum of the same products it is within
gamma_15 sum_j |k[p][j]| |x| <= gamma_15 A X, gamma_15 = 15 u / (1 - 15 u), u = 2^-24, A = max_p sum_j |k[p][j]|, X = max |x|.  A
maximum of values that are each within d of their counterparts is within d of the counterparts' maximum.
"""
import functools
import math

import numpy as np

from tests import loudness_ref as lr

WIDTH, ROLLOFF, HALF = 6, 0.99, 7
U32 = 2.0 ** -24
GAMMA_15 = 15 * U32 / (1 - 15 * U32)
SHORT_TERM = 30
ABSOLUTE_Z = 10.0 ** ((-70.0 + 0.691) / 10.0)
COLUMNS = ("true_peak", "true_peak_dbtp", "sample_peak", "short_term_max_lufs", "lra", "lra_low_lufs", "lra_high_lufs", "short_term_kept")
RATES = lr.RATES


def factor(sr):
    return 4 if sr < 96000 else 2 if sr < 192000 else 1


@functools.lru_cache(maxsize=None)
def table(F):
    """float32 [F, 15]: k[p][j] = 0.99 sinc(pi t) cos^2(pi t / 12), t = 0.99 (j - 7 - p / F) clipped to +-6; [[1]] for F = 1."""
    if F == 1:
        return np.ones((1, 1), dtype=np.float32)
    k = np.zeros((F, 2 * HALF + 1))
    for p in range(F):
        for j in range(2 * HALF + 1):
            t = min(max((-p / F + (j - HALF)) * ROLLOFF, -WIDTH), WIDTH)
            k[p, j] = (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)) * math.cos(t * math.pi / WIDTH / 2.0) ** 2 * ROLLOFF
    out = k.astype(np.float32)
    out.setflags(write=False)
    return out


def l1(F):
    """A: the largest sum_j |k[p][j]| of a phase."""
    return float(np.abs(table(F).astype(np.float64)).sum(axis=1).max())


def oversample(x, F):
    """float64 [F n]: o[F i + p] = sum_j k[p][j] x[i + j - w], x = 0 outside the utterance; the products of float32 values are
    exact in float64, their sum is rounded at 2^-53."""
    k = table(F).astype(np.float64)
    w = (k.shape[1] - 1) // 2
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    pad = np.concatenate([np.zeros(w), x, np.zeros(w)])
    o = np.zeros((n, F))
    for j in range(k.shape[1]):
        o += pad[j:j + n, None] * k[None, :, j]
    return o.reshape(-1)


def true_peak(x, sr):
    return float(np.abs(oversample(x, factor(sr))).max(initial=0.0))


def bound(x, sr):
    """What the kernel's reading may differ from ``true_peak`` by."""
    return GAMMA_15 * l1(factor(sr)) * float(np.abs(np.asarray(x, dtype=np.float64)).max(initial=0.0))


def db(v):
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def short_term(e, S):
    """zs_j, float64: 30 segment energies added in index order, over 30 S."""
    e = np.asarray(e, dtype=np.float64)
    nb = max(0, len(e) - (SHORT_TERM - 1))
    if nb == 0:
        return np.zeros(0)
    s = e[:nb].copy()
    for k in range(1, SHORT_TERM):
        s = s + e[k:k + nb]
    return s / (float(SHORT_TERM) * float(S))


def loudness_range(zs, relative=True, floor=False):
    """The gates and the two order statistics of the zs -> dict(lra, low, high (z, 0 without), low_lufs, high_lufs, kept, kept_abs,
    blocks, short_term_max_lufs, thresholds, sorted).  relative=False leaves the relative gate out and floor=True drops the + 50 of
    the percentile index: two deliberately wrong meters."""
    zs = np.asarray(zs, dtype=np.float64)
    out = {"blocks": len(zs), "short_term_max_lufs": float(lr.block_loudness(zs.max())) if len(zs) and zs.max() > 0 else -math.inf}
    keep = zs > ABSOLUTE_Z
    thresholds = [ABSOLUTE_Z]
    if keep.any() and relative:
        m = 0.0
        for z in zs[keep]:  # index order
            m += z
        thresholds.append(m / int(keep.sum()) / 100.0)
    both = keep & (zs > max(thresholds))
    srt = np.sort(zs[both])
    n = len(srt)
    out.update(kept_abs=int(keep.sum()), kept=n, thresholds=thresholds, sorted=srt)
    if n == 0:
        return dict(out, lra=0.0, low=0.0, high=0.0, low_lufs=-math.inf, high_lufs=-math.inf, i_low=None, i_high=None)
    i_low, i_high = ((n - 1) * 10 + (0 if floor else 50)) // 100, ((n - 1) * 95 + (0 if floor else 50)) // 100
    low, high = float(srt[i_low]), float(srt[i_high])
    return dict(out, lra=10.0 * math.log10(high / low), low=low, high=high, low_lufs=-0.691 + 10.0 * math.log10(low),
                high_lufs=-0.691 + 10.0 * math.log10(high), i_low=i_low, i_high=i_high)


def range_margins(r):
    """(the least distance in LU of a short-term block from a gate threshold that decides about it, the least relative distance of
    the two order statistics from a sorted neighbour that differs from them)."""
    zs = r["zs"]
    pos = zs[zs > 0]
    gate = math.inf
    for i, thr in enumerate(r["thresholds"]):
        cand = pos if i == 0 else pos[pos > ABSOLUTE_Z]
        gate = min(gate, float(np.abs(10.0 * np.log10(cand / thr)).min(initial=math.inf)))
    order = math.inf
    srt = r["sorted"]
    for i in (r["i_low"], r["i_high"]):
        if i is None:
            continue
        for nb in (i - 1, i + 1):
            if 0 <= nb < len(srt) and srt[nb] != srt[i]:
                order = min(order, abs(srt[nb] - srt[i]) / srt[i])
    return gate, order


def pure_gain(lufs, peak, tp, target, ceiling, tp_ceiling):
    """min(10^((L_t - L) / 20), C_s / peak, C_tp / tp) before any rounding, 1 without a loudness or a peak."""
    if not math.isfinite(lufs) or peak == 0 or tp == 0:
        return 1.0
    return min(10.0 ** ((target - lufs) / 20.0), 10.0 ** (ceiling / 20.0) / peak, 10.0 ** (tp_ceiling / 20.0) / tp)


# ---- signals

def faded_sine(sr, f, phase_deg, amplitude, seconds=0.4):
    """A sine with a 50 ms raised-cosine fade in and out (a hard onset has a true transient of its own), float32."""
    n = int(seconds * sr)
    t = np.arange(n, dtype=np.float64)
    x = amplitude * np.sin(2.0 * math.pi * f * t / sr + math.radians(phase_deg))
    nf = int(0.05 * sr)
    ramp = 0.5 - 0.5 * np.cos(math.pi * np.arange(nf) / nf)
    x[:nf] *= ramp
    x[n - nf:] *= ramp[::-1]
    return x.astype(np.float32)


SINES = (("fs/4 0", 4, 0.0), ("fs/4 45", 4, 45.0), ("fs/6 60", 6, 60.0), ("fs/8 67.5", 8, 67.5))
AMPLITUDES = (0.5, 10.0 ** (-3.0 / 20.0))


def speech_like(n, sr, seed=0):
    """1 / f-shaped noise under a slow envelope, peak 0.9, float32."""
    rng = np.random.default_rng(4000 + seed)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / sr)
    spec[1:] /= np.sqrt(np.maximum(f[1:], 50.0))
    spec[0] = 0.0
    x = np.fft.irfft(spec, n)
    env = 0.55 + 0.45 * np.sin(2.0 * math.pi * 3.1 * np.arange(n) / sr + 0.7) * np.sin(2.0 * math.pi * 0.43 * np.arange(n) / sr)
    x = x * env
    return (0.9 * x / np.abs(x).max()).astype(np.float32)


def peak_signals(tile, sr=8000):
    """[(name, float32 wave)] for the true-peak kernel: the lengths around the taps and the halo (w = 7, K = 15), around one and two
    tiles, the peak in the first sample, in the last, and between the last sample of one tile and the first of the next, a click,
    DC, the fs/4 45 degree sine and seeded noise."""
    out = [(f"noise_{n}", lr.noise(n, seed=20 + n)) for n in (0, 1, 6, 7, 8, 14, 15, 16)]
    out += [(f"noise_{name}", lr.noise(n, seed=40 + i)) for i, (name, n) in
            enumerate((("T-1", tile - 1), ("T", tile), ("T+1", tile + 1), ("2T+1", 2 * tile + 1)))]
    first = 0.05 * lr.noise(tile + 40, seed=50)
    first[0] = 0.9
    out.append(("peak_first", first))
    last = 0.05 * lr.noise(tile + 40, seed=51)
    last[-1] = -0.9
    out.append(("peak_last", last))
    gap = 0.05 * lr.noise(2 * tile + 3, seed=52)
    gap[tile - 1] = gap[tile] = 0.7  # the largest value lies half-way between them, and belongs to the first tile's last sample
    out.append(("peak_in_the_gap_at_a_tile_edge", gap))
    click = np.zeros(300, dtype=np.float32)
    click[123] = 1.0
    out.append(("click", click))
    out.append(("dc", np.full(200, 0.5, dtype=np.float32)))
    out.append(("sine_fs4_45", faded_sine(sr, sr / 4.0, 45.0, 0.5, seconds=0.3)))
    out.append(("noise_long", lr.noise(3 * tile + 517, seed=53)))
    return [(name, np.ascontiguousarray(x, dtype=np.float32)) for name, x in out]


@functools.lru_cache(maxsize=None)
def peak_cases(tile, sr=8000):
    """The shared, read-only reference: per signal the wave, the float64 true peak, its bound, the sample peak."""
    out = []
    for name, x in peak_signals(tile, sr):
        x.setflags(write=False)
        out.append({"name": name, "x": x, "n": len(x), "true_peak": true_peak(x, sr), "bound": bound(x, sr),
                    "sample_peak": float(np.abs(x).max(initial=0.0))})
    return tuple(out)


def two_levels(levels_dbfs, seconds=20, sr=8000, f=1000):
    """A sine of ``f`` Hz, ``seconds`` at each of the levels in turn, float32.  ``sr / f`` is a whole number of samples and every
    level is one rounded period repeated, so that the samples of a level are exactly periodic: the short-term blocks inside a level
    then come out equal in float64 once the filter has settled, not apart by a rounding error."""
    assert sr % f == 0
    period = np.sin(2.0 * math.pi * np.arange(sr // f) / (sr // f))
    return np.concatenate([np.tile((10.0 ** (level / 20.0) * period).astype(np.float32), seconds * f) for level in levels_dbfs])


LRA_CASES = ((("-20 -30", (-20.0, -30.0)), 10.0), (("-20 -15", (-20.0, -15.0)), 5.0), (("-40 -20", (-40.0, -20.0)), 20.0),
             (("-50 -35 -20 -35 -50", (-50.0, -35.0, -20.0, -35.0, -50.0)), 15.0))


@functools.lru_cache(maxsize=None)
def lra_case(i, sr=8000):
    """dict(name, x, e, zs, want, and loudness_range's results) of analytic case i."""
    (name, levels), want = LRA_CASES[i]
    x = two_levels(levels, sr=sr)
    S = sr // 10
    e = lr.segment_energies(lr.k_weight(x, sr), S)
    zs = short_term(e, S)
    for a in (x, e, zs):
        a.setflags(write=False)
    return dict(loudness_range(zs), name=name, x=x, e=e, zs=zs, want=want)


def synthetic_energies(n_blocks, S, seed, quiet=0):
    """Segment energies whose ``n_blocks`` short-term blocks (0: 29 segments, no block) all pass both gates, spread over about
    6 LU; ``quiet`` > 0 appends that many segments 40 dB down, whose blocks the relative gate drops."""
    rng = np.random.default_rng(6000 + seed)
    n = n_blocks + SHORT_TERM - 1 if n_blocks else SHORT_TERM - 1
    e = S * 1e-3 * 10.0 ** (rng.uniform(-0.6, 0.6, n))
    if quiet:
        e = np.concatenate([e, S * 1e-7 * 10.0 ** (rng.uniform(-0.1, 0.1, quiet))])
    return e


@functools.lru_cache(maxsize=None)
def range_cases(S=800):
    """The shared, read-only cases of the range kernel as segment energies: n short-term blocks past both gates for n around the
    percentile indices' steps, one wavefront's sweep (64) and two, with and without blocks that the relative gate drops, more
    blocks than the kernel keeps in LDS, 29 segments (no block) and blocks that all lie under the absolute gate."""
    out = []
    for i, n in enumerate((0, 1, 2, 10, 11, 64, 65, 129, 200)):
        out.append((f"kept_{n}", synthetic_energies(n, S, i)))
    out.append(("kept_65_and_quiet", synthetic_energies(65, S, 20, quiet=70)))
    out.append(("kept_11_and_quiet", synthetic_energies(11, S, 21, quiet=31)))
    out.append(("kept_2100", synthetic_energies(2100, S, 23)))  # more than the kernel keeps in LDS (2 048): its other path
    out.append(("under_the_absolute_gate", synthetic_energies(12, S, 22) * 1e-6))
    cases = []
    for name, e in out:
        zs = short_term(e, S)
        for a in (e, zs):
            a.setflags(write=False)
        cases.append(dict(loudness_range(zs), name=name, e=e, zs=zs))
    return tuple(cases)


# ---- the fp32 chain, the stepped gain and the limiter, as the kernels run them

def chain32(x, F):
    """float32 [n, F]: every oversampled value as the kernel's chain of fp32 fused multiply-adds in j order.  A fused multiply-add
    is restated as the float64 sum of the exact product (two float32 factors: 48 bits) and the accumulator, rounded to float32; the
    float64 rounding in between can change the result only where the exact value lies within 2^-29 of its size of a float32
    rounding boundary."""
    k = table(F)
    w = (k.shape[1] - 1) // 2
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    pad = np.concatenate([np.zeros(w), x.astype(np.float64), np.zeros(w)])
    acc = np.zeros((n, F), dtype=np.float32)
    for j in range(k.shape[1]):
        acc = (k[None, :, j].astype(np.float64) * pad[j:j + n, None] + acc.astype(np.float64)).astype(np.float32)
    return acc


def reading32(x, sr):
    """The meter's own reading: max |chain32|, float32 as a float."""
    return float(np.abs(chain32(x, factor(sr))).max(initial=0.0))


def stepped_gain(x, sr, gain_loudness, tp_ceiling, max_steps=128):
    """(g float32, steps): min(g_l, fl32(C / T)) stepped towards zero until the reading of fl32(x g) is <= C."""
    C = 10.0 ** (tp_ceiling / 20.0)
    T = reading32(x, sr)
    g = min(np.float32(gain_loudness), np.float32(min(C / T, 3.4028234663852886e38)))
    steps = 0
    while reading32(np.asarray(x, dtype=np.float32) * g, sr) > C and steps < max_steps:
        g = np.nextafter(g, np.float32(0.0))
        steps += 1
    return g, steps


def limiter(x, sr, lufs, target, ceiling, tp_ceiling):
    """Steps 1 - 7 of include/toucan_truepeak.h -> dict(y, y1 (before the trim), v, m, r, h, g, g0, C, W, tp1, t)."""
    x = np.asarray(x, dtype=np.float32)
    n, F, W = len(x), factor(sr), sr // 500
    C = 10.0 ** (min(ceiling, tp_ceiling) / 20.0)
    if not math.isfinite(lufs):
        one = np.ones(n)
        return dict(y=x.copy(), y1=x.copy(), v=x.copy(), m=np.zeros(n, dtype=np.float32), r=one, h=one, g=one, g0=np.float32(1.0), C=C, W=W,
                    tp1=max(reading32(x, sr), float(np.abs(x).max(initial=0.0))), t=np.float32(1.0))
    g0 = np.float32(min(10.0 ** ((target - lufs) / 20.0), 3.4028234663852886e38))
    v = x * g0
    o = np.abs(chain32(v, F))
    m = np.maximum(o.max(axis=1), np.abs(v)) if n else np.zeros(0, dtype=np.float32)
    if F > 1 and n > 1:
        m[1:] = np.maximum(m[1:], o[:-1, 1:].max(axis=1))
    with np.errstate(divide="ignore"):
        r = np.where(m > 0, np.minimum(1.0, C / m.astype(np.float64)), 1.0)
    # h[k] for k = -W .. n - 1: the minimum of r over k .. k + W, r = 1 outside the utterance (hp[k + W] = h[k])
    rp = np.concatenate([np.ones(W), r, np.ones(W)])
    hp = rp[:n + W].copy()
    for d in range(1, W + 1):
        hp = np.minimum(hp, rp[d:d + n + W])
    h = hp[W:]
    g = hp[:n].copy()
    for d in range(1, W + 1):
        g = g + hp[d:d + n]
    g = g / float(W + 1)
    y1 = v * g.astype(np.float32)
    tp1 = max(reading32(y1, sr), float(np.abs(y1).max(initial=0.0)))
    t = np.float32(1.0) if tp1 <= C else np.float32((C / tp1) * (1.0 - 2.0 ** -16))
    return dict(y=y1 * t, y1=y1, v=v, m=m, r=r, h=h, g=g, g0=g0, C=C, W=W, tp1=tp1, t=t)


@functools.lru_cache(maxsize=None)
def limiter_cases(sr=8000, tile=1024):
    """[(name, float32 wave)]: speech-like signals of 1.5 s - 30 blocks of 400 ms... enough for a loudness - that a loud target
    drives 1, 3 and 6 dB into the ceiling, one that stays under it, a click train, and lengths around a tile."""
    base = speech_like(int(1.2 * sr), sr, seed=1)
    out = [("speech", base), ("speech_T+1", speech_like(max(tile + 1, 5 * sr // 10 + 3), sr, seed=2)),
           ("speech_2T+W", speech_like(2 * tile + sr // 500 + 5, sr, seed=3))]
    clicks = 0.02 * lr.noise(int(0.8 * sr), seed=60)
    clicks[sr // 10::sr // 7] = 0.95
    clicks[sr // 10 + 1::sr // 7] = 0.9
    out.append(("clicks", clicks.astype(np.float32)))
    out.append(("quiet_sine", faded_sine(sr, 440.0, 0.0, 0.05, seconds=0.7)))
    for _, x in out:
        x.setflags(write=False)
    return tuple(out)
