"""Float64 restatement of the loudness meter (csrc/loudness.hip, include/toucan_loudness.h): ITU-R BS.1770-4 integrated loudness
with nothing parallel in it - two biquads one after the other, sample by sample, then the blocks and the two gates - the bound the
kernel's segment energies must meet, and the seeded signals the loudness tests share.  Nothing here imports the product's
loudness.py: the two are independent.

The bound on a segment energy e_k (derived, not measured).  u = 2^-53; X = max |x| of the utterance; r and r_s the pole radii of
the high-pass and of the shelf (sqrt of their a2); G = 1 / (1 - r)^2 and G_s = 1 / (1 - r_s)^2 bound the l1 norm of the impulse
response of a second-order recursion with poles of that radius (sum (n + 1) r^n).  Every rounding of the recurrence is u times a
value of at most A X (A = 32 covers every intermediate of both sections: their impulse responses have l1 norms below 3 and the
coefficients are below 3), at most 16 roundings per sample (the carry of the segment-parallel form included), and a rounding in the
shelf reaches the output through the shelf's recursion and the whole high-pass (numerator l1 norm 4): at most 4 G_s G.  So either
computation is within eps = 16 u A X 4 G_s G of the exact filtered signal at every sample, the two within 2 eps of each other, and
over the S samples of a segment (Cauchy-Schwarz on sum 2 |y| |dy| + dy^2, and S additions of relative error u each)

    |e_k - e_k_ref| <= 4 eps sqrt(S e_k) + 4 S eps^2 + 2 S u e_k.

It is a worst-case bound and generous by construction (rounding errors do not line up the way an l1 norm assumes); what it rules
out is a wrong coefficient, state or carry, which moves e_k by parts in 10^3.  The sharp check is the loudness itself, to 1e-6 LU.
"""
import functools
import math

import numpy as np

RATES = (8000, 16000, 22050, 24000, 48000)
U = 2.0 ** -53
A_INTERNAL, ROUNDINGS = 32.0, 16.0
ABSOLUTE_GATE, RELATIVE_GATE, OFFSET = -70.0, -10.0, -0.691
COLUMNS = ("lufs", "peak", "blocks", "blocks_abs", "blocks_both", "momentary_max_lufs", "gain", "lufs_after")
# BS.1770-4, tables 1 and 2: the coefficients at 48 kHz as printed
BS1770_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -1.69065929318241, 0.73248077421585),
              (1.0, -2.0, 1.0), (1.0, -1.99004745483398, 0.99007225036621))


def coefficients(sr):
    """((b, a), (b, a)) of the shelf and the high-pass at sr: bilinear transforms of the analogue prototypes, float64."""
    K = math.tan(math.pi * 1681.974450955533 / sr)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0), (1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / sr)
    Q = 0.5003270373238773
    d = 1.0 + K / Q + K * K
    return shelf, ((1.0, -2.0, 1.0), (1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d))


def biquad(x, b, a):
    """One biquad over the whole signal, sample by sample (direct form II transposed), Python floats = float64."""
    b0, b1, b2 = b
    _, a1, a2 = a
    s1 = s2 = 0.0
    out = [0.0] * len(x)
    for i, v in enumerate(x):
        y = b0 * v + s1
        s1 = b1 * v - a1 * y + s2
        s2 = b2 * v - a2 * y
        out[i] = y
    return out


def k_weight(x, sr, highpass=True):
    """The K-weighted signal, float64.  highpass=False leaves the second stage out (a deliberately wrong meter)."""
    shelf, high = coefficients(sr)
    y = biquad([float(v) for v in x], *shelf)
    return np.array(biquad(y, *high) if highpass else y, dtype=np.float64)


def segment_energies(y, S):
    """Sum of squares over every complete segment of S samples."""
    n = len(y) // S
    return (y[:n * S].reshape(n, S) ** 2).sum(axis=1) if n else np.zeros(0)


def block_loudness(z):
    with np.errstate(divide="ignore"):
        return OFFSET + 10.0 * np.log10(z)


def gate(e, S, relative=True):
    """Blocks of four segments, the absolute and (unless relative=False: a deliberately wrong meter) the relative gate ->
    dict(lufs, blocks, blocks_abs, blocks_both, momentary_max_lufs, l = the l_j, gamma = the relative threshold or None)."""
    nb = max(0, len(e) - 3)
    z = np.array([(e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * S) for j in range(nb)])
    l = block_loudness(z) if nb else np.zeros(0)
    keep = l > ABSOLUTE_GATE
    out = {"blocks": nb, "blocks_abs": int(keep.sum()), "l": l, "gamma": None, "momentary_max_lufs": float(l.max()) if nb else -math.inf}
    if not keep.any():
        return dict(out, lufs=-math.inf, blocks_both=0)
    gamma = OFFSET + 10.0 * math.log10(z[keep].mean()) + RELATIVE_GATE
    both = keep & (l > gamma) if relative else keep
    return dict(out, gamma=gamma, blocks_both=int(both.sum()), lufs=OFFSET + 10.0 * math.log10(z[both].mean()))


def loudness(x, sr, highpass=True, relative=True):
    """Integrated loudness of x (LUFS, -inf where there is none)."""
    S = sr // 10
    return gate(segment_energies(k_weight(x, sr, highpass), S), S, relative)["lufs"]


def gate_margin(g):
    """The least distance (LU) of a block from a gate threshold that decides about it: every block from -70, and every block past
    the absolute gate from the relative threshold."""
    l = g["l"][np.isfinite(g["l"])]
    m = float(np.abs(l - ABSOLUTE_GATE).min(initial=math.inf))
    if g["gamma"] is not None:
        m = min(m, float(np.abs(l[l > ABSOLUTE_GATE] - g["gamma"]).min(initial=math.inf)))
    return m


def pole_radius(sr):
    """(r, r_s): pole radii of the high-pass and of the shelf."""
    shelf, high = coefficients(sr)
    return math.sqrt(high[1][2]), math.sqrt(shelf[1][2])


def energy_bound(x, e, sr):
    """The bound of the module docstring for every e_k of the utterance x."""
    r, r_s = pole_radius(sr)
    S = sr // 10
    X = float(np.abs(x).max(initial=0.0))
    eps = ROUNDINGS * U * A_INTERNAL * X * 4.0 / ((1.0 - r_s) ** 2 * (1.0 - r) ** 2)
    return 4.0 * eps * np.sqrt(S * e) + 4.0 * S * eps * eps + 2.0 * S * U * e


def gain(lufs, peak, target, ceiling):
    """The gain of the definition before its rounding to float32, and whether the ceiling is what limits it."""
    if not math.isfinite(lufs) or peak == 0:
        return 1.0, False
    g, lim = 10.0 ** ((target - lufs) / 20.0), 10.0 ** (ceiling / 20.0) / peak
    return (lim, True) if lim < g else (g, False)


def sine_reading(sr, f, amplitude=1.0):
    """What a steady sine of frequency f reads: -0.691 + 10 log10(a^2 |H(e^jw)|^2 / 2)."""
    w = np.exp(-2j * math.pi * f / sr)
    h = 1.0
    for b, a in coefficients(sr):
        h = h * (b[0] + b[1] * w + b[2] * w * w) / (a[0] + a[1] * w + a[2] * w * w)
    return OFFSET + 10.0 * math.log10(amplitude ** 2 * abs(h) ** 2 / 2.0)


def noise(n, seed=0):
    """Seeded Gaussian noise x 0.3, clipped to +-1, float32."""
    return np.clip(0.3 * np.random.default_rng(2000 + seed).standard_normal(n), -1.0, 1.0).astype(np.float32)


def tone(n, sr, dbfs, f=997.0, start=0):
    return (10.0 ** (dbfs / 20.0) * np.sin(2.0 * math.pi * f * (start + np.arange(n)) / sr)).astype(np.float32)


def signals(sr, tile):
    """[(name, float32 wave)]: the lengths around four and five segments, nothing, silence, a sine with a partial last segment, a DC
    offset of 0.5 under a -30 dBFS tone (the high-pass has to take it out), one click (the peak ceiling limits its gain), a loud
    tone, silence and a tone 25 dB below it (the relative gate drops it), a tone below -70 LUFS (the absolute gate drops it); at
    8 kHz also noise of more segments than one workgroup (``tile``) and than two take."""
    S = sr // 10
    out = [(f"noise_{name}", noise(n, seed=i)) for i, (name, n) in
           enumerate((("4S-1", 4 * S - 1), ("4S", 4 * S), ("4S+1", 4 * S + 1), ("5S-1", 5 * S - 1), ("5S", 5 * S)))]
    out.append(("empty", np.zeros(0, dtype=np.float32)))
    out.append(("zeros", np.zeros(6 * S, dtype=np.float32)))
    out.append(("sine", tone(7 * S + 123, sr, -6.0)))
    out.append(("dc", (0.5 + tone(8 * S + 17, sr, -30.0)).astype(np.float32)))
    click = np.zeros(6 * S, dtype=np.float32)
    click[S // 2 + 3] = 1.0
    out.append(("click", click))
    out.append(("gates", np.concatenate([tone(20 * S, sr, -20.0), np.zeros(20 * S, dtype=np.float32), tone(20 * S, sr, -45.0, start=40 * S)])))
    out.append(("below_absolute", tone(6 * S, sr, -80.0)))
    if sr == 8000:
        out.append(("past_one_workgroup", noise((tile + 2) * S + 5, seed=11)))
        out.append(("past_two_workgroups", noise((2 * tile + 2) * S + 401, seed=12)))
    return out


@functools.lru_cache(maxsize=None)
def cases(sr, tile=64):
    """The shared, read-only reference of one rate: per signal the wave, e_k and their bounds, the peak per segment slot, the gate's
    results, the least distance of a block from a threshold."""
    S = sr // 10
    out = []
    for name, x in signals(sr, tile):
        e = segment_energies(k_weight(x, sr), S)
        g = gate(e, S)
        slots = -(-len(x) // S)
        peaks = np.array([np.abs(x[k * S:(k + 1) * S]).max() for k in range(slots)], dtype=np.float32)
        item = {"name": name, "n": len(x), "x": x, "e": e, "bound": energy_bound(x, e, sr), "peaks": peaks,
                "peak": float(peaks.max(initial=0.0)), "margin": gate_margin(g), **{k: g[k] for k in ("lufs", "blocks", "blocks_abs", "blocks_both",
                                                                                                      "momentary_max_lufs", "l", "gamma")}}
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(item)
    return tuple(out)
