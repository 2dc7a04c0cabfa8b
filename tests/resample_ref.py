"""Float64 restatement of the sample-rate converter (csrc/resample.hip), the bound its float32 results must meet, and the seeded
signals the resampling tests share.  The filter is torchaudio.transforms.Resample's (Hann window, lowpass_filter_width 6, rolloff
0.99), written from the formula the way ``style.resample_sinc`` writes it but without the final cast to float32.  Nothing here
imports the product's resample.py: the two are independent.

The bound (derived, not measured): with k the float64 table, x the float32 input and u = 2^-24,

    |y - y_ref| <= (K + 2) u sum_j |k[p][j]| |x_j|.

The kernel rounds every coefficient to float32 once (relative error u), forms K products and K - 1 sums (each a relative error
of at most u, fused or not, in any order): every term carries at most (1 + u)^(K + 1) - 1 <= (K + 1) u / (1 - (K + 1) u)
<= (K + 2) u for the K in use (K <= 475: (K + 1)(K + 2) u < 1).
"""
import functools
import math

import numpy as np

WIDTH, ROLLOFF = 6, 0.99
U = 2.0 ** -24

# conversion -> (orig, new, K), the ratios the tests cover: tables from 120 B to 304 KB
RATIOS = {
    (24000, 48000): (1, 2, 15),
    (24000, 16000): (3, 2, 23),
    (24000, 8000): (3, 1, 41),
    (24000, 44100): (80, 147, 94),
    (24000, 22050): (160, 147, 174),
    (44100, 16000): (441, 160, 475),
    (16000, 24000): (2, 3, 16),
}


def table(sr_in, sr_out):
    """(orig, new, w, k float64 [new, K])."""
    g = math.gcd(int(sr_in), int(sr_out))
    orig, new = int(sr_in) // g, int(sr_out) // g
    base = min(orig, new) * ROLLOFF
    w = int(math.ceil(WIDTH * orig / base))
    idx = np.arange(-w, w + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -WIDTH, WIDTH)
    window = np.cos(t * np.pi / WIDTH / 2.0) ** 2
    t = t * np.pi
    kern = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)
    return orig, new, w, kern


def out_length(n, sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    return int(math.ceil((int(sr_out) // g) * int(n) / (int(sr_in) // g)))


def _apply(x, kern, orig, w, count):
    """sum_j kern[p][j] x[i orig + j - w] for the first `count` outputs m = i new + p, x zero outside its length."""
    new, K = kern.shape
    blocks = -(-count // new)
    xp = np.zeros(w + max(len(x), blocks * orig) + w + orig, dtype=np.float64)
    xp[w:w + len(x)] = x
    cols = np.arange(K)[None, :] + orig * np.arange(blocks)[:, None]
    return (xp[cols] @ kern.T).reshape(-1)[:count]


def rotate(kern):
    """The table with its phases rotated by one: row p takes row p + 1's place.  A table of one phase (24 -> 8 kHz) has no other
    phase to take, so it is delayed by one tap instead: the nearest wrong filter it has."""
    return np.roll(kern, 1, axis=0) if kern.shape[0] > 1 else np.roll(kern, 1, axis=1)


def resample(x, sr_in, sr_out, out_first=0, out_count=None, rotated=False):
    """float64 outputs out_first .. out_first + out_count - 1 (default: all ceil(new n / orig)) of the float32 wave x."""
    orig, new, w, kern = table(sr_in, sr_out)
    total = out_length(len(x), sr_in, sr_out)
    out_count = total - out_first if out_count is None else out_count
    y = _apply(np.asarray(x, dtype=np.float64), rotate(kern) if rotated else kern, orig, w, out_first + out_count)
    return y[out_first:]


def bound(x, sr_in, sr_out, out_count=None):
    """(K + 2) 2^-24 sum_j |k[p][j]| |x_j| for the first out_count outputs."""
    orig, new, w, kern = table(sr_in, sr_out)
    out_count = out_length(len(x), sr_in, sr_out) if out_count is None else out_count
    return (kern.shape[1] + 2) * U * _apply(np.abs(np.asarray(x, dtype=np.float64)), np.abs(kern), orig, w, out_count)


def noise(n, seed=0):
    """Seeded Gaussian noise x 0.3, clipped to +-1, float32."""
    return np.clip(0.3 * np.random.default_rng(1000 + seed).standard_normal(n), -1.0, 1.0).astype(np.float32)


def pcm_probe():
    """Values on which float2pcm's scale / saturate / truncate show: exactly +-1, half and one and a half steps either side of 0
    (truncation toward zero, no rounding), the largest float below 1, values beyond +-1, and steps around an integer."""
    s = 1.0 / 32768.0
    return np.array([1.0, -1.0, 0.5 * s, -0.5 * s, 1.5 * s, -1.5 * s, 0.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1.25, -1.25, 3.0e4,
                     -3.0e4, 0.999 * s, -0.999 * s, 100.0 * s, 100.9 * s, -100.9 * s, 32766.5 * s, 32767.5 * s, -32767.5 * s], dtype=np.float32)


def float2pcm_int16(sig):
    """The reference's float2pcm (Utility/utils.py:20-33) for int16, restated: times 32768, saturate, drop the fraction."""
    sig = np.asarray(sig, dtype=np.float32)
    return np.clip(sig * np.float32(32768.0), -32768, 32767).astype(np.int16)


def lengths(sr_in, sr_out, tile):
    """[(n, out_count)]: the input lengths the kernel tests use for one conversion and the outputs asked of each - all of them,
    except where a count of exactly tile - 1, tile or tile + 1 is no whole utterance's count (24 -> 48 kHz has even counts only):
    there the shortest utterance with at least that many outputs is asked for exactly that many."""
    orig, new, w, kern = table(sr_in, sr_out)
    K = kern.shape[1]
    full = lambda n: out_length(n, sr_in, sr_out)
    cases = [(n, full(n)) for n in (1, w, K - 1, 3 * orig + max(1, orig // 2))]  # the last: no multiple of orig (orig > 1)
    cases += [((c - 1) * orig // new + 1, c) for c in (tile - 1, tile, tile + 1)]
    n_long = -(-(2 * tile + 37) * orig // new) + 1
    cases.append((n_long, full(n_long)))
    return cases


@functools.lru_cache(maxsize=None)
def cases(sr_in, sr_out, tile):
    """The shared, read-only reference of one conversion: per length the wave, the float64 result, the per-output bound and the
    rotated-phase result."""
    out = []
    for c, (n, count) in enumerate(lengths(sr_in, sr_out, tile)):
        x = noise(n, seed=c)
        item = {"n": n, "count": count, "x": x, "ref": resample(x, sr_in, sr_out, 0, count), "bound": bound(x, sr_in, sr_out, count),
                "rotated": resample(x, sr_in, sr_out, 0, count, rotated=True)}
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(item)
    return tuple(out)
