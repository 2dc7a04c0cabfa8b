"""The seeded ragged batch of tests/test_gpu_prominence.py and its float64 restatement, built once per process and shared (read-only):
T = 1, 2, 7, 255, 256, 257, 1000 and 4097 frames - less than a tile of 256, a tile exactly, a tile and one frame, several tiles,
halos wider than the signal -, tracks with voiceless stretches, one all-unvoiced utterance (T = 1000), and in the longest one an
empty unit and units that cross tile edges.  tests/test_prominence_cpu.py holds every decision of these cases to its margin."""
import functools

import numpy as np

from tests import prominence_ref as pr

FRAMES = (1, 2, 7, 255, 256, 257, 1000, 4097)
UNVOICED = 6  # the utterance without a voiced frame


def _smooth(rng, T, width):
    """Seeded noise smoothed over `width` frames, unit scale."""
    x = rng.standard_normal(T + 2 * width)
    k = np.hanning(2 * width + 1)
    y = np.convolve(x, k / np.sqrt((k * k).sum()), "valid")
    return y[:T]


def utterance(u, T):
    """-> (f0 float32 [T], energy float32 [T], phonemes int32 [L, 3], units int32 [n, 2])."""
    rng = np.random.default_rng(5000 + u)
    f0 = 120.0 * np.exp(0.2 * _smooth(rng, T, 6) + 0.01 * rng.standard_normal(T))
    e = np.exp(0.8 * _smooth(rng, T, 4) + 0.02 * rng.standard_normal(T))
    phones, t = [], 0
    while t < T:
        n = int(min(rng.integers(1, 13), T - t))
        phones.append((t, t + n, int(rng.random() < 0.8)))
        if rng.random() < 0.35:  # a voiceless phoneme
            f0[t:t + n] = 0.0
        if rng.random() < 0.1:  # an empty phoneme between two others
            phones.append((t + n, t + n, 1))
        t += n
    if u == UNVOICED:
        f0[:] = 0.0
    elif T > 2:
        f0[T // 2] = 110.0  # at least one voiced frame
    # units: runs of two to four phonemes, the phoneme behind each left out
    units, k = [], 0
    while k < len(phones):
        m = int(rng.integers(2, 5))
        b, e_ = phones[k][0], phones[min(k + m, len(phones)) - 1][1]
        if e_ > b:
            units.append((b, e_))
        k += m + 1
    if T == 4097:
        units = [r for r in units if r[1] <= 240 or r[0] >= 1290]
        units += [(250, 262), (262, 262), (500, 1030), (1280, 1281)]  # across a tile edge, empty, across two edges, one frame
        units.sort()
    if T == 2:
        units = [(0, 1), (1, 2)]
    if T == 1:
        units = [(0, 0), (0, 1), (1, 1)]
    return f0.astype(np.float32), e.astype(np.float32), np.asarray(phones, dtype=np.int32).reshape(-1, 3), np.asarray(units, dtype=np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def batch():
    """-> list of (f0, energy, phonemes, units), one per entry of FRAMES."""
    return [utterance(u, T) for u, T in enumerate(FRAMES)]


@functools.lru_cache(maxsize=None)
def restated():
    """The restatement of every utterance of ``batch()`` at the default weights and band."""
    return [pr.measure_tracks(*case) for case in batch()]
