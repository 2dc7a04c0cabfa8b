"""The numpy restatement of include/toucan_intelligibility.h (STOI: Taal, Hendriks, Heusdens, Jensen, IEEE TASL 19(7), 2011; ESTOI:
Jensen and Taal, IEEE/ACM TASLP 24(11), 2016), written from the two publications; its parity with any toolkit is not pinned.
Every function takes a ``dtype``: float64 is the definition, float32 the stand-in whose error sets the end-to-end tolerances,
numpy.longdouble the arbiter that sets the tolerance of the tail.  The silent-frame mask is discrete and is always taken in at least
float64.  Also the seeded generators of the tests."""
import numpy as np

FS = 10000
N_FRAME, HOP, N_FFT, N_BINS = 256, 128, 512, 257
N_BANDS, SEG = 15, 30
DYN_RANGE_DB = 40.0
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)  # y' <= (1 + 10^(-beta / 20)) x, beta = -15 dB
EPS = float(np.finfo(np.float64).eps)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
         (138, 174), (174, 219))


def band_table():
    """The formula: centres 150 2^(j / 3) Hz, edges 2^(-+1/6) of them, each mapped to the nearest of the 257 bin frequencies."""
    f = np.arange(N_BINS, dtype=np.float64) * FS / N_FFT
    out = []
    for j in range(N_BANDS):
        cf = 150.0 * 2.0 ** (j / 3.0)
        lo, hi = cf * 2.0 ** (-1.0 / 6.0), cf * 2.0 ** (1.0 / 6.0)
        out.append((int(np.argmin(np.abs(f - lo))), int(np.argmin(np.abs(f - hi)))))
    return tuple(out)


def window(dtype=np.float64):
    """The 258-point Hann window without its zero end points, computed in float64 and rounded once."""
    i = np.arange(N_FRAME, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * (i + 1.0) / (N_FRAME + 1.0)))).astype(dtype)


def n_frames(n):
    return (int(n) - N_FRAME) // HOP + 1 if n >= N_FRAME else 0


def windowed_frames(x, dtype=np.float64):
    """[F, 256]: w x_f, the product in ``dtype``."""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    F = n_frames(x.size)
    if F == 0:
        return np.zeros((0, N_FRAME), dtype=dtype)
    return np.stack([x[f * HOP: f * HOP + N_FRAME] for f in range(F)]) * window(dtype)


def frame_energies(x, dtype=np.float64):
    """e[f] = 20 log10(|| w x_f || + eps) of the recording, in at least float64."""
    dt = np.result_type(dtype, np.float64)
    fr = windowed_frames(x, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        return 20.0 * np.log10(np.sqrt((fr * fr).sum(axis=1)) + dt.type(EPS))


def kept_frames(x, dtype=np.float64):
    """The indices of the frames of the recording that are kept, ascending."""
    e = frame_energies(x, dtype)
    if e.size == 0:
        return np.zeros(0, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(e > e.max() - DYN_RANGE_DB).astype(np.int64)  # a NaN or Inf energy: max is NaN or Inf, nothing is kept


def threshold_margin(x):
    """The smallest distance in dB of a frame energy from the 40 dB threshold (float64)."""
    e = frame_energies(x)
    return float(np.abs(e - (e.max() - DYN_RANGE_DB)).min()) if e.size else float("inf")


def compacted(x, kept, dtype=np.float64):
    """The materialised overlap-add of the windowed kept frames at hop 128: [128 (K - 1) + 256], frames added in ascending order."""
    fr = windowed_frames(x, dtype)[kept]
    K = len(kept)
    out = np.zeros(HOP * (K - 1) + N_FRAME if K else 0, dtype=dtype)
    for q in range(K):
        out[q * HOP: q * HOP + N_FRAME] += fr[q]
    return out


def gathered_rows(x, kept, dtype=np.float64):
    """[K, 256]: the windowed frames of the compacted signal from the source and the kept list alone.  Compacted sample 128 q + r
    (r < 128) is (0 + w[r + 128] x[128 kept[q - 1] + r + 128]) + w[r] x[128 kept[q] + r], a term that does not exist counting as 0;
    row m is w times the compacted samples 128 m .. 128 m + 255.  Every operation in ``dtype``, in this order."""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    w = window(dtype)
    kept = np.asarray(kept, dtype=np.int64)
    K = len(kept)
    if K == 0:
        return np.zeros((0, N_FRAME), dtype=dtype)
    r = np.arange(HOP)
    first = x[kept[:, None] * HOP + r[None, :]] * w[None, :HOP]           # [K, 128]: the first half of kept frame q
    second = x[kept[:, None] * HOP + HOP + r[None, :]] * w[None, HOP:]    # [K, 128]: its second half
    zero = np.zeros((1, HOP), dtype=dtype)
    prev = np.concatenate([zero, second])                                 # [K + 1, 128]: block q gets the second half of frame q - 1
    cur = np.concatenate([first, zero])                                   # and the first half of frame q
    blocks = (zero + prev) + cur                                          # compacted samples 128 q .. 128 q + 127, q = 0 .. K
    rows = np.concatenate([blocks[:-1], blocks[1:]], axis=1)              # row m = blocks m and m + 1
    return rows * w[None, :]


def basis(dtype=np.float64):
    """[256, 514]: columns [cos | -sin] of the 512-point DFT for the 256 samples that are not padding."""
    dt = np.dtype(dtype).type
    two_pi = dt(8.0) * np.arctan(dt(1.0))
    ang = two_pi * np.outer(np.arange(N_FRAME), np.arange(N_BINS)).astype(dtype) / dt(N_FFT)
    return np.concatenate([np.cos(ang), -np.sin(ang)], axis=1).astype(dtype)


def basis_f32():
    """The float32 basis the kernels are given: computed in float64, rounded once."""
    return basis(np.float64).astype(np.float32)


def band_values(rows, dtype=np.float64):
    """rows [M, 256] (windowed) -> [M, 15]: sqrt of the sum of |X(k)|^2 over a band's bins; the DFT is a matrix product in ``dtype``
    (float32: on the float32 basis, numpy's own summation order)."""
    rows = np.asarray(rows, dtype=dtype)
    b = basis_f32() if np.dtype(dtype) == np.float32 else basis(dtype)
    z = rows @ b
    p = z[:, :N_BINS] ** 2 + z[:, N_BINS:] ** 2
    return np.sqrt(np.stack([p[:, lo:hi].sum(axis=1) for lo, hi in BANDS], axis=1))


def _unit(m, axis, eps):
    m = m - m.mean(axis=axis, keepdims=True)
    return m / (np.sqrt((m * m).sum(axis=axis, keepdims=True)) + eps)


def tail(X, Y, dtype=np.float64):
    """Band values [M, 15] of the recording and of the generated signal -> (segment STOI [S], segment ESTOI [S], STOI, ESTOI) in
    ``dtype``: the segment STOI is the mean of d over the 15 bands, STOI the mean of that over the segments.  No segments: NaN."""
    dt = np.dtype(dtype).type
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    S = X.shape[0] - SEG + 1
    if S <= 0:
        return np.zeros(0, dtype=dtype), np.zeros(0, dtype=dtype), dt(np.nan), dt(np.nan)
    eps, clip = dt(EPS), dt(CLIP)
    idx = np.arange(S)[:, None] + np.arange(SEG)[None, :]
    xs, ys = X[idx].transpose(0, 2, 1), Y[idx].transpose(0, 2, 1)  # [S, 15, 30]
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = np.sqrt((xs * xs).sum(axis=2)) / (np.sqrt((ys * ys).sum(axis=2)) + eps)
        yp = np.minimum(alpha[:, :, None] * ys, clip * xs)
        xm, ym = xs - xs.mean(axis=2, keepdims=True), yp - yp.mean(axis=2, keepdims=True)
        d = (xm * ym).sum(axis=2) / (np.sqrt((xm * xm).sum(axis=2)) * np.sqrt((ym * ym).sum(axis=2)) + eps)
        seg_stoi = d.sum(axis=1) / dt(N_BANDS)
        xn, yn = _unit(_unit(xs, 2, eps), 1, eps), _unit(_unit(ys, 2, eps), 1, eps)
        seg_estoi = (xn * yn).sum(axis=1).sum(axis=1) / dt(SEG)
        return seg_stoi, seg_estoi, seg_stoi.sum() / dt(S), seg_estoi.sum() / dt(S)


def score(x, y, dtype=np.float64):
    """x: the recording, y: the generated signal, both at 10 kHz -> dict: stoi, estoi, status, frames, kept_frames, segments, kept
    (the indices), segment_stoi, segment_estoi, lengths."""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    n = min(x.size, y.size)
    out = {"lengths": (x.size, y.size), "frames": n_frames(n)}
    x, y = x[:n], y[:n]
    kept = kept_frames(x, dtype)
    K = len(kept)
    M = K if K >= SEG else 0
    X, Y = (band_values(gathered_rows(s, kept[:M], dtype), dtype) for s in (x, y))
    ss, se, stoi, estoi = tail(X, Y, dtype)
    out.update(stoi=float(stoi), estoi=float(estoi), status="ok" if M else "too_short", kept_frames=K, segments=max(0, M - SEG + 1), kept=kept,
               segment_stoi=ss, segment_estoi=se, bands=(X, Y))
    return out


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def speech_like(n, seed, amplitude=0.1):
    """Lightly coloured noise under a slow envelope of its own - three sinusoids of seeded frequency (1.5 to 8 Hz) and phase, between
    0.3 and 1, so every frame is within some 11 dB of the loudest -, float32."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n + 1)
    col = z[1:] + 0.5 * z[:-1]
    t = np.arange(n) / FS
    m = sum(np.sin(2.0 * np.pi * rng.uniform(1.5, 8.0) * t + rng.uniform(0.0, 2.0 * np.pi)) for _ in range(3)) / 3.0
    return (amplitude * (0.65 + 0.35 * m) * col / 1.118).astype(np.float32)


def white(n, seed, rms):
    return (rms * np.random.default_rng([seed, 777]).standard_normal(n)).astype(np.float32)  # (a stream speech_like never draws from)


def at_snr(x, snr_db, seed):
    """x plus white noise at the given signal-to-noise ratio, float32."""
    rms = float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))
    return (x + white(len(x), seed, rms * 10.0 ** (-snr_db / 20.0))).astype(np.float32)


def with_gap(x, first_block, blocks):
    """x with 128 ``blocks`` exact zeros from sample 128 ``first_block`` on."""
    y = np.array(x, dtype=np.float32)
    y[HOP * first_block: HOP * (first_block + blocks)] = 0.0
    return y
