"""The spectral distances of include/toucan_fidelity.h restated in numpy: float64 with numpy.fft (the reference every test measures
against), and the same definition in float32 - the DFT as a matrix product, the tail - whose distance from the float64 one is what
float32 arithmetic costs on a case and therefore what the tolerances of tests/test_gpu_fidelity.py are derived from.  Nothing here
imports the package's kernels; the filterbank is style.mel_filterbank, the one piece both sides share by definition."""
import numpy as np

from ims_toucan_prosody_variance_amd import style

SR, N_REF, HOP_REF, N_MELS, FMIN, FMAX = 24000, 1536, 384, 100, 80.0, 12000.0
RESOLUTIONS = ((768, 192), (1536, 384), (3072, 768))
FLOOR = 1e-10
SUMS = ("mel", "diff_sq", "ref_sq", "log_mag")


def mel_matrix():
    """float32 [100, 769], as the kernels get it."""
    return style.mel_filterbank(SR, N_REF, N_MELS, FMIN, FMAX)


def n_frames(n, hop):
    return 1 + n // hop


def padded(x, n_fft):
    x = np.asarray(x).reshape(-1)
    if x.size <= n_fft // 2:
        raise ValueError(f"{x.size} samples: the centred STFT with reflection padding needs more than {n_fft // 2}")
    return np.pad(x, n_fft // 2, mode="reflect")


def row_buffer(x, hop):
    """The padded signal in whole rows of ``hop`` samples, the tail of the last row zero: float32 [rows, hop]."""
    p = padded(np.asarray(x, dtype=np.float32), 4 * hop)
    rows = -(-p.size // hop)
    buf = np.zeros(rows * hop, dtype=np.float32)
    buf[:p.size] = p
    return buf.reshape(rows, hop)


def frames(x, n_fft, dtype=np.float64):
    hop = n_fft // 4
    p = padded(np.asarray(x, dtype=dtype), n_fft)
    F = n_frames(p.size - n_fft, hop)
    return np.stack([p[f * hop: f * hop + n_fft] for f in range(F)])


def window(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)  # periodic Hann


def spectrum(x, n_fft):
    """float64 (re, im) [F, N / 2 + 1] by numpy.fft."""
    z = np.fft.rfft(frames(x, n_fft) * window(n_fft), axis=1)
    return z.real, z.imag


def basis(n_fft):
    """float64 [N, 2 (N / 2 + 1)]: columns [w cos | -w sin]."""
    n = np.arange(n_fft, dtype=np.float64)
    ang = 2.0 * np.pi * np.outer(n, np.arange(n_fft // 2 + 1, dtype=np.float64)) / n_fft
    w = window(n_fft)[:, None]
    return np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1)


def spectrum_f32(x, n_fft):
    """float32 (re, im): the frames times the float32 basis, numpy's own summation order."""
    nb = n_fft // 2 + 1
    z = frames(x, n_fft, np.float32) @ basis(n_fft).astype(np.float32)
    assert z.dtype == np.float32
    return z[:, :nb], z[:, nb:]


def amplitude(re, im):
    """In the dtype of its arguments."""
    dt = re.dtype.type
    return np.sqrt(np.maximum(re * re + im * im, dt(FLOOR)))


def frame_sums(spec_a, spec_b, mel=None, dtype=np.float64):
    """The tail: (re, im) of both signals [F, bins] -> [F, 4] (``SUMS``) with every operation in ``dtype``; float64 is the definition,
    float32 the stand-in whose error sets the tolerances.  mel: [n_mels, bins] or None (column 0 stays 0)."""
    dt = np.dtype(dtype).type
    a = amplitude(np.asarray(spec_a[0], dtype=dtype), np.asarray(spec_a[1], dtype=dtype))
    b = amplitude(np.asarray(spec_b[0], dtype=dtype), np.asarray(spec_b[1], dtype=dtype))
    out = np.zeros((a.shape[0], 4), dtype=dtype)
    if mel is not None:
        M = np.asarray(mel, dtype=dtype).T
        la = np.log10(np.maximum(a @ M, dt(FLOOR)))
        lb = np.log10(np.maximum(b @ M, dt(FLOOR)))
        out[:, 0] = np.abs(la - lb).sum(axis=1, dtype=dtype)
    out[:, 1] = ((a - b) ** 2).sum(axis=1, dtype=dtype)
    out[:, 2] = (b * b).sum(axis=1, dtype=dtype)
    out[:, 3] = np.abs(np.log(a) - np.log(b)).sum(axis=1, dtype=dtype)
    return out


def measures(sums, bins, n_mels=N_MELS):
    """[F, 4] frame sums -> dict: mel_l1, frame_mel_l1 [F], spectral_convergence, log_magnitude_l1 (float64 from here on)."""
    s = np.asarray(sums, dtype=np.float64)
    F = s.shape[0]
    tot = s.sum(axis=0)
    return {"mel_l1": tot[0] / (F * n_mels), "frame_mel_l1": s[:, 0] / n_mels, "spectral_convergence": np.sqrt(tot[1]) / np.sqrt(tot[2]),
            "log_magnitude_l1": tot[3] / (F * bins)}


def distance(a, b, resolutions=RESOLUTIONS, f32=False):
    """The whole definition for one pair: {"mel_l1", "frame_mel_l1", "lengths", (N, hop): {...}}; f32: the float32 stand-in."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    n = min(a.size, b.size)
    out = {"lengths": (a.size, b.size)}
    for n_fft, hop in resolutions:
        assert n_fft == 4 * hop
        ref = (n_fft, hop) == (N_REF, HOP_REF)
        spec = spectrum_f32 if f32 else spectrum
        m = measures(frame_sums(spec(a[:n], n_fft), spec(b[:n], n_fft), mel_matrix() if ref else None, np.float32 if f32 else np.float64),
                     n_fft // 2 + 1)
        out[(n_fft, hop)] = {k: m[k] for k in ("spectral_convergence", "log_magnitude_l1")}
        if ref:
            out["mel_l1"], out["frame_mel_l1"] = m["mel_l1"], m["frame_mel_l1"]
    return out


def log_mel(x):
    """The reference's MelSpectrogram.forward of one signal in float64: [F, 100]."""
    re, im = spectrum(x, N_REF)
    return np.log10(np.maximum(amplitude(re, im) @ mel_matrix().astype(np.float64).T, FLOOR))


# ---- the seeded cases of the golden fixture (tests/golden/fidelity/mel_loss.npz stores the seeds, not the waves) ------------------
GOLDEN_LENGTHS = (769, 1152, 5000, 12288)
GOLDEN_KINDS = ("half", "noisy")


def golden_wave(n, seed):
    """0.1 N(0, 1) from fixture_weights.uniform01 by Box-Muller: float32 [n]."""
    from ims_toucan_prosody_variance_amd import fixture_weights as fw
    u1 = fw.uniform01("fidelity.golden", n, seed, 0)
    u2 = fw.uniform01("fidelity.golden", n, seed, 1)
    z = np.sqrt(-2.0 * np.log(np.maximum(u1, 1e-12))) * np.cos(2.0 * np.pi * u2)
    return (0.1 * z).astype(np.float32)


def golden_pair(n, kind, seed):
    """(generated, recording): the recording is the seeded noise; "half": generated = half of it; "noisy": plus 1 % of other noise."""
    b = golden_wave(n, seed)
    if kind == "half":
        return (0.5 * b).astype(np.float32), b
    assert kind == "noisy"
    return (b + np.float32(0.01) * golden_wave(n, seed + 1000)).astype(np.float32), b


def golden_cases():
    return [(n, kind, 100 + 10 * i + j) for i, n in enumerate(GOLDEN_LENGTHS) for j, kind in enumerate(GOLDEN_KINDS)]
