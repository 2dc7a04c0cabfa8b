"""Float64 / numpy restatement of the per-phoneme prosody curves (include/toucan_prosody_curves.h), written
from the definition, not from the kernel:

* overrides and the pause factor as in tests/prosody_ref.py;
* durations: ed = S.duration * C[r][0] is ONE fp32 product by definition, and so is (float)d * ed before the round-half-even - this
  part is exact and is done in float32 here too;
* pitch, energy: avg = mean of the non-zero entries of the whole utterance; es = S.pitch * C[r][1], one fp32 product (it decides which
  rows are skipped, so it is part of the definition); rows with es != 1 become max(0, (v - avg) * es + avg) - in float64; rows with
  es == 1 are left alone;
* offsets: rows whose value after that is not 0 and whose offset is not 0 become max(0, v + o) - in float64.
"""
import numpy as np

from tests.prosody_ref import F_PHONEME, F_SILENCE, F_VOICED, F_WORD_BOUNDARY

NEUTRAL = np.array([1.0, 1.0, 1.0, 0.0, 0.0], dtype=np.float32)


def neutral(rows):
    return np.tile(NEUTRAL, (rows, 1))


def constant(lengths, rows_of_values):
    """The packed table that is constant over utterance u at rows_of_values[u] = (c_d, c_p, c_e) with offsets 0."""
    return np.concatenate([np.tile(np.float32(list(v) + [0.0, 0.0]), (n, 1)) for n, v in zip(lengths, rows_of_values)])


def scale_variance_curve(seq, scale, factors, offsets):
    seq = np.asarray(seq, dtype=np.float64)
    es = np.float32(scale) * np.asarray(factors, dtype=np.float32)  # (fp32 by definition)
    nz = seq[seq != 0.0]
    avg = nz.mean() if nz.size else np.float64("nan")
    with np.errstate(invalid="ignore"):
        scaled = (seq - avg) * es.astype(np.float64) + avg
        scaled = np.where(scaled < 0.0, 0.0, scaled)  # (NaN < 0 is false: NaN stays)
        out = np.where(es != 1.0, scaled, seq)
        o = np.asarray(offsets, dtype=np.float32).astype(np.float64)
        moved = out + o
        moved = np.where(moved < 0.0, 0.0, moved)
    return np.where((o != 0.0) & (out != 0.0), moved, out)


def control_one(text, pitch, energy, dur, scales, curves):
    """One utterance.  scales: (duration, pitch, energy, pause) or None for all 1; curves [L, 5] -> (pitch f64, energy f64, dur i64)."""
    text, curves = np.asarray(text), np.asarray(curves, dtype=np.float32)
    ds, ps, es, pause = (np.float32(1.0),) * 4 if scales is None else (np.float32(s) for s in scales)
    pitch = np.where(text[:, F_VOICED] == 0, 0.0, np.asarray(pitch, dtype=np.float64))
    energy = np.where(text[:, F_PHONEME] == 0, 0.0, np.asarray(energy, dtype=np.float64))
    dur = np.where(text[:, F_WORD_BOUNDARY] == 1, 0, np.asarray(dur, dtype=np.int64))
    if pause != 1.0:
        dur = np.where(text[:, F_SILENCE] == 1, np.rint(dur.astype(np.float32) * pause).astype(np.int64), dur)
    ed = ds * curves[:, 0]
    assert ed.dtype == np.float32
    dur = np.where(ed != 1.0, np.rint(dur.astype(np.float32) * ed).astype(np.int64), dur)
    return (scale_variance_curve(pitch, ps, curves[:, 1], curves[:, 3]), scale_variance_curve(energy, es, curves[:, 2], curves[:, 4]), dur)


def control(text, pitch, energy, dur, lengths, scales, curves):
    """A packed ragged batch (utterance u = rows sum(lengths[:u]) ...) with scales [B, 4] or None and the packed table [R, 5]."""
    outs, b0 = [], 0
    for u, n in enumerate(lengths):
        sl = slice(b0, b0 + n)
        outs.append(control_one(text[sl], pitch[sl], energy[sl], dur[sl], None if scales is None else scales[u], curves[sl]))
        b0 += n
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3))


def effective_scale(scales, curves, lengths, col):
    """Largest |S[col] * C[r][col]| per utterance (col 1: pitch, 2: energy)."""
    out, b0 = [], 0
    for u, n in enumerate(lengths):
        s = np.float32(1.0) if scales is None else np.float32(scales[u][col])
        out.append(float(np.abs(s * np.asarray(curves[b0:b0 + n, col], dtype=np.float32)).max()))
        b0 += n
    return out
