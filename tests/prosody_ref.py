"""Float64 / numpy restatement of the per-utterance prosody control and its statistics (include/toucan_prosody.h, DESIGN.md
section 14).  Written from the definition (InferenceToucanTTS.py:214-227, _scale_variance :333-343), not from the kernels:

* overrides: pitch 0 where the phoneme is unvoiced, energy 0 off phonemes, duration 0 at word boundaries;
* durations: round-half-even of the fp32 product with the pause factor (silences) and then the duration factor - the product is an
  fp32 product by definition (``dur.float() * scale``), so this part is exact and is done in float32 here too;
* _scale_variance: mean over the non-zero entries, EVERY entry shifted, scaled, shifted back, negatives clamped to 0; skipped when
  the scale is exactly 1 - here in float64;
* statistics: count, mean and population variance of the non-zero entries (0 when there is none), sum of durations, rows.
"""
import numpy as np

F_PHONEME, F_SILENCE, F_WORD_BOUNDARY, F_VOICED = 15, 16, 21, 61  # articulatory_features.py:817-901


def scale_variance(seq, scale):
    seq = np.asarray(seq, dtype=np.float64)
    if scale == 1.0:
        return seq.copy()
    nz = seq[seq != 0.0]
    avg = nz.mean() if nz.size else np.float64("nan")  # (torch's mean of an empty selection)
    out = (seq - avg) * np.float64(scale) + avg
    return np.where(out < 0.0, 0.0, out)  # (NaN < 0 is false: NaN stays)


def control_one(text, pitch, energy, dur, scales=None):
    """One utterance.  scales: (duration, pitch, energy, pause) or None for the overrides alone -> (pitch f64, energy f64, dur i64)."""
    text = np.asarray(text)
    pitch = np.where(text[:, F_VOICED] == 0, 0.0, np.asarray(pitch, dtype=np.float64))
    energy = np.where(text[:, F_PHONEME] == 0, 0.0, np.asarray(energy, dtype=np.float64))
    dur = np.where(text[:, F_WORD_BOUNDARY] == 1, 0, np.asarray(dur, dtype=np.int64))
    if scales is None:
        return pitch, energy, dur
    ds, ps, es, pause = (np.float32(s) for s in scales)
    if pause != 1.0:
        dur = np.where(text[:, F_SILENCE] == 1, np.rint(dur.astype(np.float32) * pause).astype(np.int64), dur)
    if ds != 1.0:
        dur = np.rint(dur.astype(np.float32) * ds).astype(np.int64)
    return scale_variance(pitch, ps), scale_variance(energy, es), dur


def control(text, pitch, energy, dur, lengths, scales=None):
    """A packed ragged batch (utterance u = rows sum(lengths[:u]) ...) with scales [B, 4] (None: overrides alone)."""
    outs, b0 = [], 0
    for u, n in enumerate(lengths):
        sl = slice(b0, b0 + n)
        outs.append(control_one(text[sl], pitch[sl], energy[sl], dur[sl], None if scales is None else scales[u]))
        b0 += n
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3))


def stats_one(pitch, energy, dur):
    row = np.zeros(8, dtype=np.float64)
    for k, seq in enumerate((pitch, energy)):
        seq = np.asarray(seq, dtype=np.float64)
        nz = seq[seq != 0.0]
        row[3 * k] = nz.size
        if nz.size:
            row[3 * k + 1] = nz.mean()
            row[3 * k + 2] = ((nz - nz.mean()) ** 2).mean()
    row[6] = np.asarray(dur, dtype=np.int64).sum()
    row[7] = len(dur)
    return row


def stats(pitch, energy, dur, lengths):
    """[B, 8] float64: n_pitch, mean_pitch, var_pitch, n_energy, mean_energy, var_energy, frames, phones."""
    rows, b0 = [], 0
    for n in lengths:
        rows.append(stats_one(pitch[b0:b0 + n], energy[b0:b0 + n], dur[b0:b0 + n]))
        b0 += n
    return np.stack(rows)


def assert_stats_match(got, want):
    """The kernel's block against this file's: counts, frames and phones exact; means and variances within 1e-6 relative + 1e-12
    absolute (the kernel accumulates in fp64 and rounds to fp32 once - half an fp32 ulp, 6e-8 - and the bound leaves a few ulps for
    the cast of this reference); a NaN (an utterance whose scaled pitch is NaN) must be a NaN on both sides."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    for col in (0, 3, 6, 7):
        assert np.array_equal(got[:, col], want[:, col]), (col, got[:, col], want[:, col])
    for col in (1, 2, 4, 5):
        g, w = got[:, col], want[:, col]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (col, g, w)
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= 1e-6 * np.abs(w[ok]) + 1e-12), (col, g, w)
