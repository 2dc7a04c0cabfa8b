"""Per-utterance prosody scales: host-side helpers shared by both sequencers and the interface (include/toucan_prosody.h).

The four knobs of the reference's inference call (InferenceToucanTTS.py:214-227) are scalars of a whole batch there.  Here each
accepts a scalar or one value per utterance; an all-scalar call keeps the scalar entries (and its bits), any sequence takes the
``_v`` entries, which also report the statistics of pitch / energy / durations before and after the scales.

Below the utterance, every phoneme can have its own: a curve table [R, 5] (``CURVE_COLUMNS``), given per utterance as an array or as
a list of ``Span``s - ``emphasis(feats, [k])`` stresses word k of ``word_spans(feats)`` - takes the ``_c`` entries, which also report
the statistics of every Span (include/toucan_prosody_curves.h)."""
import itertools
import math

import numpy as np

KNOBS = ("duration_scaling_factor", "pitch_variance_scale", "energy_variance_scale", "pause_duration_scaling_factor")  # column order of a scales table
STATS = ("n_pitch", "mean_pitch", "var_pitch", "n_energy", "mean_energy", "var_energy", "frames", "phones")  # columns of a statistics block


def _is_scalar(v):
    return np.ndim(v) == 0


def resolve_scales(batch, duration_scaling_factor=1.0, pitch_variance_scale=1.0, energy_variance_scale=1.0,
                   pause_duration_scaling_factor=1.0):
    """None when all four are scalars (the scalar entries serve the call), else the float32 [batch, 4] table of the ``_v`` entries with
    the scalars among them broadcast.  ValueError for a sequence whose length is not ``batch`` and for a duration factor that is
    not positive and finite (the message names the utterance)."""
    values = (duration_scaling_factor, pitch_variance_scale, energy_variance_scale, pause_duration_scaling_factor)
    if all(_is_scalar(v) for v in values):
        return None
    table = np.empty((batch, 4), dtype=np.float32)
    for col, (name, v) in enumerate(zip(KNOBS, values)):
        if _is_scalar(v):
            table[:, col] = float(v)
            continue
        v = np.asarray(v, dtype=np.float64)
        if v.ndim != 1 or v.shape[0] != batch:
            raise ValueError(f"{name}: a sequence must hold one value per utterance ({batch}), got shape {tuple(v.shape)}")
        table[:, col] = v
    for u, d in enumerate(table[:, 0]):
        if not (math.isfinite(d) and d > 0):
            raise ValueError(f"duration_scaling_factor of utterance {u} is {float(d)!r}: it must be positive and finite")
    return table


def broadcast_scales(batch, duration_scaling_factor=1.0, pitch_variance_scale=1.0, energy_variance_scale=1.0,
                     pause_duration_scaling_factor=1.0):
    """``resolve_scales`` for a call that takes the per-utterance kernels anyway (one with curves): the [batch, 4] table also when all
    four are scalars - None only when they are all exactly 1, which the kernels read as "no scales"."""
    table = resolve_scales(batch, duration_scaling_factor, pitch_variance_scale, energy_variance_scale, pause_duration_scaling_factor)
    if table is not None:
        return table
    values = [float(v) for v in (duration_scaling_factor, pitch_variance_scale, energy_variance_scale, pause_duration_scaling_factor)]
    if all(v == 1.0 for v in values):
        return None
    return resolve_scales(batch, [values[0]] * batch, *values[1:])


# ---- per-phoneme curves (include/toucan_prosody_curves.h) --------------------------------------------------
CURVE_COLUMNS = ("duration", "pitch", "energy", "pitch_offset", "energy_offset")  # columns of a curve table; neutral: 1, 1, 1, 0, 0
CURVE_NEUTRAL = (1.0, 1.0, 1.0, 0.0, 0.0)
F_PHONEME = 15  # articulatory feature "phoneme": 0 on silences, word boundaries and punctuation


class Span:
    """Phonemes [start, stop) of one utterance, 0 <= start <= stop <= L, with three factors on the utterance's duration / pitch
    variance / energy variance scales and two offsets added to the pitch and energy values behind them.

    ``pitch=`` / ``energy=`` scale the deviation from the mean of the WHOLE utterance (its non-zero entries), as the reference's
    _scale_variance does for a call: above 1 the span's contour moves away from the utterance's mean, below 1 towards it.  The
    reference's quirk is kept: a zero entry (an unvoiced phoneme, a pause) inside a span scaled below 1 becomes mean * (1 - scale).
    The offsets touch non-zero entries only and clamp at 0."""

    __slots__ = ("start", "stop") + CURVE_COLUMNS

    def __init__(self, start, stop, duration=1.0, pitch=1.0, energy=1.0, pitch_offset=0.0, energy_offset=0.0):
        self.start, self.stop = int(start), int(stop)
        self.duration, self.pitch, self.energy = float(duration), float(pitch), float(energy)
        self.pitch_offset, self.energy_offset = float(pitch_offset), float(energy_offset)

    def values(self):
        return tuple(getattr(self, c) for c in CURVE_COLUMNS)

    def __repr__(self):
        return "Span({}, {}, {})".format(self.start, self.stop, ", ".join(f"{c}={v!r}" for c, v in zip(CURVE_COLUMNS, self.values())))


def word_spans(feats):
    """(start, stop) of every word of an [L, 62] feature matrix: the maximal runs of rows whose phoneme feature (15) is 1.  Word
    boundaries, silences, the end-of-sentence symbol and punctuation all have it 0, so each of them ends a run."""
    flags = np.asarray(feats)[:, F_PHONEME] == 1
    edges = np.flatnonzero(np.diff(np.concatenate([[False], flags, [False]]).astype(np.int8)))
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def emphasis(feats, words, duration=1.2, pitch=1.3, energy=1.2, pitch_offset=0.0, energy_offset=0.0):
    """The ``Span``s that stress the words with the given indices (into ``word_spans(feats)``), every one with the same factors."""
    spans = word_spans(feats)
    out = []
    for w in words:
        if not 0 <= int(w) < len(spans):
            raise ValueError(f"word {w}: the text has {len(spans)} words")
        out.append(Span(*spans[int(w)], duration=duration, pitch=pitch, energy=energy, pitch_offset=pitch_offset, energy_offset=energy_offset))
    return out


def _bad_curve_value(u, i, col, value):
    need = "positive and finite" if col == 0 else "finite"
    return ValueError(f"prosody curve of utterance {u}, phoneme {i}: {CURVE_COLUMNS[col]} is {float(value)!r}, it must be {need}")


def resolve_curves(lengths, curves):
    """``curves``: per utterance None, an [L_u, 5] array (columns ``CURVE_COLUMNS``) or a list of ``Span``s.  None when every entry
    is None (the call takes the path without curves), else ``(table, ranges, counts)``: the packed float32 [R, 5] table, the packed
    int32 [n, 2] row ranges of all Spans in utterance and list order, and the number of Spans per utterance.  Overlapping Spans
    multiply their three factors and add their two offsets, in list order, in float32.  ValueError for a wrong number of entries, a
    wrong shape, a Span outside its utterance, a duration factor that is not positive and finite and any other value that is not
    finite (the message names the utterance and the phoneme), and for more Spans than the batch has phonemes."""
    lengths = [int(n) for n in lengths]
    if curves is None:
        return None
    if len(curves) != len(lengths):
        raise ValueError(f"prosody_curves must hold one entry per utterance ({len(lengths)}), got {len(curves)}")
    if all(c is None for c in curves):
        return None
    begins = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    table = np.empty((int(begins[-1]), len(CURVE_COLUMNS)), dtype=np.float32)  # (one packed table: this runs once per call, on its host path)
    table[:] = CURVE_NEUTRAL
    ranges, counts = [], []
    with np.errstate(over="ignore", invalid="ignore"):  # (an overflow is a value that is not finite: the check below names it)
        for u, (n, c) in enumerate(zip(lengths, curves)):
            b0 = int(begins[u])
            count = 0
            if c is None:
                pass
            elif isinstance(c, (list, tuple)) and all(isinstance(s, Span) for s in c):
                for k, s in enumerate(c):
                    if not 0 <= s.start <= s.stop <= n:
                        raise ValueError(f"prosody curve of utterance {u}: span {k} is phonemes [{s.start}, {s.stop}), the utterance has {n}")
                    v = s.values()
                    for col, x in enumerate(v):  # (here and not only on the table: an empty Span's values are checked too)
                        if not math.isfinite(x) or (col == 0 and not x > 0):
                            raise _bad_curve_value(u, s.start, col, x)
                    v = np.float32(v)
                    table[b0 + s.start:b0 + s.stop, :3] *= v[:3]
                    table[b0 + s.start:b0 + s.stop, 3:] += v[3:]
                    ranges.append((b0 + s.start, b0 + s.stop))
                count = len(c)
            else:
                c = c.detach().cpu().numpy() if hasattr(c, "detach") else np.asarray(c)
                if c.shape != (n, len(CURVE_COLUMNS)):
                    raise ValueError(f"prosody curve of utterance {u}: an array must be [{n}, {len(CURVE_COLUMNS)}], got {tuple(c.shape)}")
                table[b0:b0 + n] = c
            counts.append(count)
    bad = ~np.isfinite(table)
    bad[:, 0] |= ~(table[:, 0] > 0)
    if bad.any():
        r, col = (int(x) for x in np.argwhere(bad)[0])
        u = int(np.searchsorted(begins, r, side="right")) - 1
        raise _bad_curve_value(u, r - int(begins[u]), col, table[r, col])
    if len(ranges) > table.shape[0]:
        raise ValueError(f"prosody_curves hold {len(ranges)} spans, a batch of {table.shape[0]} phonemes takes at most {table.shape[0]}")
    return table, np.asarray(ranges, dtype=np.int32).reshape(-1, 2), counts


def split_span_stats(span_stats, counts):
    """The packed (before [n, 8], after [n, 8]) span blocks of a batch -> per utterance (before [n_u, 8], after [n_u, 8])."""
    before, after = span_stats
    out, k = [], 0
    for n in counts:
        out.append((before[k:k + n], after[k:k + n]))
        k += n
    return out


def grid(duration_scaling_factors=(1.0,), pitch_variance_scales=(1.0,), energy_variance_scales=(1.0,),
         pause_duration_scaling_factors=(1.0,)):
    """The Cartesian product of the four tuples as (duration, pitch, energy, pause) tuples, row-major in that order (the last
    varies fastest)."""
    axes = [tuple(float(x) for x in a) for a in (duration_scaling_factors, pitch_variance_scales, energy_variance_scales,
                                                 pause_duration_scaling_factors)]
    if any(len(a) == 0 for a in axes):
        raise ValueError("every axis of a prosody grid needs at least one value")
    return list(itertools.product(*axes))
