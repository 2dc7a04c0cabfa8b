"""Per-utterance prosody scales: host-side helpers shared by both sequencers and the interface (include/toucan_prosody.h).

The four knobs of the reference's inference call (InferenceToucanTTS.py:214-227) are scalars of a whole batch there.  Here each
accepts a scalar or one value per utterance; an all-scalar call keeps the scalar entries (and its bits), any sequence takes the
``_v`` entries, which also report the statistics of pitch / energy / durations before and after the scales."""
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


def grid(duration_scaling_factors=(1.0,), pitch_variance_scales=(1.0,), energy_variance_scales=(1.0,),
         pause_duration_scaling_factors=(1.0,)):
    """The Cartesian product of the four tuples as (duration, pitch, energy, pause) tuples, row-major in that order (the last
    varies fastest)."""
    axes = [tuple(float(x) for x in a) for a in (duration_scaling_factors, pitch_variance_scales, energy_variance_scales,
                                                 pause_duration_scaling_factors)]
    if any(len(a) == 0 for a in axes):
        raise ValueError("every axis of a prosody grid needs at least one value")
    return list(itertools.product(*axes))
