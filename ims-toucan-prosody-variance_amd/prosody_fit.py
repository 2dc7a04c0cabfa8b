"""Time budgets: host-side helpers shared by both sequencers and the interface (include/toucan_prosody_fit.h).

The scales and curves of prosody.py are relative.  A ``Fit`` is absolute: "this utterance in exactly N frames" (``knob="duration"``:
the utterance's duration scale is solved for), "... and keep the speech tempo" (``knob="pause"``: its pause scale absorbs the slot),
or "phonemes [start, stop) in exactly N frames" (a multiplier on column 0 of their curve rows).  The solve runs on the device between
the predictors and the control kernel of the same pass; ``exact=True`` hands out the frames no scale reaches, ``exact=False`` takes
the nearest scale.  Everything else of the call - the other scales, ``prosody_curves=``, gold ``durations=`` - stays as given."""
import math

import numpy as np

FRAMES_PER_SECOND = 62.5  # one mel frame is 384 samples at 24 kHz
UTT_DURATION, UTT_PAUSE, SPAN = 0, 1, 2  # segment kinds
SEGMENT_COLUMNS = ("utterance", "kind", "begin", "end", "target", "lo", "hi", "exact")  # a row of the segment table (begin, end: packed rows)
FIT_COLUMNS = ("target", "frames", "frames_scaled", "value", "status", "iterations", "extra_rows", "base_frames")  # a row of the report
STATUS = ("EMPTY", "EXACT", "REPAIRED", "NEAREST", "CLAMPED_LOW", "CLAMPED_HIGH")  # report column 4 indexes this
DEFAULT_BOUNDS = {UTT_DURATION: (0.25, 4.0), UTT_PAUSE: (0.0, 8.0), SPAN: (0.25, 4.0)}
MAX_TARGET, MAX_BOUND = 1 << 24, 64.0


class Fit:
    """A target for one utterance (``start`` and ``stop`` both None) or for its phonemes [start, stop) (``knob="duration"`` only):
    ``target_frames`` mel frames, or ``target_seconds`` (rounded to floor(seconds * 62.5 + 0.5) frames).  ``bounds`` = (lo, hi) of the
    knob; the defaults are 0.25 .. 4 for durations and 0 .. 8 for pauses.  ``resolve_fits`` checks the values."""

    __slots__ = ("target_frames", "target_seconds", "knob", "exact", "bounds", "start", "stop")

    def __init__(self, target_frames=None, target_seconds=None, knob="duration", exact=True, bounds=None, start=None, stop=None):
        self.target_frames, self.target_seconds, self.knob, self.exact = target_frames, target_seconds, knob, bool(exact)
        self.bounds, self.start, self.stop = bounds, start, stop

    def whole(self):
        return self.start is None and self.stop is None

    def __repr__(self):
        return "Fit({})".format(", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__ if getattr(self, k) is not None))


def _frames(fit, where):
    if (fit.target_frames is None) == (fit.target_seconds is None):
        raise ValueError(f"{where}: give one of target_frames and target_seconds")
    if fit.target_seconds is not None:
        sec = float(fit.target_seconds)
        if not math.isfinite(sec):
            raise ValueError(f"{where}: target_seconds is {sec!r}")
        t = math.floor(sec * FRAMES_PER_SECOND + 0.5)
    else:
        t = fit.target_frames
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
            if not (isinstance(t, (float, np.floating)) and float(t).is_integer()):
                raise ValueError(f"{where}: target_frames is {t!r}, not a whole number of frames")
        t = int(t)
    if not 1 <= t <= MAX_TARGET:
        raise ValueError(f"{where}: the target of {t} frames is outside 1 .. 2^24")
    return t


def _bounds(fit, kind, where):
    b = DEFAULT_BOUNDS[kind] if fit.bounds is None else fit.bounds
    try:
        lo, hi = (float(np.float32(v)) for v in b)
    except (TypeError, ValueError):
        raise ValueError(f"{where}: bounds must be (lo, hi), got {b!r}") from None
    positive = lo >= 0 if kind == UTT_PAUSE else lo > 0
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi and positive and hi <= MAX_BOUND):
        need = "0 <= lo" if kind == UTT_PAUSE else "0 < lo"
        raise ValueError(f"{where}: bounds ({lo!r}, {hi!r}) must be finite with {need} <= hi <= {int(MAX_BOUND)}")
    return lo, hi


def resolve_fits(lengths, fits):
    """``fits``: per utterance None, a ``Fit`` or a list of span ``Fit``s.  None when every entry is None (the call takes the path
    without a fit), else the packed float32 [n_seg, 8] segment table (columns ``SEGMENT_COLUMNS``) in utterance and list order.
    ValueError, naming the utterance and the segment, for a wrong number of entries, both or neither target, a target that is no
    whole number of frames in 1 .. 2^24, bad bounds, an unknown knob, a span that is empty, outside its utterance or on the pause
    knob, overlapping spans, and a whole-utterance Fit beside others."""
    lengths = [int(n) for n in lengths]
    if fits is None:
        return None
    if len(fits) != len(lengths):
        raise ValueError(f"prosody_fit must hold one entry per utterance ({len(lengths)}), got {len(fits)}")
    if all(f is None for f in fits):
        return None
    begins = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = []
    for u, (n, entry) in enumerate(zip(lengths, fits)):
        if entry is None:
            continue
        listed = [entry] if isinstance(entry, Fit) else list(entry)
        if not all(isinstance(f, Fit) for f in listed):
            raise ValueError(f"prosody_fit of utterance {u}: an entry is None, a Fit or a list of Fits")
        taken = []
        for k, f in enumerate(listed):
            where = f"prosody_fit of utterance {u}, segment {k}"
            if f.knob not in ("duration", "pause"):
                raise ValueError(f"{where}: knob {f.knob!r} is neither 'duration' nor 'pause'")
            if f.whole():
                if len(listed) > 1:
                    raise ValueError(f"{where}: a whole-utterance Fit stands alone, the utterance has {len(listed)} Fits")
                kind, a, b = (UTT_DURATION if f.knob == "duration" else UTT_PAUSE), 0, n
                if n == 0:
                    raise ValueError(f"{where}: the utterance has no phonemes")
            else:
                if f.knob != "duration":
                    raise ValueError(f"{where}: a span takes knob='duration' only")
                kind, a, b = SPAN, (0 if f.start is None else int(f.start)), (n if f.stop is None else int(f.stop))
                if not 0 <= a < b <= n:
                    raise ValueError(f"{where}: phonemes [{a}, {b}) are empty or outside the utterance's {n}")
                for j, (a2, b2) in enumerate(taken):
                    if a < b2 and a2 < b:
                        raise ValueError(f"{where}: phonemes [{a}, {b}) overlap segment {j} [{a2}, {b2})")
                taken.append((a, b))
            t = _frames(f, where)
            lo, hi = _bounds(f, kind, where)
            rows.append((u, kind, int(begins[u]) + a, int(begins[u]) + b, t, lo, hi, 1.0 if f.exact else 0.0))
    if int(begins[-1]) > MAX_TARGET:
        raise ValueError(f"prosody_fit: a batch of {int(begins[-1])} phonemes is past the 2^24 rows a segment table can name")
    return np.asarray(rows, dtype=np.float32).reshape(-1, len(SEGMENT_COLUMNS))


def segment_counts(segments, batch):
    """Segments per utterance of a segment table."""
    return np.bincount(segments[:, 0].astype(np.int64), minlength=batch).tolist()


def device_tables(segments):
    """The segment table as tts_prosody_fit takes it: int32 [4, n_seg] (begin | end | utterance | kind) and float32 [n_seg, 4]
    (target, lo, hi, exact)."""
    ints = np.ascontiguousarray(segments[:, [2, 3, 0, 1]].T.astype(np.int32))
    return ints, np.ascontiguousarray(segments[:, 4:8], dtype=np.float32)


def split_report(report, counts):
    """The packed report [n_seg, 8] of a batch -> per utterance [n_u, 8]."""
    out, k = [], 0
    for n in counts:
        out.append(report[k:k + n])
        k += n
    return out


def result(report, scales, extra, segments, lengths):
    """What a call with ``prosody_fit=`` adds to its result: the report per utterance, the solved scales table and the extra frames
    per utterance."""
    counts = segment_counts(segments, len(lengths))
    begins = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return dict(report=split_report(report, counts), scales=scales, extra=[extra[int(b):int(b) + int(n)] for b, n in zip(begins, lengths)])
