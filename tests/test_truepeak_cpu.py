"""The delivery meter without a GPU: the restated interpolator against the resampler's table, faded sines against the EBU Tech 3341
meter tolerance, the loudness range against the analytic cases of Tech 3342, two deliberately wrong range meters that the cases
must tell from the right one, the conditions on the cases (no short-term block on a gate threshold, no order statistic a rounding
away from its neighbour), the limiter's restatement, the keyword errors, and the binding of include/toucan_truepeak.h."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, interface, resample, truepeak
from tests import loudness_ref as lr
from tests import truepeak_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 1024


def test_the_restated_table_is_the_resamplers():
    for sr, F in ((8000, 4), (24000, 4), (48000, 4), (96000, 2), (191990, 2), (192000, 1)):
        assert tr.factor(sr) == truepeak.oversampling(sr) == F
        orig, new, w, tab = resample.kernel_table(sr, F * sr)
        assert (orig, new) == (1, F) and np.array_equal(tab, tr.table(F)) and tab.dtype == np.float32
        got_F, got_w, got = truepeak.interpolator(sr)
        assert (got_F, got_w) == (F, w) and np.array_equal(got, tab) and np.array_equal(truepeak.kernel_table(sr), tab.T)
        assert w == (capi.TRUEPEAK_HALF_WIDTH if F > 1 else 0) and tab.shape[1] == (capi.TRUEPEAK_TAPS if F > 1 else 1)
    # the figures the header's derivations use: A, the centre tap of phase 0 and the sum of its other taps
    assert abs(tr.l1(4) - 1.8689) < 1e-4 and tr.l1(2) == tr.l1(4) and tr.l1(1) == 1.0
    row = np.abs(tr.table(4)[0].astype(np.float64))
    assert abs(row[tr.HALF] - 0.99) < 1e-7 and 0.0505 < row.sum() - row[tr.HALF] < 0.0506
    assert 31 * tr.l1(4) / (row[tr.HALF] - (row.sum() - row[tr.HALF])) < 61.7  # steps of the gain, margin of the trim


@pytest.mark.parametrize("sr", tr.RATES)
def test_faded_sines_read_within_the_meter_tolerance(sr):
    """Every reading within +0.2 / -0.4 dB of the amplitude (EBU Tech 3341); the fs/4 sine at 45 degrees, whose samples all lie
    3.01 dB under its crest, has a sample peak at least 2.9 dB below its true-peak reading."""
    for name, div, phase in tr.SINES:
        for a in tr.AMPLITUDES:
            x = tr.faded_sine(sr, sr / div, phase, a)
            err = tr.db(tr.true_peak(x, sr)) - tr.db(a)
            print(f"{sr} Hz {name} amplitude {a:.4f}: reading {err:+.4f} dB re amplitude")
            assert -0.4 <= err <= 0.2, (sr, name, a, err)
            if (div, phase) == (4, 45.0):
                assert tr.db(tr.true_peak(x, sr)) - tr.db(float(np.abs(x).max())) >= 2.9
            # the fp32 chain the kernel runs stays inside the derived bound of the float64 sum
            assert abs(tr.reading32(x, sr) - tr.true_peak(x, sr)) <= tr.bound(x, sr)


@pytest.mark.parametrize("i", range(len(tr.LRA_CASES)))
def test_loudness_range_of_the_analytic_cases(i):
    c = tr.lra_case(i)
    print(f"{c['name']}: LRA {c['lra']:.6f} LU, {c['kept']} of {c['blocks']} blocks kept ({c['kept_abs']} past the absolute gate)")
    assert abs(c["lra"] - c["want"]) <= 1.0, (c["name"], c["lra"])
    assert c["blocks"] == len(c["x"]) // 800 - 29


def test_a_range_meter_without_the_relative_gate_misses_the_five_level_case():
    c = tr.lra_case(3)
    wrong = tr.loudness_range(c["zs"], relative=False)
    assert abs(wrong["lra"] - c["want"]) > 1.0 and c["kept"] < c["kept_abs"] == wrong["kept"]


def test_a_range_meter_that_floors_the_percentile_index_misses_its_case():
    """Eleven blocks 2 LU apart: ((11 - 1) 95 + 50) / 100 = 10 picks the loudest, the floor picks the one below."""
    zs = 10.0 ** ((np.array([-30.0 + 2.0 * i for i in range(11)]) + 0.691) / 10.0)[::-1].copy()
    right, wrong = tr.loudness_range(zs), tr.loudness_range(zs, floor=True)
    assert right["kept"] == wrong["kept"] == 11 and (right["i_low"], right["i_high"]) == (1, 10) and wrong["i_high"] == 9
    assert abs(right["lra"] - 18.0) < 1e-9 and abs(wrong["lra"] - 18.0) > 1.0


def test_no_block_lies_on_a_gate_and_no_order_statistic_next_to_a_neighbour():
    """The conditions on the inputs: every short-term block at least 1e-3 LU from a gate threshold that decides about it, and the
    two order statistics more than 1e-9 relative from their sorted neighbours, or equal to them.  A different selection on the
    GPU is then a bug, never rounding."""
    cases = [tr.lra_case(i) for i in range(len(tr.LRA_CASES))] + list(tr.range_cases())
    for c in cases:
        gate, order = tr.range_margins(c)
        assert gate >= 1e-3 and order > 1e-9, (c["name"], gate, order)
    kept = [c["kept"] for c in tr.range_cases()]
    assert kept[:9] == [0, 1, 2, 10, 11, 64, 65, 129, 200] and kept[9] < tr.range_cases()[9]["kept_abs"] + 1
    assert tr.range_cases()[9]["blocks"] > tr.range_cases()[9]["kept"] > 0 and tr.range_cases()[-1]["kept_abs"] == 0


@pytest.mark.parametrize("drive", (-2.0, 1.0, 3.0, 6.0))
def test_limiter_restatement(drive):
    """g <= r up to the rounding of its W + 1 additions and one division; g = 1 and the output bit-equal to v where nothing within
    W samples exceeds C; the output's true peak <= C, hard; an utterance without a loudness keeps its bits.  The size of the trim
    is printed, not asserted."""
    sr = 8000
    for name, x in tr.limiter_cases(sr):
        L = lr.loudness(x, sr)
        target = L + (-1.0 - tr.db(tr.reading32(x, sr))) + drive if math.isfinite(L) else -16.0
        res = tr.limiter(x, sr, L, target, -1.0, -1.0)
        W, C, n = res["W"], res["C"], len(x)
        assert W == 16 and (res["g"] <= res["r"] * (1.0 + (W + 2) * 2.0 ** -53)).all(), name
        assert (res["g"] <= 1.0).all() and (res["g"] > 0).all()
        over = res["m"].astype(np.float64) > C
        near = np.convolve(over.astype(np.int64), np.ones(2 * W + 1, dtype=np.int64))[W:W + n] > 0  # an over within W either side
        assert (res["g"][~near] == 1.0).all() and np.array_equal(res["y1"][~near].view(np.uint32), res["v"][~near].view(np.uint32)), name
        if not math.isfinite(L):  # too short for a loudness: through the limiter with its bits, whatever its peaks
            assert np.array_equal(res["y"].view(np.uint32), x.view(np.uint32)) and name == "speech_2T+W" and not over.any()
            continue
        assert tr.reading32(res["y"], sr) <= C and float(np.abs(res["y"]).max()) <= C, name
        assert float(np.abs(res["y1"]).max()) <= C * (1 + 2.0 ** -23)  # samples before the trim: g <= r, then two float32 roundings
        if drive < 0:
            assert not over.any() and res["t"] == 1.0 and np.array_equal(res["y"], res["v"])
        else:
            assert over.any()
        print(f"{name} driven {drive:+.0f} dB: least gain {res['g'].min():.4f}, true peak before the trim {tr.db(res['tp1'] / C):+.5f} dB re ceiling, "
              f"trim {float(res['t']):.7f}")


def test_stepped_gain_restatement():
    """The gain under the true-peak ceiling: the reading of the scaled utterance is <= C, the gain one step up reads over it or
    was not limited by the true peak at all, and the steps stay far inside the header's bound of 63."""
    sr = 8000
    for name, x in tr.limiter_cases(sr) + tuple((c["name"], c["x"]) for c in tr.peak_cases(TILE) if c["n"] > 16):
        g, steps = tr.stepped_gain(x, sr, np.float32(8.0), -1.0)
        C = 10.0 ** (-1.0 / 20.0)
        assert tr.reading32(x * g, sr) <= C and steps <= 63, (name, steps)
        print(f"{name}: {steps} steps")
        if g < np.float32(8.0):
            assert tr.reading32(x * np.nextafter(g, np.float32(9.0)), sr) > C or steps == 0, name


def test_interface_keyword_errors():
    """Either keyword without loudness, together with speech_level, a ceiling above 0 or not finite, stream(), distributed=True and
    increased_compatibility_mode raise ValueError before anything is synthesised (the object has no engines)."""
    tts = object.__new__(interface.ToucanTTSInterface)
    calls = lambda **kw: (lambda: tts.forward("a", **kw), lambda: tts.synthesize_batch(["a"], **kw),
                          lambda: tts.synthesize_ensemble("a", [None], **kw), lambda: tts.synthesize_grid("a", **kw),
                          lambda: tts.read_to_file(["a"], "x.wav", **kw))
    for kw, msg in ((dict(true_peak_ceiling=-1.0), "give loudness"), (dict(limiter=True), "give loudness"),
                    (dict(speech_level=-26.0, true_peak_ceiling=-1.0), "speech_level"), (dict(speech_level=-26.0, limiter=True), "speech_level"),
                    (dict(loudness=-23.0, true_peak_ceiling=0.5), "above full scale"), (dict(loudness=-23.0, true_peak_ceiling=float("nan")), "finite"),
                    (dict(loudness=-23.0, true_peak_ceiling=float("-inf")), "finite"), (dict(loudness=-23.0, true_peak_ceiling="loud"), "finite"),
                    (dict(loudness=-23.0, true_peak_ceiling=True, limiter=True), "finite")):
        for call in calls(**kw):
            with pytest.raises(ValueError, match=msg):
                call()
    for kw in (dict(loudness=-23.0, true_peak_ceiling=-1.0), dict(loudness=-23.0, limiter=True), dict(true_peak_ceiling=-1.0)):
        with pytest.raises(ValueError, match="true-peak ceiling"):
            next(tts.stream("a", **kw))
        with pytest.raises(ValueError, match="distributed"):
            tts.synthesize_batch(["a"], distributed=True, **kw)
        with pytest.raises(ValueError, match="increased_compatibility_mode"):
            tts.read_to_file(["a"], "x.wav", increased_compatibility_mode=True, **kw)
    check = tts._check_delivery
    assert check(None, None, None, False) is False and check(-23.0, None, None, False) is False
    assert check(-23.0, None, -1.0, False) is True and check(-23.0, None, None, True) is True and check(-16, None, 0, True) is True
    with pytest.raises(capi.ToucanHipError, match="GPU only"):
        truepeak.DeliveryMeter("cpu")
    assert truepeak.DELIVERY_COLUMNS == tr.COLUMNS and truepeak.RANGE_COLUMNS[:8] == truepeak.DELIVERY_COLUMNS
    assert len(truepeak.RANGE_COLUMNS) == capi.DELIVERY_N_COLUMNS and len(truepeak.LIMITER_COLUMNS) == capi.LIMITER_N_COLUMNS


def test_truepeak_header_binding_and_library_agree():
    """include/toucan_truepeak.h, capi.TRUEPEAK_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, disjoint from
    every other table and from toucan_tts.h, with the constants the binding mirrors; the entries find bad spans, rates, factors and
    ceilings before anything touches a device, and name the utterance."""
    root = os.path.dirname(HERE)
    raw = open(os.path.join(root, "include", "toucan_truepeak.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.TRUEPEAK_PROTOTYPES) == ["tts_limit_true_peak", "tts_loudness_range", "tts_true_peak", "tts_truepeak_gain",
                                                            "tts_truepeak_tile_samples"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "TRUEPEAK_PROTOTYPES"]
    assert len(tables) >= 12 and all(not set(declared) & set(t) for t in tables)
    for other in ("toucan_tts.h", "toucan_loudness.h"):
        abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", other), encoding="utf-8").read(), flags=re.S)
        assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", abi))
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TTS_TRUEPEAK_TAPS": capi.TRUEPEAK_TAPS, "TTS_TRUEPEAK_HALF_WIDTH": capi.TRUEPEAK_HALF_WIDTH,
                      "TTS_TRUEPEAK_MAX_STEPS": capi.TRUEPEAK_MAX_STEPS, "TTS_TRUEPEAK_TILED_ROUNDS": capi.TRUEPEAK_TILED_ROUNDS, "TTS_TRUEPEAK_SHORT_TERM_SEGMENTS": capi.TRUEPEAK_SHORT_TERM_SEGMENTS,
                      "TTS_DELIVERY_COLUMNS": capi.DELIVERY_N_COLUMNS, "TTS_LIMITER_COLUMNS": capi.LIMITER_N_COLUMNS}
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(capi.TRUEPEAK_PROTOTYPES[name][1]), name
    assert build.SOURCES.index("truepeak.hip") < build.SOURCES.index("activity.hip")
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.TRUEPEAK_PROTOTYPES[n][1] and fn.restype == capi.TRUEPEAK_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15
    assert handle.tts_truepeak_tile_samples() == TILE
    err = lambda: handle.tts_last_error().decode()
    spans = np.array([[0, 5], [3, 11], [5, 5]], dtype=np.int64)
    host = spans.ctypes.data
    peak = lambda n=10, h=host, b=3, mc=11, F=4: handle.tts_true_peak(None, n, None, h, b, mc, None, F, None, None, None)
    gain = lambda c=-1.0, F=4: handle.tts_truepeak_gain(None, 10, None, host, 3, None, F, None, c, None, None, None, None)
    limit = lambda S=2400, F=4, t=-16.0, c=-1.0, ctp=-1.0, mc=11: handle.tts_limit_true_peak(None, 10, None, host, 3, mc, S, None, F, None, t, c, ctp,
                                                                                             None, None, None, None, None, None)
    for call in (peak, gain, limit):
        assert call() == -1 and "utterance 1" in err() and "does not lie inside" in err()
    spans[1] = (3, -1)
    for call in (peak, gain, limit):
        assert call() == -1 and "utterance 1" in err() and "negative" in err()
    spans[1] = (3, 7)
    assert peak(F=3) == -1 and "oversampling factor 3" in err()
    assert gain(F=8) == -1 and "oversampling factor" in err() and limit(F=0) == -1 and "oversampling factor" in err()
    assert peak(mc=6) == -1 and "max_count" in err() and limit(mc=6) == -1 and "max_count" in err()
    assert peak(h=None) == -1 and "host copy" in err()
    assert peak() == -1 and "null pointer" in err() and gain() == -1 and "null pointer" in err() and limit() == -1 and "null pointer" in err()
    assert gain(c=0.5) == -1 and "above full scale" in err() and gain(c=float("nan")) == -1 and "finite" in err()
    assert limit(ctp=0.5) == -1 and "above full scale" in err() and limit(c=0.1) == -1 and "above full scale" in err()
    assert limit(t=float("inf")) == -1 and "finite" in err() and limit(S=799) == -1 and "8000 .. 192000" in err()
    rng = lambda S=2400, ms=1: handle.tts_loudness_range(None, None, None, 10, None, 3, S, ms, None, None, None)
    assert rng(S=19201) == -1 and "8000 .. 192000" in err() and rng(ms=0) == -1 and "max_segments" in err()
    assert rng() == -1 and "null pointer" in err()
    # an empty batch launches nothing
    assert peak(b=0, h=None) == 0 and handle.tts_loudness_range(None, None, None, 10, None, 0, 2400, 1, None, None, None) == 0
    assert handle.tts_truepeak_gain(None, 10, None, None, 0, None, 4, None, -1.0, None, None, None, None) == 0
