"""The speech-activity meter without a GPU: the three forms of the hangover count of tests/activity_ref.py against each other (the
definition, the literal counter, the segment form the kernels use), scale covariance, the full-scale sine, the bounds of a burst,
padding invariance, the condition under which the GPU's counts may be demanded exact, the segment-parallel envelope (zero-state
runs, T, carry) against the sequential one, the keyword errors, and the binding of include/toucan_activity.h."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import activity, align, build, capi
from tests import activity_ref as ar
from tests.test_interface_cpu import models_dir, tts  # noqa: F401  (the CPU fixture: the interface on the ABI emulator)

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 64


def case(sr, name):
    return next(c for c in ar.cases(sr, TILE) if c["name"] == name)


@pytest.mark.parametrize("sr,names", [(8000, ("noise_S+1", "click", "bursts_far", "three_runs", "partial_only", "across_workgroups")),
                                      (22050, ("noise_S-1", "bursts_close", "partial_only"))])
def test_the_three_forms_of_the_count_agree(sr, names):
    """Sample by sample with the literal hangover counter, by the definition, and from the first and last sample of every segment
    with the integer carry: the same number at every threshold of the ladder and at the final one; the runs likewise."""
    S = sr // 10
    for name in names:
        c = case(sr, name)
        for thr, want in list(zip(ar.LADDER, c["a"])) + [(c["c_star"], None)]:
            above = c["q"] >= thr
            a = ar.active_count(above, 2 * S)
            assert a == ar.active_count_literal(above, 2 * S) == ar.active_count_segments(above, S, 2 * S), (name, thr)
            assert want is None or a == want
        # the runs from the segments' first and last positions, as the kernel walks them
        runs, begin, last = [], -1, -1
        for k, (_, f, l) in enumerate(ar.segment_positions(c["q"] >= c["c_star"], S)):
            if f < 0:
                continue
            if begin >= 0 and k * S + f - last > 2 * S:
                runs.append((begin, last + 1))
                begin = -1
            begin = k * S + f if begin < 0 else begin
            last = k * S + l
        if begin >= 0:
            runs.append((begin, last + 1))
        assert runs == c["runs"], name


def test_halving_the_signal_moves_the_counts_one_threshold_up():
    """0.5 x: a_j(0.5 x) = a_{j+1}(x) exactly (halving is exact in binary and the ladder is powers of two), both levels lower by
    20 log10 2 within 1e-12 dB, the runs the same."""
    for sr, name in ((8000, "bursts_far"), (16000, "sine"), (8000, "noise_S+1")):
        c = case(sr, name)
        half = ar.measure(c["x"] * np.float32(0.5), sr)
        assert half["a"][:-1] == c["a"][1:] and half["a"][-1] <= c["a"][-1]
    c = case(8000, "bursts_far")
    # (the level moves by exactly 6.02 dB only where the same pair of thresholds brackets it: bursts_far at 8 kHz does not use a_0)
    assert c["threshold_db"] > 20.0 * math.log10(ar.LADDER[1])
    half = ar.measure(c["x"] * np.float32(0.5), 8000)
    step = 20.0 * math.log10(2.0)
    assert abs(half["active_db"] - (c["active_db"] - step)) < 1e-12 and abs(half["long_term_db"] - (c["long_term_db"] - step)) < 1e-12
    assert abs(half["threshold_db"] - (c["threshold_db"] - step)) < 1e-12 and half["runs"] == c["runs"]


def test_full_scale_sine_reads_minus_3_01():
    x = ar.tone(3 * 8000, 8000, 0.0)
    m = ar.measure(x, 8000)
    assert abs(m["long_term_db"] - (-3.0103)) < 1e-3
    assert abs(m["active_db"] - m["long_term_db"]) <= 0.05, m["active_db"]  # (-2.977: the 20 ms of the onset are not active)
    assert 0.98 < m["activity"] <= 1.0 and len(m["runs"]) == 1


@pytest.mark.parametrize("sr", ar.RATES)
def test_the_bounds_of_a_burst_trail_its_onset_and_offset(sr):
    """The envelope crosses the final threshold within 25 ms of an onset and within 120 ms of an offset (about 20 and 100)."""
    S = sr // 10
    c = case(sr, "bursts_far")
    (b0, e0), (b1, e1) = c["runs"]
    for got, true, late in ((b0, 1 * S, 0.025), (e0, 4 * S, 0.120), (b1, 12 * S, 0.025), (e1, 15 * S, 0.120)):
        assert 0 <= got - true <= late * sr, (got, true)
    assert c["speech_begin"] == b0 and c["speech_end"] == e1
    assert len(case(sr, "bursts_close")["runs"]) == 1 and len(case(sr, "three_runs")["runs"]) == 3 > ar.MAX_RUNS
    assert case(sr, "partial_only")["speech_begin"] >= 3 * S and case(sr, "partial_only")["speech_end"] == case(sr, "partial_only")["n"]
    # the product's host helpers on these rows
    row = np.zeros((1, 8))
    row[0, 4:6] = (b0, e1)
    assert activity.bounds(row, lead=sr * 30 // 1000) == [(b0 - sr * 30 // 1000, e1)] and activity.bounds(np.zeros((1, 8)), 5) == [None]
    assert activity.bounds(row, lead=10 ** 9) == [(0, e1)]
    assert activity.pauses(np.array(c["runs"] + [(0, 0)]), 2) == [(e0, b1)] and activity.pauses(np.zeros((4, 2)), 0) == []
    assert activity.pauses(np.array(case(sr, "three_runs")["runs"][:2]), 3) == [(case(sr, "three_runs")["runs"][0][1], case(sr, "three_runs")["runs"][1][0])]


def test_zeros_behind_a_second_of_zeros_change_nothing_but_the_long_term_level():
    sr = 8000
    x = np.concatenate([ar.bursts(sr, [(1, False), (3, True)]), np.zeros(sr, dtype=np.float32)])
    longer = np.concatenate([x, np.zeros(3 * sr + 17, dtype=np.float32)])
    a, b = ar.measure(x, sr), ar.measure(longer, sr)
    assert a["a"] == b["a"] and a["sq"] == b["sq"] and a["active_db"] == b["active_db"] and a["runs"] == b["runs"]
    assert abs(b["long_term_db"] - (a["long_term_db"] - 10.0 * math.log10(len(longer) / len(x)))) < 1e-12


@pytest.mark.parametrize("sr", ar.RATES)
def test_no_envelope_sample_of_a_case_lies_on_a_threshold(sr):
    """The condition on the inputs: every q_t is at least 1e-9 (relative) away from every threshold of the ladder and from the
    final one.  The kernel's envelope differs from the restatement's by parts in 10^13 (the state bound), so a count, a run or a
    bound that differs on the GPU is then a bug, never rounding.  The lengths and contents aim at the edges."""
    S = sr // 10
    cs = {c["name"]: c for c in ar.cases(sr, TILE)}
    for c in cs.values():
        assert c["ladder_margin"] >= 1e-9 and c["final_margin"] >= 1e-9, (c["name"], c["ladder_margin"], c["final_margin"])
        assert len(c["starts"]) == -(-c["n"] // S) and all(x >= y for x, y in zip(c["a"], c["a"][1:]))
    assert [cs[n]["n"] for n in ("empty", "one", "noise_S-1", "noise_S", "noise_S+1")] == [0, 1, S - 1, S, S + 1]
    for name in ("empty", "one", "zeros", "too_quiet"):
        c = cs[name]
        assert c["a"][0] == 0 and c["active_db"] == c["long_term_db"] == c["threshold_db"] == -math.inf and c["runs"] == [], name
    assert cs["too_quiet"]["sq"] > 0 and cs["zeros"]["sq"] == 0 and cs["one"]["sq"] == 0.25
    # the click: no threshold stands within 15.9 dB of its level, so the last one with active samples is taken; and a target of
    # -26 dB would need a gain its peak does not allow under -1 dBFS
    k = cs["click"]
    last = max(j for j in range(15) if k["a"][j] > 0)
    assert k["threshold_db"] == 20.0 * math.log10(ar.LADDER[last]) and k["active_db"] - k["threshold_db"] > ar.MARGIN_DB
    assert ar.gain(k["active_db"], k["peak"], -26.0, -1.0)[1] and k["peak"] == 1.0
    assert not ar.gain(cs["bursts_far"]["active_db"], cs["bursts_far"]["peak"], -26.0, -1.0)[1]
    assert S % 64 != 0 if sr == 22050 else True
    if sr == 8000:
        assert cs["one_workgroup"]["n"] == TILE * S and -(-cs["across_workgroups"]["n"] // S) == TILE + 3
        assert cs["past_two_workgroups"]["n"] == (2 * TILE + 3) * S == 104800
        # the burst ends five samples before the first workgroup's last segment: at the upper thresholds the last sample at the
        # threshold lies in that workgroup and its hangover runs on into the next
        c = cs["across_workgroups"]
        lasts = [int(np.flatnonzero(c["q"] >= t)[-1]) for t, a in zip(ar.LADDER, c["a"]) if a > 0]
        assert min(lasts) < TILE * S <= min(lasts) + 2 * S and max(lasts) >= TILE * S
        assert all(c["n"] < 200000 for c in cs.values())


@pytest.mark.parametrize("sr,name", [(8000, "across_workgroups"), (22050, "bursts_close"), (48000, "noise_S+1"), (24000, "three_runs")])
def test_segment_parallel_envelope_equals_the_sequential_one(sr, name):
    """The kernels' decomposition in numpy float64: every complete segment from the zero state, the carry s_{k+1} = T s_k + end_k
    with the product's T: the start states of all slots within the bound the kernel is held to."""
    c = case(sr, name)
    S, g = sr // 10, activity.coefficient(sr)
    assert g == ar.coefficient(sr)
    T = activity.transition(sr)
    tab = activity.kernel_table(sr)
    assert tab.shape == (capi.ACTIVITY_TABLE_DOUBLES,) and tab[0] == g and tab[1] == 1.0 - g and np.array_equal(tab[2:].reshape(2, 2), T)
    assert T[0, 1] == 0.0 and 0 < T[1, 0] < 0.13 and abs(T[0, 0] - math.exp(-10.0 / 3.0)) < 1e-12 and T[0, 0] == T[1, 1]
    starts = np.zeros_like(c["starts"])
    for k in range(len(starts) - 1):
        end = np.array([v[-1] for v in ar.envelope(c["x"][k * S:(k + 1) * S], sr)])
        starts[k + 1] = T @ starts[k] + end
    assert np.abs(starts).max() > 0 or c["n"] <= S
    assert (np.abs(starts - c["starts"]) <= c["state_bound"]).all() and c["state_bound"] < 1e-11


def test_module_refuses_rates_targets_and_the_cpu():
    for bad in (7990, 192010, 22055, 0, 24000.5, True, "24000", None):
        with pytest.raises(ValueError, match="multiple of 10"):
            activity.coefficient(bad)
        with pytest.raises(ValueError, match="8000 .. 192000"):
            activity.kernel_table(bad)
    for ok in (8000, 22050, 24000, 192000):
        assert activity.segment_samples(ok) * 10 == ok
    for target, ceiling, msg in ((float("nan"), -1.0, "finite"), (float("inf"), -1.0, "finite"), ("loud", -1.0, "finite"), (-26.0, None, "finite"),
                                 (-26.0, float("-inf"), "finite"), (-26.0, 0.5, "above full scale")):
        with pytest.raises(ValueError, match=msg):
            activity.check_target(target, ceiling)
    activity.check_target(-26, 0.0)
    with pytest.raises(ValueError, match="negative"):
        activity.bounds(np.zeros((1, 8)), -1)
    with pytest.raises(capi.ToucanHipError, match="GPU only"):
        activity.SpeechActivity("cpu")
    assert activity.ACTIVITY_COLUMNS == ar.COLUMNS and len(activity.ACTIVITY_COLUMNS) == capi.ACTIVITY_N_COLUMNS == 8
    assert activity.ACTIVITY_COLUMNS.index("gain") == 6  # where the gain kernel of the loudness meter reads it
    assert align.DETECT == "detect" and align.DETECT_LEAD == 16000 * activity.DEFAULT_LEAD_MS // 1000 == 480


def test_interface_keyword_errors(tts):  # noqa: F811
    """loudness and speech_level together, a target or ceiling that is not finite, a ceiling above 0, stream(), distributed=True,
    increased_compatibility_mode and evaluate_against_recordings raise ValueError before anything is launched."""
    calls = lambda **kw: (lambda: tts.forward("a", **kw), lambda: tts.synthesize_batch(["a"], **kw),
                          lambda: tts.synthesize_ensemble("a", [None], **kw), lambda: tts.synthesize_grid("a", **kw),
                          lambda: tts.read_to_file(["a"], "x.wav", **kw))
    before = capi.CALLS
    for kw, msg in ((dict(speech_level=float("nan")), "finite"), (dict(speech_level=float("inf")), "finite"), (dict(speech_level="loud"), "finite"),
                    (dict(speech_level=-26.0, peak_ceiling=float("-inf")), "finite"), (dict(speech_level=-26.0, peak_ceiling=None), "finite"),
                    (dict(speech_level=-26.0, peak_ceiling=0.5), "above full scale"), (dict(speech_level=-26.0, loudness=-23.0), "give one of them")):
        for call in calls(**kw):
            with pytest.raises(ValueError, match=msg):
                call()
    with pytest.raises(ValueError, match="whole utterance"):
        next(tts.stream("a", speech_level=-26.0))
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch(["a"], distributed=True, speech_level=-26.0)
    with pytest.raises(ValueError, match="increased_compatibility_mode"):
        tts.read_to_file(["a"], "x.wav", increased_compatibility_mode=True, speech_level=-26.0)
    with pytest.raises(ValueError, match="peak"):
        tts.evaluate_against_recordings(["a"], [(np.zeros(10), 24000)], speech_level=-26.0)
    assert capi.CALLS == before and tts.last_speech_activity is None
    assert tts._check_speech_level(None, None, float("nan")) is False and tts._check_speech_level(None, -26, -1) is True
    with pytest.raises(ValueError, match="pairs or 'detect'"):
        align.extract_prosody_batch(None, ["a"], [np.zeros(16000)], 16000, speech_bounds="find")
    with pytest.raises(ValueError, match="utterance 0"):
        align.extract_prosody_batch(None, ["a"], [np.zeros(16000)], 16000, speech_bounds=["find"])


def test_activity_header_binding_and_library_agree():
    """include/toucan_activity.h, capi.ACTIVITY_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, disjoint from
    every other table, with the constants the binding mirrors; the entries find bad spans, rates and targets before anything
    touches a device, and name the utterance."""
    root = os.path.dirname(HERE)
    raw = open(os.path.join(root, "include", "toucan_activity.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.ACTIVITY_PROTOTYPES) == ["tts_activity_envelope", "tts_activity_level", "tts_activity_runs", "tts_activity_tile_segments"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "ACTIVITY_PROTOTYPES"]
    assert len(tables) >= 11 and all(not set(declared) & set(t) for t in tables)
    for other in os.listdir(os.path.join(root, "include")):
        if other != "toucan_activity.h":
            theirs = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", other), encoding="utf-8").read(), flags=re.S)
            assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", theirs)), other
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_ACTIVITY_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TTS_ACTIVITY_MIN_RATE": capi.ACTIVITY_MIN_RATE, "TTS_ACTIVITY_MAX_RATE": capi.ACTIVITY_MAX_RATE,
                      "TTS_ACTIVITY_COLUMNS": capi.ACTIVITY_N_COLUMNS, "TTS_ACTIVITY_THRESHOLDS": capi.ACTIVITY_THRESHOLDS,
                      "TTS_ACTIVITY_COUNTS": capi.ACTIVITY_COUNTS, "TTS_ACTIVITY_TABLE_DOUBLES": capi.ACTIVITY_TABLE_DOUBLES}
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(capi.ACTIVITY_PROTOTYPES[name][1]), name
    assert build.SOURCES[-1] == "activity.hip" and "loudness.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.ACTIVITY_PROTOTYPES[n][1] and fn.restype == capi.ACTIVITY_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15 == capi.ABI_VERSION
    assert handle.tts_activity_tile_segments() == TILE
    err = lambda: handle.tts_last_error().decode()
    spans = np.array([[0, 5], [3, 11], [5, 5]], dtype=np.int64)
    host = spans.ctypes.data
    envelope = lambda host, batch, S, most: handle.tts_activity_envelope(None, 10, None, host, batch, S, None, most, None, None, None, None, None)
    runs = lambda host, batch, S, most, cap: handle.tts_activity_runs(None, 10, None, host, batch, S, None, most, None, None, cap, None, None, None, None)
    assert envelope(host, 3, 2400, 1) == -1 and "utterance 1" in err()
    assert runs(host, 3, 2400, 1, 4) == -1 and "utterance 1" in err()
    spans[1] = (3, -1)
    assert envelope(host, 3, 2400, 1) == -1 and "utterance 1" in err() and "negative" in err()
    spans[1] = (3, 7)
    assert envelope(host, 3, 799, 1) == -1 and "8000 .. 192000" in err()
    assert envelope(host, 3, 2400, 0) == -1 and "max_segments" in err()
    assert envelope(None, 3, 2400, 1) == -1 and "host copy" in err()
    assert envelope(host, 3, 2400, 1) == -1 and "null pointer" in err()
    assert runs(host, 3, 2400, 1, -1) == -1 and "max_runs" in err()
    assert runs(host, 3, 2400, 1, 4) == -1 and "null pointer" in err()
    level = lambda target, ceiling: handle.tts_activity_level(None, None, None, 10, None, 3, 2400, 1, target, ceiling, None, None, None, None)
    for target, ceiling, word in ((-26.0, 0.5, "above full scale"), (float("inf"), -1.0, "finite"), (-26.0, float("nan"), "finite")):
        assert level(target, ceiling) == -1 and word in err()
    assert level(float("nan"), 7.0) == -1 and "null pointer" in err()
    assert envelope(None, 0, 2400, 1) == 0 and runs(None, 0, 2400, 1, 4) == 0  # an empty batch launches nothing
