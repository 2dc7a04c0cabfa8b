"""The loudness meter without a GPU: the K-weighting coefficients against the table printed in BS.1770-4 and against the analytic
reading of a steady sine, the segment-parallel form the kernels use (zero-state runs, M, carry) against the sequential filter in
numpy, two deliberately wrong meters that the cases must tell from the right one, the condition that no block of a case sits on a
gate threshold, the keyword errors, and the binding of include/toucan_loudness.h."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, interface, loudness
from tests import loudness_ref as lr

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = 64


def case(sr, name):
    return next(c for c in lr.cases(sr, TILE) if c["name"] == name)


def test_coefficients_at_48_khz_are_the_table_of_bs1770():
    for got in (loudness.k_weighting(48000), lr.coefficients(48000)):
        flat = [np.asarray(v, dtype=np.float64) for stage in got for v in stage]
        for have, want in zip(flat, lr.BS1770_48K):
            assert have.dtype == np.float64 and np.abs(have - np.array(want)).max() < 1e-12
    for sr in lr.RATES:
        for (b, a), (rb, ra) in zip(loudness.k_weighting(sr), lr.coefficients(sr)):
            assert np.array_equal(b, np.array(rb)) and np.array_equal(a, np.array(ra))


def test_full_scale_997_hz_sine_at_48_khz_reads_minus_3_01():
    got = lr.loudness(lr.tone(3 * 48000, 48000, 0.0), 48000)
    assert abs(got - (-3.01)) <= 0.01, got


@pytest.mark.parametrize("sr", lr.RATES)
def test_steady_sine_reads_what_the_frequency_response_says(sr):
    """-0.691 + 10 log10(|H|^2 / 2) at 997 Hz and at 2 kHz, within 1e-3 LU: the analytic check of the rates the standard prints no
    table for.  The difference between the rates is the bilinear warp of the shelf."""
    for f in (997.0, 2000.0):
        got = lr.loudness(lr.tone(3 * sr, sr, 0.0, f=f), sr)
        assert abs(got - lr.sine_reading(sr, f)) < 1e-3, (f, got, lr.sine_reading(sr, f))
    want = {48000: -3.0103, 24000: -2.9843, 16000: -2.9700}.get(sr)
    if want is not None:
        assert abs(lr.sine_reading(sr, 997.0) - want) < 1e-4


def segment_parallel(x, sr):
    """The kernels' decomposition in numpy float64, all segments side by side: every segment from the zero state (end states), the
    carry s_{k+1} = M s_k + end_k, every segment again from its start state -> (e_k, start states)."""
    S = sr // 10
    (b, a), (_, c) = loudness.k_weighting(sr)
    M = loudness.transition(sr)
    n = len(x) // S
    seg = np.asarray(x[:n * S], dtype=np.float64).reshape(n, S)

    def run(s):
        s1, s2, s3, s4 = (s[:, i].copy() for i in range(4))
        e = np.zeros(n)
        for t in range(S):
            v = seg[:, t]
            y1 = b[0] * v + s1
            s1, s2 = (b[1] * v + s2) - a[1] * y1, b[2] * v - a[2] * y1
            y2 = y1 + s3
            s3, s4 = (s4 - 2.0 * y1) - c[1] * y2, y1 - c[2] * y2
            e += y2 * y2
        return np.stack([s1, s2, s3, s4], axis=1), e

    ends, _ = run(np.zeros((n, 4)))
    starts = np.zeros((n, 4))
    for k in range(n - 1):
        starts[k + 1] = M @ starts[k] + ends[k]
    return run(starts)[1], starts


@pytest.mark.parametrize("sr,name", [(8000, "past_one_workgroup"), (24000, "noise_5S"), (24000, "dc"), (48000, "sine"), (22050, "gates")])
def test_segment_parallel_form_equals_the_sequential_one(sr, name):
    c = case(sr, name)
    e, starts = segment_parallel(c["x"], sr)
    assert e.shape == c["e"].shape and len(e) >= 4
    # the first segments of the quiet part of "gates" hold the decaying tail only: relative to the loudest segment there
    scale = c["e"] if name != "gates" else np.maximum(c["e"], c["e"].max() * 1e-6)
    assert (np.abs(e - c["e"]) <= 1e-10 * scale).all(), np.abs(e - c["e"]).max()
    assert np.abs(starts[1:]).max() > 0
    assert (np.abs(e - c["e"]) <= c["bound"]).all()  # (and inside the bound the kernel is held to)


def test_transition_is_the_zero_input_map():
    """M applied to a state equals the recurrence run from that state over one segment of zeros; its spectral radius is r^S."""
    for sr in (8000, 24000):
        S, M = sr // 10, loudness.transition(sr)
        assert M.shape == (4, 4) and M.dtype == np.float64
        (b, a), (_, c) = loudness.k_weighting(sr)
        s = np.array([0.3, -0.7, 0.11, 0.5])
        want = s.copy()
        for _ in range(S):
            y1 = want[0]
            y2 = y1 + want[2]
            want = np.array([want[1] - a[1] * y1, -a[2] * y1, want[3] - 2.0 * y1 - c[1] * y2, y1 - c[2] * y2])
        assert np.abs(M @ s - want).max() < 1e-12 * np.abs(want).max()
        r = lr.pole_radius(sr)[0]
        assert abs(np.abs(np.linalg.eigvals(M)).max() ** (1.0 / S) - r) < 1e-3
        tab = loudness.kernel_table(sr)
        assert tab.shape == (capi.LOUDNESS_TABLE_DOUBLES,) and np.array_equal(tab[8:].reshape(4, 4), M) and tab[7] == 0.0
        assert np.array_equal(tab[:7], np.concatenate([b, a[1:], c[1:]]))
    assert [round(lr.pole_radius(sr)[0], 5) for sr in (8000, 24000, 48000)] == [0.97051, 0.99007, 0.99502]


@pytest.mark.parametrize("sr", lr.RATES)
def test_a_meter_without_the_high_pass_misses_the_dc_case(sr):
    c = case(sr, "dc")
    assert abs(lr.loudness(c["x"], sr, highpass=False) - c["lufs"]) > 1.0
    # the offset is gone; what is left is the tone and, in the first block, the step with which the offset sets in
    assert abs(c["lufs"] - (lr.sine_reading(sr, 997.0) - 30.0)) < 1.5


@pytest.mark.parametrize("sr", lr.RATES)
def test_a_meter_without_the_relative_gate_misses_the_two_level_case(sr):
    c = case(sr, "gates")
    assert abs(lr.gate(c["e"], sr // 10, relative=False)["lufs"] - c["lufs"]) > 1.0
    assert c["blocks"] == 57 and c["blocks_both"] < c["blocks_abs"] < c["blocks"]
    assert abs(c["lufs"] - (lr.sine_reading(sr, 997.0) - 20.0)) < 0.5  # the loud part alone


@pytest.mark.parametrize("sr", lr.RATES)
def test_no_block_of_a_case_lies_on_a_gate_threshold(sr):
    """The condition on the inputs: every block is at least 1e-3 LU away from -70 and, past the absolute gate, from the relative
    threshold.  A gate decision that differs on the GPU is then a bug, never rounding.  The lengths aim at the edges."""
    S = sr // 10
    cs = {c["name"]: c for c in lr.cases(sr, TILE)}
    for c in cs.values():
        assert c["margin"] >= 1e-3, (c["name"], c["margin"])
        assert c["blocks"] == max(0, c["n"] // S - 3) and len(c["peaks"]) == -(-c["n"] // S)
    assert [cs[f"noise_{n}"]["blocks"] for n in ("4S-1", "4S", "4S+1", "5S-1", "5S")] == [0, 1, 1, 1, 2]
    assert cs["noise_4S-1"]["lufs"] == -math.inf and cs["empty"]["n"] == 0 and cs["empty"]["lufs"] == -math.inf
    assert cs["zeros"]["blocks"] == 3 and cs["zeros"]["blocks_abs"] == 0 and cs["zeros"]["lufs"] == -math.inf
    assert cs["below_absolute"]["blocks_abs"] == 0 and cs["below_absolute"]["lufs"] == -math.inf and cs["below_absolute"]["peak"] > 0
    assert -90 < cs["below_absolute"]["momentary_max_lufs"] < -70
    # the click: loud enough to be measured, and a target of -23 LUFS would need a gain its peak does not allow under -1 dBFS
    g, limited = lr.gain(cs["click"]["lufs"], cs["click"]["peak"], -23.0, -1.0)
    assert limited and cs["click"]["peak"] == 1.0 and abs(g - 10 ** (-1 / 20)) < 1e-15
    assert not lr.gain(cs["gates"]["lufs"], cs["gates"]["peak"], -23.0, -1.0)[1]
    if sr == 8000:
        assert -(-cs["past_one_workgroup"]["n"] // S) > TILE and -(-cs["past_two_workgroups"]["n"] // S) > 2 * TILE
        assert all(c["n"] < 200000 for c in cs.values())
    assert (np.diff([c["n"] for c in cs.values()]) % 4 != 0).any()  # a ragged batch of them starts utterances at odd samples


def test_k_weighting_refuses_rates_outside_the_rule():
    for bad in (7990, 192010, 22055, 44101, 0, -24000, 24000.5, True, "24000", None):
        with pytest.raises(ValueError, match="multiple of 10"):
            loudness.k_weighting(bad)
        with pytest.raises(ValueError, match="8000 .. 192000"):
            loudness.transition(bad)
    for ok in (8000, 22050, 24000, 44100, 192000):
        assert loudness.segment_samples(ok) * 10 == ok
    with pytest.raises(capi.ToucanHipError, match="GPU only"):
        loudness.LoudnessMeter("cpu")
    assert loudness.LOUDNESS_COLUMNS == lr.COLUMNS and len(loudness.LOUDNESS_COLUMNS) == capi.LOUDNESS_N_COLUMNS == 8


def test_interface_keyword_errors():
    """A target or ceiling that is not finite, a ceiling above 0, stream(), distributed=True, increased_compatibility_mode and
    evaluate_against_recordings raise ValueError before anything is synthesised (the object has no engines)."""
    tts = object.__new__(interface.ToucanTTSInterface)
    calls = lambda **kw: (lambda: tts.forward("a", **kw), lambda: tts.synthesize_batch(["a"], **kw),
                          lambda: tts.synthesize_ensemble("a", [None], **kw), lambda: tts.synthesize_grid("a", **kw),
                          lambda: tts.read_to_file(["a"], "x.wav", **kw))
    for kw, msg in ((dict(loudness=float("nan")), "finite"), (dict(loudness=float("inf")), "finite"), (dict(loudness="loud"), "finite"),
                    (dict(loudness=-23.0, peak_ceiling=float("-inf")), "finite"), (dict(loudness=-23.0, peak_ceiling=None), "finite"),
                    (dict(loudness=-23.0, peak_ceiling=0.5), "above full scale")):
        for call in calls(**kw):
            with pytest.raises(ValueError, match=msg):
                call()
    with pytest.raises(ValueError, match="whole utterance"):
        next(tts.stream("a", loudness=-23.0))
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch(["a"], distributed=True, loudness=-23.0)
    with pytest.raises(ValueError, match="increased_compatibility_mode"):
        tts.read_to_file(["a"], "x.wav", increased_compatibility_mode=True, loudness=-23.0)
    with pytest.raises(ValueError, match="peak"):
        tts.evaluate_against_recordings(["a"], [(np.zeros(10), 24000)], loudness=-23.0)
    assert tts._check_loudness(None, float("nan")) is False and tts._check_loudness(-23, -1) is True and tts._check_loudness(-16.0, 0.0) is True


def test_loudness_header_binding_and_library_agree():
    """include/toucan_loudness.h, capi.LOUDNESS_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, disjoint from
    every other table, with the constants the binding mirrors; the entries find bad spans, rates and targets before anything
    touches a device, and name the utterance."""
    root = os.path.dirname(HERE)
    raw = open(os.path.join(root, "include", "toucan_loudness.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.LOUDNESS_PROTOTYPES) == ["tts_apply_gain", "tts_kweight_energy", "tts_loudness_gate", "tts_loudness_tile_segments"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "LOUDNESS_PROTOTYPES"]
    assert len(tables) >= 10 and all(not set(declared) & set(t) for t in tables)
    abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "toucan_tts.h"), encoding="utf-8").read(), flags=re.S)
    assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", abi))
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_LOUDNESS_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TTS_LOUDNESS_MIN_RATE": capi.LOUDNESS_MIN_RATE, "TTS_LOUDNESS_MAX_RATE": capi.LOUDNESS_MAX_RATE,
                      "TTS_LOUDNESS_COLUMNS": capi.LOUDNESS_N_COLUMNS, "TTS_LOUDNESS_TABLE_DOUBLES": capi.LOUDNESS_TABLE_DOUBLES}
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(capi.LOUDNESS_PROTOTYPES[name][1]), name
    assert "loudness.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.LOUDNESS_PROTOTYPES[n][1] and fn.restype == capi.LOUDNESS_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15
    assert handle.tts_loudness_tile_segments() == TILE
    err = lambda: handle.tts_last_error().decode()
    spans = np.array([[0, 5], [3, 11], [5, 5]], dtype=np.int64)
    host = spans.ctypes.data
    assert handle.tts_kweight_energy(None, 10, None, host, 3, 2400, None, 1, None, None, None, None) == -1 and "utterance 1" in err()
    assert handle.tts_apply_gain(None, 10, None, host, 3, 11, None, None, None) == -1 and "utterance 1" in err()
    spans[1] = (3, -1)
    assert handle.tts_kweight_energy(None, 10, None, host, 3, 2400, None, 1, None, None, None, None) == -1
    assert "utterance 1" in err() and "negative" in err()
    spans[1] = (3, 7)
    assert handle.tts_kweight_energy(None, 10, None, host, 3, 799, None, 1, None, None, None, None) == -1 and "8000 .. 192000" in err()
    assert handle.tts_kweight_energy(None, 10, None, host, 3, 2400, None, 0, None, None, None, None) == -1 and "max_segments" in err()
    assert handle.tts_kweight_energy(None, 10, None, None, 3, 2400, None, 1, None, None, None, None) == -1 and "host copy" in err()
    assert handle.tts_kweight_energy(None, 10, None, host, 3, 2400, None, 1, None, None, None, None) == -1 and "null pointer" in err()
    assert handle.tts_apply_gain(None, 10, None, host, 3, 6, None, None, None) == -1 and "max_count" in err()
    for target, ceiling, word in ((-23.0, 0.5, "above full scale"), (float("inf"), -1.0, "finite"), (-23.0, float("nan"), "finite")):
        assert handle.tts_loudness_gate(None, None, 10, None, 3, 2400, 1, target, ceiling, None, None) == -1 and word in err()
    assert handle.tts_loudness_gate(None, None, 10, None, 3, 2400, 1, float("nan"), 7.0, None, None) == -1 and "null pointer" in err()
    assert handle.tts_kweight_energy(None, 10, None, None, 0, 2400, None, 1, None, None, None, None) == 0  # an empty batch launches nothing
