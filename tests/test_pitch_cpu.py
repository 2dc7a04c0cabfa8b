"""The pitch tracker without a GPU: the float64 restatement (tests/pitch_ref.py) against the analytic frequency of the seeded
signals, its frame geometry against the formulas of the definition, how robust its decisions are on the
signals the GPU tests compare on, and that the header, the binding and the library declare the same entries."""
import ctypes
import math
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, build, capi, pitch
from tests import pitch_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = pr.SHORT + ("long40",)
WITH_F0 = tuple(n for n in ALL if n != "zeros")


def signal(name):
    return pr.long40() if name == "long40" else pr.signals()[name]


@pytest.mark.parametrize("name", WITH_F0)
def test_restatement_against_analytic_f0(name):
    """At every frame whose window is fully voiced the restatement is within 0.5 % of the analytic frequency at the frame's centre;
    where the window holds only the noise floor no frame is voiced."""
    wave, f0, voiced = signal(name)
    got = pr.analysed(name)["f0"]
    full, silent = pr.window_state(len(wave), voiced)
    analytic = np.interp(pr.frame_times(len(wave)) * pr.SR, np.arange(len(wave)), f0)
    assert full.any() and (got[full] > 0).all()
    rel = np.abs(got[full] - analytic[full]) / analytic[full]
    print(f"{name}: {len(got)} frames, {int(full.sum())} fully voiced, worst relative error {rel.max():.2e}, {int(silent.sum())} silent")
    assert rel.max() <= 5e-3
    assert not (got[silent] > 0).any()
    if name.startswith("glide") or name == "long40":
        assert silent.any()


def test_extremes_of_the_search_range_and_the_octave_step():
    assert np.allclose(pr.analysed("low45")["f0"], 45.0, rtol=5e-3)
    assert np.allclose(pr.analysed("high580")["f0"], 580.0, rtol=5e-3)
    f0 = pr.analysed("step")["f0"]
    assert abs(f0[5] - 200.0) < 1.0 and abs(f0[-5] - 100.0) < 0.5
    assert pr.analysed("high580")["n_cand"].max() == pr.MAX_CAND  # more maxima than places: the pruning runs
    z = pr.analysed("zeros")
    assert not z["f0"].any() and (z["n_cand"] == 1).all() and np.allclose(z["strength"][:, 0], 2.45)


def test_shortest_wave_and_refusal():
    assert len(pr.analysed("shortest")["f0"]) == 1
    for fn in (pr.frame_count, pitch.frame_count, pitch.frame_times):
        with pytest.raises(ValueError):
            fn(pr.MIN_SAMPLES - 1)
    with pytest.raises(ValueError):
        pr.analyse(np.zeros(pr.MIN_SAMPLES - 1, dtype=np.float32))


@pytest.mark.parametrize("n", [1200, 1201, 1455, 1456, 15555, 19200, 160000, 640000])
def test_frame_geometry_matches_the_formulas(n):
    """nfr = floor((n dx - 0.075) / dt) + 1, t = 0.5 n dx - 0.5 nfr dt + 0.5 dt + f dt, left = floor(t / dx - 0.5), in exact
    rationals; the window of every frame lies inside the wave."""
    dx, dt = Fraction(1, 16000), Fraction(256, 16000)
    nfr = math.floor((n * dx - Fraction(75, 1000)) / dt) + 1
    assert pr.frame_count(n) == pitch.frame_count(n) == nfr
    t = [n * dx / 2 - nfr * dt / 2 + dt / 2 + f * dt for f in range(nfr)]
    for times in (pr.frame_times(n), pitch.frame_times(n)):
        assert len(times) == nfr and np.allclose(times, [float(v) for v in t], rtol=0, atol=1e-12)
    left = pr.frame_left(n)
    assert [int(v) for v in left] == [math.floor(v / dx - Fraction(1, 2)) for v in t]
    assert left[0] + 1 - pr.HW >= 0 and left[-1] + 1 - pr.HW + pr.NW <= n


def test_constants_and_window_tables():
    assert (pr.NPER, pr.HPER, pr.HW, pr.NW, pr.MAXLAG, pr.BIX) == (400, 201, 599, 1198, 401, 599)
    assert (pitch.N_CAND, pitch.N_LAGS, pitch.N_WIN, pitch.MIN_SAMPLES) == (pr.MAX_CAND, pr.BIX + 1, pr.NW, pr.MIN_SAMPLES)
    win, wr = pitch.window_tables()
    ref_win, ref_wr = pr.window()
    assert win.dtype == np.float32 and wr.dtype == np.float64 and wr[0] == 1.0
    assert np.abs(win - ref_win).max() < 1e-7 and np.abs(wr - ref_wr).max() < 1e-14


def test_fragile_frames_are_few():
    """A frame is fragile when a rounding error of the kernel's fp32 autocorrelation could change its candidate set."""
    fragile = np.concatenate([pr.analysed(n)["fragile"] for n in ALL])
    print(f"fragile frames: {int(fragile.sum())} of {len(fragile)}")
    assert fragile.mean() <= 0.05


@pytest.mark.parametrize("name", ALL)
def test_path_margins_of_the_test_signals(name):
    """Every decision on the chosen path wins by more than 1e-4, so candidates that differ in the sixth digit give the same path."""
    margin = pr.analysed(name)["margin"]
    print(f"{name}: smallest path margin {margin.min():.2e}")
    assert margin.min() > 1e-4


def test_viterbi_takes_the_first_maximum_on_ties():
    freq = np.zeros((2, pr.MAX_CAND))
    strength = np.zeros((2, pr.MAX_CAND))
    freq[:, 1] = freq[:, 2] = 100.0
    strength[:, 0], strength[:, 1], strength[:, 2] = 0.1, 0.9, 0.9
    f0, margin = pr.viterbi(freq, strength, np.array([3, 3]))
    assert (f0 == 100.0).all() and margin.min() == 0.0


def test_f0_keyword_values():
    stub = types.SimpleNamespace(_tracker=None, device="cpu")
    waves = [np.zeros(2000, dtype=np.float32)] * 2
    assert align.ProsodyExtractor.tracked_f0(stub, waves, None) is None
    given = [np.ones(3), np.ones(4)]
    assert align.ProsodyExtractor.tracked_f0(stub, waves, given) == given and stub._tracker is None
    with pytest.raises(ValueError):
        align.ProsodyExtractor.tracked_f0(stub, waves, "praat")
    with pytest.raises(ValueError):
        align.ProsodyExtractor.tracked_f0(stub, waves, [np.ones(3), "yin"])


def test_pitch_header_binding_and_library_agree():
    """include/toucan_pitch.h, capi.PITCH_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, with the constants
    the binding mirrors; include/toucan_align.h still declares its five entries."""
    root = os.path.dirname(HERE)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", name), encoding="utf-8").read(), flags=re.S)
    text = strip("toucan_pitch.h")
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.PITCH_PROTOTYPES) == ["tts_pitch_candidates", "tts_pitch_path", "tts_wave_stats"]
    others = set(capi.PROTOTYPES) | set(capi.ALIGN_PROTOTYPES) | set(capi.SCORE_PROTOTYPES) | set(capi.GAN_PROTOTYPES)
    assert not set(declared) & others
    macros = dict(re.findall(r"#define\s+(TTS_PITCH_[A-Z_]+)\s+(\d+)", text))
    assert {k: int(v) for k, v in macros.items()} == {
        "TTS_PITCH_CANDIDATES": capi.PITCH_CANDIDATES, "TTS_PITCH_LAGS": capi.PITCH_LAGS, "TTS_PITCH_WINDOW": capi.PITCH_WINDOW,
        "TTS_PITCH_MIN_SAMPLES": capi.PITCH_MIN_SAMPLES, "TTS_PITCH_PATH_LDS_FRAMES": capi.PITCH_PATH_LDS_FRAMES}
    for arg_list, name in zip(re.findall(r"\bint\s+tts_[a-z0-9_]+\s*\((.*?)\)\s*;", text, flags=re.S), re.findall(r"\bint\s+(tts_[a-z0-9_]+)\s*\(", text)):
        assert len(arg_list.split(",")) == len(capi.PITCH_PROTOTYPES[name][1]), name
    assert len(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", strip("toucan_align.h")))) == 5
    assert "pitch.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        assert hasattr(handle, n) and getattr(handle, n).argtypes == capi.PITCH_PROTOTYPES[n][1], n
    assert handle.tts_abi_version() == 15
