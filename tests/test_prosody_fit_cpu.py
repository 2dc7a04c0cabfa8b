"""Time budgets without a GPU: the numpy restatement (tests/prosody_fit_ref.py) checked against the frame count itself, the seeded
fixture's coverage, monotonicity, prosody_fit.resolve_fits, header / binding / library agreement, the entries' argument checks and
the interface's validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, interface, prosody_fit
from ims_toucan_prosody_variance_amd.prosody_fit import Fit
from tests import abi_emulator, prosody_fit_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PHONES_A = "~həlˈoʊ wˈɜːld~#"
PHONES_B = "~tˈɛst~#"
CONFIGS = [(True, True), (True, False), (False, True), (False, False)]  # (input scales, input curve table)


@pytest.fixture(scope="module")
def fx():
    return ref.fixture()


def _tables(fx, with_scales, with_curves):
    return (fx["scales"] if with_scales else None), (fx["curves"] if with_curves else None)


def _segment_inputs(fx, g, scales, curves):
    u, kind, b, e = (int(v) for v in g[:4])
    c = np.ones(e - b, dtype=np.float32) if curves is None else curves[b:e, 0]
    sd, sp = (1.0, 1.0) if scales is None else (scales[u][0], scales[u][3])
    return fx["text"][b:e], fx["dur"][b:e], c, kind, sd, sp


@pytest.mark.parametrize("with_scales,with_curves", CONFIGS)
def test_every_solved_segment_against_the_frame_count_itself(fx, with_scales, with_curves):
    """(i) the search is not trusted on its own: F is evaluated at the value, at its neighbours and at the bounds."""
    scales, curves = _tables(fx, with_scales, with_curves)
    scales_out, curves_out, extra, report, solved = ref.fit(fx["text"], fx["dur"], fx["lengths"], fx["segments"], scales, curves)
    final = ref.control_durations(fx["text"], fx["dur"], fx["lengths"], scales_out, curves_out) + extra
    given = ref.control_durations(fx["text"], fx["dur"], fx["lengths"], scales, curves)
    for s, (one, g) in enumerate(zip(solved, fx["segments"])):
        text, dur, c, kind, sd, sp = _segment_inputs(fx, g, scales, curves)
        b, e, T, lo, hi = int(g[2]), int(g[3]), int(g[4]), np.float32(g[5]), np.float32(g[6])
        F = lambda x: ref.frames(text, dur, c, kind, x, sd, sp)
        D = lambda x: ref.rows(text, dur, c, kind, x, sd, sp)
        v, status = one["value"], one["status"]
        assert report[s, 0] == T and report[s, 2] == F(v) and report[s, 3] == v and report[s, 4] == status, s
        assert report[s, 7] == given[b:e].sum() and report[s, 1] == final[b:e].sum() == F(v) + one["extra"].sum(), s
        assert report[s, 5] <= 31 and report[s, 6] == (one["extra"] > 0).sum(), s
        if status == ref.EXACT:
            assert F(v) == T and lo <= v <= hi and (v == lo or F(ref.pred(v)) < T), s
        elif status == ref.REPAIRED:
            assert lo <= v < hi and F(v) < T <= F(ref.succ(v)), s
            delta = D(ref.succ(v)) - D(v)
            assert (one["extra"] >= 0).all() and (one["extra"] <= delta).all() and one["extra"].sum() == T - F(v), s
            assert final[b:e].sum() == T, s
        elif status == ref.NEAREST:
            x0, x1 = one["x0"], one["x1"]
            assert x1 == ref.succ(x0) and F(x0) < T < F(x1) and v in (x0, x1) and not g[7], s
            other = x1 if v == x0 else x0
            assert abs(F(v) - T) <= abs(F(other) - T) and (v == x0 or abs(F(v) - T) < abs(F(other) - T)), s
        elif status == ref.CLAMPED_LOW:
            assert v == lo and F(lo) > T, s
        elif status == ref.CLAMPED_HIGH:
            assert v == hi and F(hi) < T, s
        else:
            assert status == ref.EMPTY and F(lo) == F(hi) and np.array_equal(final[b:e], given[b:e]), s
        if status not in (ref.REPAIRED,):
            assert not one["extra"].any(), s
    covered = np.zeros(len(fx["dur"]), dtype=bool)
    for g in fx["segments"]:
        covered[int(g[2]):int(g[3])] = True
    assert np.array_equal(final[~covered], given[~covered]) and not extra[~covered].any()
    if curves is not None:  # only column 0 of solved spans is rewritten
        assert np.array_equal(curves_out[:, 1:], curves[:, 1:]) and np.array_equal(curves_out[~covered], curves[~covered])


def test_fixture_holds_every_case(fx):
    """(ii) lengths, the two special utterances, every status, and a row that gains two frames between neighbouring knob values."""
    assert set(fx["lengths"]) == {1, 7, 257, 1000}
    begins = np.concatenate([[0], np.cumsum(fx["lengths"])])
    zero, quiet = (slice(begins[u], begins[u + 1]) for u in (ref.ALL_ZERO, ref.NO_SILENCE))
    assert not fx["dur"][zero].any() and not (fx["text"][quiet, ref.F_SILENCE] == 1).any()
    kinds = {(int(g[0]), int(g[1])) for g in fx["segments"]}
    assert (ref.NO_SILENCE, ref.UTT_PAUSE) in kinds and (ref.ALL_ZERO, ref.UTT_DURATION) in kinds and ref.UNFITTED not in {u for u, _ in kinds}
    assert 0 <= fx["dur"].min() and fx["dur"].max() <= 12
    _, _, extra, report, solved = ref.fit(fx["text"], fx["dur"], fx["lengths"], fx["segments"], fx["scales"], fx["curves"])
    assert {one["status"] for one in solved} == {ref.EMPTY, ref.EXACT, ref.REPAIRED, ref.NEAREST, ref.CLAMPED_LOW, ref.CLAMPED_HIGH}
    by_segment = {(int(g[0]), int(g[1])): one["status"] for one, g in zip(solved, fx["segments"])}
    assert by_segment[(ref.ALL_ZERO, ref.UTT_DURATION)] == ref.EMPTY and by_segment[(ref.NO_SILENCE, ref.UTT_PAUSE)] == ref.EMPTY
    assert {int(g[1]) for one, g in zip(solved, fx["segments"]) if one["status"] == ref.REPAIRED} == {ref.UTT_DURATION, ref.UTT_PAUSE, ref.SPAN}
    largest = 0
    for one, g in zip(solved, fx["segments"]):
        if one["status"] == ref.REPAIRED:
            text, dur, c, kind, sd, sp = _segment_inputs(fx, g, fx["scales"], fx["curves"])
            delta = ref.rows(text, dur, c, kind, one["x1"], sd, sp) - ref.rows(text, dur, c, kind, one["x0"], sd, sp)
            largest = max(largest, int(delta.max()))
    assert largest == 2 and extra.max() == 2
    assert (report < 2 ** 24).all()


def test_hand_made_repair():
    text = np.zeros((4, 62), dtype=np.float32)
    dur = np.array([3, 3, 3, 3])
    one = ref.solve_one(text, dur, np.ones(4, dtype=np.float32), ref.UTT_DURATION, 14, 0.25, 4.0, True)
    # F(s) = 4 rint(3 s): 12 up to s = 7/6 (3.5 rounds to 4 at the tie), 16 from there on
    assert one["status"] == ref.REPAIRED and ref.frames(text, dur, np.ones(4, dtype=np.float32), ref.UTT_DURATION, one["value"], 1, 1) == 12
    assert one["extra"].tolist() == [0, 1, 0, 1] and one["report"].tolist()[:3] == [14, 14, 12] and one["report"][6] == 2
    near = ref.solve_one(text, dur, np.ones(4, dtype=np.float32), ref.UTT_DURATION, 14, 0.25, 4.0, False)
    assert near["status"] == ref.NEAREST and near["value"] == one["value"] and not near["extra"].any()  # (a tie goes to x0)
    assert ref.solve_one(text, dur, np.ones(4, dtype=np.float32), ref.UTT_DURATION, 15, 0.25, 4.0, False)["value"] == ref.succ(one["value"])
    text[1, ref.F_SILENCE] = 1
    pause = ref.solve_one(text, dur, np.ones(4, dtype=np.float32), ref.UTT_PAUSE, 11, 0.0, 8.0, True)
    assert pause["status"] == ref.EXACT and ref.rows(text, dur, np.ones(4, dtype=np.float32), ref.UTT_PAUSE, pause["value"], 1, 1).tolist() == [3, 2, 3, 3]
    assert ref.solve_one(text, dur, np.ones(4, dtype=np.float32), ref.UTT_PAUSE, 8, 0.0, 8.0, True)["status"] == ref.CLAMPED_LOW
    text[1, ref.F_SILENCE] = 0
    assert ref.solve_one(text, dur, np.ones(4, dtype=np.float32), ref.UTT_PAUSE, 11, 0.0, 8.0, True)["status"] == ref.EMPTY


@pytest.mark.parametrize("kind", [ref.UTT_DURATION, ref.UTT_PAUSE, ref.SPAN])
def test_frame_count_does_not_decrease_in_the_knob(fx, kind):
    """(iii)"""
    rng = np.random.default_rng(5)
    xs = np.sort(np.concatenate([rng.uniform(0.0 if kind == ref.UTT_PAUSE else 0.05, 8.0, 400), [0.25, 0.5, 1.0, 1.5, 2.0, 4.0]]).astype(np.float32))
    xs = np.sort(np.concatenate([xs, [ref.pred(x) for x in xs[1:]], [ref.succ(x) for x in xs]]).astype(np.float32))
    begins = np.concatenate([[0], np.cumsum(fx["lengths"])])
    for u in (2, 3):
        sl = slice(begins[u], begins[u + 1])
        counts = [ref.frames(fx["text"][sl], fx["dur"][sl], fx["curves"][sl, 0], kind, x, fx["scales"][u][0], fx["scales"][u][3]) for x in xs]
        assert all(a <= b for a, b in zip(counts, counts[1:])) and counts[0] < counts[-1]


def test_resolve_fits_and_its_errors():
    """(iv)"""
    assert prosody_fit.resolve_fits([3, 4], None) is None and prosody_fit.resolve_fits([3, 4], [None, None]) is None
    t = prosody_fit.resolve_fits([3, 4, 5], [Fit(target_frames=40), None, [Fit(target_seconds=0.2, start=1, stop=3), Fit(7, start=3, exact=False, bounds=(0.5, 2))]])
    assert t.dtype == np.float32 and t.tolist() == [[0, 0, 0, 3, 40, 0.25, 4, 1], [2, 2, 8, 10, 13, 0.25, 4, 1], [2, 2, 10, 12, 7, 0.5, 2, 0]]
    assert prosody_fit.resolve_fits([3], [Fit(target_frames=5, knob="pause")]).tolist() == [[0, 1, 0, 3, 5, 0, 8, 1]]
    assert prosody_fit.resolve_fits([3], [[Fit(target_frames=5)]]).tolist() == [[0, 0, 0, 3, 5, 0.25, 4, 1]]
    assert prosody_fit.segment_counts(t, 3) == [1, 0, 2]
    assert [r.shape for r in prosody_fit.split_report(np.zeros((3, 8), dtype=np.float32), [1, 0, 2])] == [(1, 8), (0, 8), (2, 8)]
    # target_seconds rounds to floor(seconds * 62.5 + 0.5)
    for sec, want in ((3.2, 200), (0.008, 1), (0.024, 2), (1.0, 63), (0.023, 1), (0.04, 3)):
        assert prosody_fit.resolve_fits([2], [Fit(target_seconds=sec)])[0, 4] == want == np.floor(sec * 62.5 + 0.5), sec
    assert prosody_fit.FIT_COLUMNS == ("target", "frames", "frames_scaled", "value", "status", "iterations", "extra_rows", "base_frames")
    assert prosody_fit.STATUS == ("EMPTY", "EXACT", "REPAIRED", "NEAREST", "CLAMPED_LOW", "CLAMPED_HIGH")
    assert [prosody_fit.STATUS.index(n) for n in prosody_fit.STATUS] == [ref.EMPTY, ref.EXACT, ref.REPAIRED, ref.NEAREST, ref.CLAMPED_LOW, ref.CLAMPED_HIGH]
    cases = [
        ([None], "one entry per utterance"),
        ([None, Fit()], "utterance 1, segment 0: give one of"),
        ([None, Fit(target_frames=5, target_seconds=1.0)], "utterance 1, segment 0: give one of"),
        ([Fit(target_frames=0), None], "utterance 0, segment 0: the target of 0 frames"),
        ([Fit(target_frames=-3), None], "utterance 0, segment 0: the target"),
        ([Fit(target_frames=2.5), None], "utterance 0, segment 0: target_frames is 2.5"),
        ([Fit(target_frames=(1 << 24) + 1), None], "utterance 0, segment 0: the target"),
        ([Fit(target_seconds=0.001), None], "utterance 0, segment 0: the target of 0 frames"),
        ([Fit(target_seconds=float("nan")), None], "utterance 0, segment 0: target_seconds"),
        ([None, Fit(5, bounds=(2.0, 1.0))], "utterance 1, segment 0: bounds"),
        ([None, Fit(5, bounds=(0.0, 1.0))], "utterance 1, segment 0: bounds"),
        ([None, Fit(5, bounds=(-0.5, 1.0), knob="pause")], "utterance 1, segment 0: bounds"),
        ([None, Fit(5, bounds=(0.5, 65.0))], "utterance 1, segment 0: bounds"),
        ([None, Fit(5, bounds=(0.5, float("inf")))], "utterance 1, segment 0: bounds"),
        ([None, Fit(5, bounds=(0.5,))], "utterance 1, segment 0: bounds"),
        ([None, Fit(5, knob="pitch")], "utterance 1, segment 0: knob"),
        ([None, [Fit(5, start=0, stop=2), Fit(5, start=2, stop=5)]], "utterance 1, segment 1: phonemes"),
        ([None, [Fit(5, start=2, stop=2)]], "utterance 1, segment 0: phonemes"),
        ([[Fit(5, start=-1, stop=2)], None], "utterance 0, segment 0: phonemes"),
        ([None, [Fit(5, start=0, stop=3), Fit(5, start=2, stop=4)]], "utterance 1, segment 1: phonemes .* overlap segment 0"),
        ([None, [Fit(5), Fit(5, start=2, stop=4)]], "utterance 1, segment 0: a whole-utterance Fit stands alone"),
        ([None, [Fit(5, start=0, stop=2, knob="pause")]], "utterance 1, segment 0: a span takes"),
        ([None, ["Fit"]], "utterance 1"),
    ]
    for fits, match in cases:
        with pytest.raises(ValueError, match=match):
            prosody_fit.resolve_fits([3, 4], fits)
    assert prosody_fit.resolve_fits([3], [Fit(5, bounds=(0.0, 64.0), knob="pause")])[0, 5:7].tolist() == [0, 64]


def test_resolved_table_feeds_the_restatement(fx):
    """The package's segment table and the restatement's agree on the columns: the fixture's segments, written as Fits."""
    begins = np.concatenate([[0], np.cumsum(fx["lengths"])])
    fits = [None] * len(fx["lengths"])
    for u, kind, b, e, target, lo, hi, exact in fx["segments"]:
        u, b0 = int(u), int(begins[int(u)])
        if kind == ref.SPAN:
            fits[u] = (fits[u] or []) + [Fit(int(target), exact=bool(exact), bounds=(lo, hi), start=int(b) - b0, stop=int(e) - b0)]
        else:
            fits[u] = Fit(int(target), knob="pause" if kind == ref.UTT_PAUSE else "duration", exact=bool(exact), bounds=(lo, hi))
    table = prosody_fit.resolve_fits(fx["lengths"], fits)
    assert np.array_equal(table, fx["segments"])
    rows, spec = prosody_fit.device_tables(table)
    assert rows.dtype == np.int32 and np.array_equal(rows, fx["segments"][:, [2, 3, 0, 1]].T) and np.array_equal(spec, fx["segments"][:, 4:])


def test_fit_header_binding_and_library_agree():
    """(v) include/toucan_prosody_fit.h, capi.FIT_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, disjoint from
    the other headers' tables; the macros are the binding's constants; the ABI version stays."""
    root = os.path.dirname(HERE)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", name), encoding="utf-8").read(), flags=re.S)
    text = strip("toucan_prosody_fit.h")
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.FIT_PROTOTYPES) == ["tts_control_and_regulate_t", "tts_copy_prosody_fit", "tts_prosody_fit", "tts_prosody_fit_apply"]
    for other in os.listdir(os.path.join(root, "include")):
        if other != "toucan_prosody_fit.h":
            assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", strip(other))), other
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "FIT_PROTOTYPES"]
    assert len(tables) >= 8 and not any(set(declared) & set(t) for t in tables)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_FIT_[A-Z_]+)\s+(\d+)", text)}
    assert macros == dict(TTS_FIT_UTT_DURATION=capi.FIT_UTT_DURATION, TTS_FIT_UTT_PAUSE=capi.FIT_UTT_PAUSE, TTS_FIT_SPAN=capi.FIT_SPAN,
                          TTS_FIT_SPEC=capi.FIT_SPEC, TTS_FIT_COLUMNS=capi.FIT_N_COLUMNS, TTS_FIT_MAX_TARGET=capi.FIT_MAX_TARGET,
                          TTS_FIT_MAX_BOUND=capi.FIT_MAX_BOUND, **{"TTS_FIT_" + n: i for i, n in enumerate(prosody_fit.STATUS)})
    assert (prosody_fit.UTT_DURATION, prosody_fit.UTT_PAUSE, prosody_fit.SPAN) == (capi.FIT_UTT_DURATION, capi.FIT_UTT_PAUSE, capi.FIT_SPAN)
    assert capi.FIT_N_COLUMNS == len(prosody_fit.FIT_COLUMNS) == len(prosody_fit.SEGMENT_COLUMNS) and prosody_fit.MAX_TARGET == capi.FIT_MAX_TARGET
    for arg_list, name in zip(re.findall(r"\bint\s+tts_[a-z0-9_]+\s*\((.*?)\)\s*;", text, flags=re.S), re.findall(r"\bint\s+(tts_[a-z0-9_]+)\s*\(", text)):
        assert len(arg_list.split(",")) == len(capi.FIT_PROTOTYPES[name][1]), name
    assert "prosody.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        assert hasattr(handle, n) and getattr(handle, n).argtypes == capi.FIT_PROTOTYPES[n][1], n
    assert handle.tts_abi_version() == 15


def test_entries_check_their_arguments_without_a_gpu():
    """tts_control_and_regulate_t / tts_copy_prosody_fit on a handle with no batch in flight, and the kernel entries' host checks:
    error codes and messages, nothing enqueued."""
    lib = capi.lib()
    assert isinstance(lib, ctypes.CDLL)
    h = ctypes.c_void_p()
    cfg = capi.TtsConfig(1, 1, 0, 0, 0, 0.0)
    assert lib.tts_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    seg = (ctypes.c_float * 8)(0, 0, 0, 1, 5, 0.25, 4, 1)
    assert lib.tts_control_and_regulate_t(h, None, None, None, 0, seg, 1, None, None) != 0 and b"tts_encoder" in lib.tts_last_error()
    out = (ctypes.c_float * 8)()
    assert lib.tts_copy_prosody_fit(h, out, None, None, None) != 0 and b"tts_control_and_regulate_t" in lib.tts_last_error()
    assert lib.tts_prosody_fit(None, 62, None, None, None, 0, None, None, None, None, 0, None, None, None, None, None, None, None, None) == 0
    assert lib.tts_prosody_fit(None, 62, None, None, None, 2, None, None, None, None, 1, None, None, None, None, None, None, None, None) != 0
    assert b"null" in lib.tts_last_error()
    assert lib.tts_prosody_fit(None, 62, None, None, None, -1, None, None, None, None, 0, None, None, None, None, None, None, None, None) != 0
    assert b"negative" in lib.tts_last_error()
    assert lib.tts_prosody_fit(None, 62, None, None, None, 0, None, None, None, None, 3, None, None, None, None, None, None, None, None) != 0
    assert lib.tts_prosody_fit_apply(None, None, 0, None) == 0
    assert lib.tts_prosody_fit_apply(None, None, 4, None) != 0 and b"null" in lib.tts_last_error()
    assert lib.tts_prosody_fit_apply(None, None, -4, None) != 0 and b"negative" in lib.tts_last_error()
    assert lib.tts_destroy(h) == 0


@pytest.fixture(scope="module")
def models_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("Models")
    interface.write_fixture_checkpoints(str(d), n_lang=20)
    return str(d)


@pytest.fixture()
def tts(monkeypatch, models_dir):
    abi_emulator.install(monkeypatch)
    monkeypatch.setattr(interface, "MODELS_DIR", models_dir)
    return interface.ToucanTTSInterface(device="cpu", tts_model_path="Meta", faster_vocoder=True)


def test_interface_validates_fits_before_anything_runs(tts):
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch([PHONES_A, PHONES_B], prosody_fit=[None, Fit(target_frames=50)], distributed=True)
    with pytest.raises(ValueError, match="one entry per utterance"):
        tts.synthesize_batch([PHONES_A, PHONES_B], prosody_fit=[None])
    with pytest.raises(ValueError, match="utterance 1, segment 0: phonemes"):
        tts.synthesize_batch([PHONES_A, PHONES_B], prosody_fit=[None, [Fit(9, start=0, stop=8)]])  # (PHONES_B has 7 phonemes)
    with pytest.raises(ValueError, match="utterance 0, segment 0: give one of"):
        tts(PHONES_A, input_is_phones=True, prosody_fit=Fit())
    with pytest.raises(ValueError, match="prosody_fit"):
        next(tts.stream(PHONES_A, input_is_phones=True, prosody_fit=Fit(40)))
    assert tts.last_prosody_fit is None and tts.last_prosody_stats is None
