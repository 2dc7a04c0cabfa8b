"""The prominence meter without a GPU: the float64 restatement (tests/prominence_ref.py) against closed forms and answers worked out
by hand, its discrete decisions held to a margin, every refusal of the Python layer and of the library, header / binding / library
agreement, ``to_emphasis`` on the fixture strings and the grid keyword on a stub pipeline."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, cloner, interface, prominence, prosody
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from tests import abi_emulator, prominence_cases as cases, prominence_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
PHONES_A = "~həlˈoʊ wˈɜːld~#"
PHONES_C = "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#"
MARGIN = 1e-9  # the smallest relative gap a discrete decision of a fixture may have


def header_text():
    raw = open(os.path.join(os.path.dirname(HERE), "include", "toucan_prominence.h"), encoding="utf-8").read()
    return re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


# ---- the transform against closed forms --------------------------------------------------------------------------------------------
def test_gaussian_bump_has_its_closed_form_at_every_scale():
    """exp(-(t - c)^2 / 2 sigma^2) far from the ends: W[j, c] = C sqrt(2 pi) sigma s^(5/2) / (sigma^2 + s^2)^(3/2).  The discrete sum
    of the definition, truncation at 8 s included, agrees to 1e-12 relative for sigma >= 2 (sigma = 1 at s = 2 is off by 2.5e-6: the
    sum then under-samples the product)."""
    T, c = 4097, 2048
    t = np.arange(T, dtype=np.float64)
    for sigma in (2.0, 3.0, 8.0 / math.sqrt(5.0)):
        x = np.exp(-(t - c) ** 2 / (2.0 * sigma * sigma))
        got = np.array([pr.cwt_at(x, j, c) for j in range(6)])
        want = np.array([pr.C_PSI * math.sqrt(2.0 * math.pi) * sigma * s ** 2.5 / (sigma * sigma + s * s) ** 1.5 for s in pr.SCALES])
        rel = np.abs(got - want) / want
        print(sigma, rel.max())
        assert rel.max() <= 1e-12, (sigma, rel)
    # scale selectivity: the response over j peaks where s^2 = 5 sigma^2
    x = np.exp(-(t - c) ** 2 / (2.0 * 64.0 / 5.0))
    assert int(np.argmax([pr.cwt_at(x, j, c) for j in range(6)])) == 2 and pr.SCALES[2] == 8


def test_constant_input_leaves_the_truncation_residual():
    x = np.ones(4097)
    for j, s in enumerate(pr.SCALES):
        w = abs(pr.cwt_at(x, j, 2048))
        print(s, w)
        assert w <= 2e-12 * math.sqrt(s), (s, w)


def test_tables_of_the_module_and_of_the_restatement_are_the_same_numbers():
    table = prominence.wavelet_table()
    assert table.shape == (6, 1026) and table.dtype == np.float64 and np.array_equal(table, pr.wavelet_table())
    for j, s in enumerate(prominence.SCALES):
        assert s == 2 ** (j + 1) and np.count_nonzero(table[j, 16 * s + 1:1025]) == 0 and table[j, 1025] == s ** -0.5
        assert table[j, 8 * s] == pr.C_PSI and np.array_equal(table[j, :16 * s + 1], table[j, :16 * s + 1][::-1])
    assert [16 * s + 1 for s in prominence.SCALES] == [33, 65, 129, 257, 513, 1025]
    assert prominence.COLUMNS == pr.COLUMNS == ("prominence", "peak_frame", "mean", "pitch_part", "energy_part", "rate_part", "boundary_after",
                                                "valley_frame")


# ---- gap filling and normalisation by hand --------------------------------------------------------------------------------------------
def test_gap_filling_by_hand():
    v = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    ok = lambda *idx: np.isin(np.arange(5), idx)
    assert np.array_equal(pr.fill(v, ok(0, 1, 2, 3, 4)), v)                       # all voiced
    assert np.array_equal(pr.fill(v, ok()), np.zeros(5))                          # none voiced
    assert np.array_equal(pr.fill(v, ok(2)), np.full(5, 4.0))                     # one voiced frame: held both ways
    assert np.array_equal(pr.fill(v, ok(0, 4)), [1.0, 4.75, 8.5, 12.25, 16.0])    # voiced only at both ends: the straight line
    assert np.array_equal(pr.fill(v, ok(1, 3)), [2.0, 2.0, 5.0, 8.0, 8.0])        # held in front and behind, one frame between
    # a gap longer than a chunk of 256 frames
    T = 700
    f0 = np.zeros(T, dtype=np.float32)
    f0[100], f0[500] = 100.0, 200.0
    got = pr.channels(f0, np.ones(T, dtype=np.float32), np.zeros((0, 3)))["filled"][0]
    a, b = math.log(100.0), math.log(200.0)
    assert np.all(got[:101] == a) and np.all(got[500:] == b)
    t = np.arange(101, 500)
    assert np.array_equal(got[101:500], a + (b - a) * ((t - 100) / 400.0))
    assert got[300] == a + (b - a) * 0.5


def test_channel_values_and_normalisation():
    f0 = np.array([0, 100, 0, 200, 0], dtype=np.float32)
    e = np.array([1.0, 0.5, 1e-6, 2.0, 2.0], dtype=np.float32)
    phones = [(0, 2, 1), (2, 2, 1), (2, 4, 0), (4, 5, 1)]
    v, valid = pr.raw_values(f0, e, phones)
    assert valid[0].tolist() == [False, True, False, True, False] and valid[1].all() and valid[2].tolist() == [True, True, False, False, True]
    assert v[0, 1] == math.log(100.0) and v[1, 2] == math.log(1e-3 * 2.0) and v[1, 1] == math.log(0.5)
    assert v[2, 0] == v[2, 1] == math.log(2.0) and v[2, 4] == 0.0  # (ln 1)
    ch = pr.channels(f0, e, phones)
    for c in range(3):
        assert abs(ch["x"][c].mean()) < 1e-14 and abs(ch["x"][c].std() - 1.0) < 1e-14
    # a constant channel and T = 1 give zeros; so does a channel whose spread fp64 cannot tell from zero
    flat = pr.channels(np.full(9, 120.0, dtype=np.float32), np.full(9, 0.25, dtype=np.float32), [(0, 9, 1)])
    assert not flat["x"].any() and max(flat["std"]) < 1e-14
    one = pr.channels(np.array([120.0], dtype=np.float32), np.array([0.3], dtype=np.float32), [(0, 1, 1)])
    assert one["x"].shape == (3, 1) and not one["x"].any()
    assert not pr.znorm(np.array([1e6, 1e6 * (1 + 2 ** -52)]))[0].any()
    # an all-zero energy track keeps a finite logarithm
    assert np.isfinite(pr.channels(np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32), [])["filled"]).all()


# ---- semantics, on tracks --------------------------------------------------------------------------------------------------------------
def five_units(stressed=None, pause_after=None, seed=0):
    """Five units of 25 frames with 6 unvoiced, quieter frames between and around them; 2 % seeded jitter on both tracks so that no
    two frames tie.  stressed: the unit with an f0 bump of +30 % and energy x 1.5.  pause_after: 20 more frames behind that unit
    with invalid f0 and energy at the floor.  -> (f0, energy, phoneme table, unit table)."""
    rng = np.random.default_rng(seed)
    f0, e, phones, unit_rows, t = [], [], [], [], 0

    def stretch(n, hz, level, counts):
        nonlocal t
        f0.extend([hz] * n)
        e.extend([level] * n)
        phones.append((t, t + n, counts))
        t += n

    stretch(6, 0.0, 0.3, 0)
    for k in range(5):
        unit_rows.append((t, t + 25))
        stretch(25, 120.0 * (1.3 if k == stressed else 1.0), 1.5 if k == stressed else 1.0, 1)
        stretch(6, 0.0, 0.3, 0)
        if k == pause_after:
            stretch(20, 0.0, 1e-5, 0)
    f0 = np.asarray(f0) * (1.0 + 0.02 * rng.uniform(-1, 1, t))
    e = np.asarray(e) * (1.0 + 0.02 * rng.uniform(-1, 1, t))
    return f0.astype(np.float32), e.astype(np.float32), np.asarray(phones), np.asarray(unit_rows)


def test_the_stressed_unit_is_the_most_prominent_and_the_pause_the_strongest_boundary():
    for k in range(5):
        r = pr.measure_tracks(*five_units(stressed=k, seed=k))
        print(k, np.round(r["rows"][:, 0], 3), min(r["gaps"]))
        assert int(np.argmax(r["rows"][:, 0])) == k and min(r["gaps"]) >= MARGIN
        b, e = five_units(stressed=k)[3][k]
        assert b <= r["rows"][k, 1] < e and r["rows"][k, 3] > 0 and r["rows"][k, 4] > 0
    r = pr.measure_tracks(*five_units(pause_after=2, seed=7))
    print(np.round(r["rows"][:, 6], 3), min(r["gaps"]))
    assert int(np.nanargmax(r["rows"][:, 6])) == 2 and math.isnan(r["rows"][4, 6]) and r["rows"][4, 7] == -1 and min(r["gaps"]) >= MARGIN
    lo, hi = five_units(pause_after=2)[3][2][1], five_units(pause_after=2)[3][3][0]
    assert lo <= r["rows"][2, 7] < hi  # the valley lies in the pause


def test_units_first_index_rule_empty_units_and_gaps():
    P = np.array([0.0, 3.0, 3.0, 1.0, -2.0, -2.0, 5.0, 4.0])
    parts = np.stack([P * 0.5, P * 0.25, P * 0.25])
    rows, gaps = pr.units(P, parts, [(0, 4), (4, 4), (5, 8)])
    assert rows[0, :3].tolist() == [3.0, 1.0, 1.75] and rows[0, 3:6].tolist() == [1.5, 0.75, 0.75] and rows[0, 6:].tolist() == [2.0, 4.0]
    assert np.isnan(rows[1, [0, 2, 3, 4, 5, 6]]).all() and rows[1, 1] == rows[1, 7] == -1
    assert rows[2, :2].tolist() == [5.0, 6.0] and math.isnan(rows[2, 6]) and rows[2, 7] == -1
    assert gaps == [0.0, 0.2, 0.0]  # two ties and (5 - 4) / max |P|: a fixture like this one fails the margin
    assert pr.units(P, parts, [(1, 2)])[1] == [math.inf]


def test_every_decision_of_the_seeded_batch_has_its_margin():
    """The ragged batch the GPU tests compare on (tests/prominence_cases.py): every peak and every valley of the restatement is at
    least 1e-9 of max |P| away from the runner-up, so the kernels' rounding (1e-13 at most) cannot move a decision.  No case is
    excused: a fixture that loses its margin fails here."""
    for u, (case, ref) in enumerate(zip(cases.batch(), cases.restated())):
        T, units = len(case[0]), case[3]
        assert T == cases.FRAMES[u] and len(ref["gaps"]) >= (1 if T > 1 else 0)
        prominence.check_tracks([case[0]], [case[1]], [case[2]], [units])  # the tables are ones the entries accept
        print(T, len(units), min(ref["gaps"], default=math.inf))
        assert min(ref["gaps"], default=math.inf) >= MARGIN, (u, sorted(ref["gaps"])[:3])
    assert not cases.batch()[cases.UNVOICED][0].any() and cases.batch()[7][3].tolist().count([262, 262]) == 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_python_layer():
    f0, e = [np.full(10, 100.0)], [np.ones(10)]
    ok_ph, ok_un = [[(0, 10, 1)]], [[(0, 5), (5, 10)]]
    assert prominence.check_tracks(f0, e, ok_ph, ok_un)[0] == [10]
    with pytest.raises(ValueError, match="utterance 0, unit 1 begins at frame 4, before the end of the one in front of it"):
        prominence.check_tracks(f0, e, ok_ph, [[(0, 5), (4, 10)]])
    with pytest.raises(ValueError, match=r"utterance 0, unit 1 is frames \[5, 11\), the utterance has 10"):
        prominence.check_tracks(f0, e, ok_ph, [[(0, 5), (5, 11)]])
    with pytest.raises(ValueError, match=r"utterance 0, phoneme 0 is frames \[3, 2\)"):
        prominence.check_tracks(f0, e, [[(3, 2, 1)]], ok_un)
    with pytest.raises(ValueError, match="utterance 1: 3 f0 values for 4 energy values"):
        prominence.check_tracks(f0 + [np.ones(3)], e + [np.ones(4)], ok_ph * 2, ok_un * 2)
    with pytest.raises(ValueError, match="past the cap of 65536"):
        prominence.check_tracks([np.ones(65537)], [np.ones(65537)], [[]], [[]])
    with pytest.raises(ValueError, match="no frames"):
        prominence.check_tracks([np.ones(0)], [np.ones(0)], [[]], [[]])
    with pytest.raises(ValueError, match="one of each per utterance"):
        prominence.check_tracks(f0, e, ok_ph, [])
    with pytest.raises(ValueError, match="the rate weight is -0.5"):
        prominence.check_weights((1.0, 1.0, -0.5))
    with pytest.raises(ValueError, match="the pitch weight is nan"):
        prominence.check_weights((math.nan, 1.0, 0.5))
    with pytest.raises(ValueError, match="the energy weight is inf"):
        prominence.check_weights((1.0, math.inf, 0.5))
    for band in ((-1, 3), (1, 6), (3, 1), (0.5, 2)):
        with pytest.raises(ValueError, match="outside 0 .. 5"):
            prominence.check_band(band)
    assert prominence.check_band((0, 5)) == (0, 5) and prominence.check_weights((0, 0, 0)) == (0.0, 0.0, 0.0)
    assert prominence.MAX_FRAMES == 65536
    with pytest.raises(ValueError, match="a duration is negative"):
        prominence.duration_frames([3, -1], 10)
    assert prominence.duration_frames([3, 4, 5], 10).tolist() == [0, 3, 7, 10]


def test_header_binding_and_library_agree_and_the_library_refuses():
    """include/toucan_prominence.h, capi.PROMINENCE_PROTOTYPES and the exports are one set, disjoint from every other table; argument
    counts agree; the ABI version is still 15; every entry finds a bad table on the host, before a pointer is looked at, and names
    the utterance and the unit."""
    root = os.path.dirname(HERE)
    text = header_text()
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.PROMINENCE_PROTOTYPES) == ["tts_prominence_channels", "tts_prominence_cwt", "tts_prominence_max_frames",
                                                              "tts_prominence_units"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "PROMINENCE_PROTOTYPES"]
    assert len(tables) >= 15 and all(not set(declared) & set(t) for t in tables)
    for other in sorted(os.listdir(os.path.join(root, "include"))):
        if other != "toucan_prominence.h":
            abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", other), encoding="utf-8").read(), flags=re.S)
            assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", abi)), other
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert (0 if args.strip() == "void" else len(args.split(","))) == len(capi.PROMINENCE_PROTOTYPES[name][1]), name
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_PROMINENCE_[A-Z_]+)\s+(\d+)\s", text)}
    assert macros == {"TTS_PROMINENCE_MAX_FRAMES": capi.PROMINENCE_MAX_FRAMES, "TTS_PROMINENCE_CHANNELS": capi.PROMINENCE_CHANNELS,
                      "TTS_PROMINENCE_SCALES": capi.PROMINENCE_SCALES, "TTS_PROMINENCE_MAX_TAPS": capi.PROMINENCE_MAX_TAPS,
                      "TTS_PROMINENCE_TABLE_LD": capi.PROMINENCE_TABLE_LD, "TTS_PROMINENCE_COLUMNS": capi.PROMINENCE_N_COLUMNS,
                      "TTS_PROMINENCE_UTT_COLUMNS": capi.PROMINENCE_UTT_COLUMNS, "TTS_PROMINENCE_TILE": capi.PROMINENCE_TILE}
    assert len(prominence.COLUMNS) == capi.PROMINENCE_N_COLUMNS
    assert "prominence.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.PROMINENCE_PROTOTYPES[n][1] and fn.restype == capi.PROMINENCE_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15 == capi.ABI_VERSION
    assert handle.tts_prominence_max_frames() == 65536
    err = lambda: handle.tts_last_error().decode()
    utts = np.array([[0, 10, 0, 1, 0, 2], [10, 7, 1, 2, 2, 1]], dtype=np.int64)
    phones = np.array([[0, 10, 1], [0, 3, 1], [3, 7, 0]], dtype=np.int32)
    units = np.array([[0, 5], [5, 10], [2, 7]], dtype=np.int32)

    def channels(u=utts, ph=phones, total=17, n=2):
        return handle.tts_prominence_channels(None, None, total, None, u.ctypes.data, n, None, ph.ctypes.data, len(ph), None, None)

    def with_row(table, row, values):
        t = table.copy()
        t[row] = values
        return t

    assert channels(total=16) == -1 and "utterance 1 (frames 10 .. 17) does not lie inside the 16 frames" in err()
    assert channels(u=with_row(utts, 0, [0, 65537, 0, 1, 0, 2]), total=70000) == -1 and "utterance 0 has 65537 frames, an utterance has 1 .. 65536" in err()
    assert channels(u=with_row(utts, 1, [10, 0, 1, 2, 2, 1])) == -1 and "utterance 1 has 0 frames" in err()
    assert channels(u=with_row(utts, 1, [10, 7, 2, 2, 2, 1])) == -1 and "utterance 1 (phoneme rows 2 .. 4) does not lie inside the 3 rows" in err()
    assert channels(ph=with_row(phones, 2, [2, 7, 0])) == -1 and "utterance 1, phoneme 1 begins at frame 2, before the end of the one in front of it (3)" in err()
    assert channels(ph=with_row(phones, 2, [3, 8, 0])) == -1 and "utterance 1, phoneme 1 is frames [3, 8), the utterance has 7" in err()
    assert channels() == -1 and "null pointer" in err()  # every check passed: the pointers are looked at last
    assert channels(n=0) == 0
    cwt = lambda total=17: handle.tts_prominence_cwt(None, total, None, utts.ctypes.data, 2, None, None, None)
    assert cwt(16) == -1 and "utterance 1" in err() and cwt() == -1 and "null pointer" in err()

    def rows(un=units, w=(1.0, 1.0, 0.5), band=(1, 3), u=utts):
        return handle.tts_prominence_units(None, 17, None, u.ctypes.data, 2, None, un.ctypes.data, len(un), w[0], w[1], w[2], band[0], band[1], None, None, None)

    assert rows(un=with_row(units, 1, [4, 10])) == -1 and "utterance 0, unit 1 begins at frame 4, before the end of the one in front of it (5)" in err()
    assert rows(un=with_row(units, 2, [2, 8])) == -1 and "utterance 1, unit 0 is frames [2, 8), the utterance has 7" in err()
    assert rows(u=with_row(utts, 1, [10, 7, 1, 2, 2, 2])) == -1 and "utterance 1 (unit rows 2 .. 4) does not lie inside the 3 rows" in err()
    assert rows(w=(1.0, -1.0, 0.5)) == -1 and "the energy weight is -1" in err()
    assert rows(w=(math.nan, 1.0, 0.5)) == -1 and "the pitch weight" in err()
    assert rows(w=(1.0, 1.0, math.inf)) == -1 and "the rate weight" in err()
    for band in ((-1, 3), (1, 6), (3, 1)):
        assert rows(band=band) == -1 and "is outside 0 .. 5" in err()
    assert rows() == -1 and "null pointer" in err()


# ---- wiring ----------------------------------------------------------------------------------------------------------------------------
def test_to_emphasis_on_the_fixture_strings():
    feats = phones_to_features(PHONES_C)
    words = prosody.word_spans(feats)
    assert len(words) == 4
    report = np.full((4, 8), math.nan)
    report[:, 0] = [0.5, 2.0, math.nan, 2.0]
    spans = prominence.to_emphasis(feats, report)
    assert len(spans) == 1 and (spans[0].start, spans[0].stop) == words[1] and spans[0].values() == (1.2, 1.3, 1.2, 0.0, 0.0)  # a tie: the earlier word
    spans = prominence.to_emphasis(feats, report, n=3, pitch=1.5, duration=1.0)
    assert [(s.start, s.stop) for s in spans] == [words[0], words[1], words[3]] and all(s.pitch == 1.5 and s.duration == 1.0 for s in spans)
    assert len(prominence.to_emphasis(feats, report, n=4)) == 3 and prominence.to_emphasis(feats, report, n=0) == []  # the word without frames is never chosen
    assert prosody.resolve_curves([feats.shape[0]], [spans]) is not None  # ready for prosody_curves=
    with pytest.raises(ValueError, match="3 rows, the text has 4 words"):
        prominence.to_emphasis(feats, report[:3])
    with pytest.raises(ValueError, match="count of words"):
        prominence.to_emphasis(feats, report, n=-1)
    # the words in frames, through clipped durations
    feats_a = phones_to_features(PHONES_A)
    cum = prominence.duration_frames(np.full(feats_a.shape[0], 3), 30)
    assert cum[-1] == 30 and cum[5] == 15
    table = prominence.phoneme_table(feats_a, cum)
    assert table.shape == (feats_a.shape[0], 3) and np.array_equal(table[:, 2] != 0, np.asarray(feats_a)[:, prosody.F_PHONEME] != 0)
    assert [tuple(r) for r in prominence.word_units(feats_a, cum)] == [(min(3 * a, 30), min(3 * b, 30)) for a, b in prosody.word_spans(feats_a)]


def test_the_keywords_are_additive_and_default_to_off():
    par = inspect.signature(interface.ToucanTTSInterface.synthesize_grid).parameters
    assert par["word_prominence"].default is False and list(par)[-1] == "word_prominence"
    for fn in (interface.ToucanTTSInterface.stream, interface.ToucanTTSInterface.read_to_file, interface.ToucanTTSInterface.synthesize_batch):
        assert "word_prominence" not in inspect.signature(fn).parameters
    par = inspect.signature(interface.ToucanTTSInterface.word_prominence).parameters
    assert list(par)[:3] == ["self", "texts", "input_is_phones"] and par["input_is_phones"].default is True
    assert list(inspect.signature(cloner.UtteranceCloner.word_prominence).parameters)[:4] == ["self", "transcript", "path", "speech_bounds"]
    par = inspect.signature(prominence.ProminenceMeter.measure_tracks).parameters
    assert list(par) == ["self", "f0", "energy", "phoneme_frames", "units", "weights", "band", "return_scalogram"]
    assert par["weights"].default == (1.0, 1.0, 0.5) and par["band"].default == (1, 3) and par["return_scalogram"].default is False
    par = inspect.signature(prominence.ProminenceMeter.measure).parameters
    assert list(par)[:5] == ["self", "waves", "sr", "feats", "durations"] and par["durations"].default is None


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


class StubPipe:
    """Stands in for native.NativePipeline.forward: variant k (counted over all calls) is 768 samples of the value k, with durations
    k + 1 on every phoneme."""

    def __init__(self):
        self.seen = 0

    def forward(self, phones, emb, lang_ids, z_noise=None, durations=None, pitch=None, energy=None, prosody_curves=None, **kw):
        n = len(phones)
        table = prosody.resolve_scales(n, **kw)
        table = np.ones((n, 4), dtype=np.float32) if table is None else table  # (all scalars: synthesize_batch)
        wav = torch.cat([torch.full((768,), float(self.seen + i)) for i in range(n)])
        durs = [torch.full((int(p.shape[0]),), self.seen + i + 1, dtype=torch.int32) for i, p in enumerate(phones)]
        self.seen += n
        stats = np.concatenate([table, np.zeros((n, 4), dtype=np.float32)], axis=1)
        per = [torch.zeros(1)] * n
        out = dict(wav=wav, wav_spans=[(768 * i, 768) for i in range(n)], durations=durs, pitch=per, energy=per, mel=per, prosody_stats=(stats, stats))
        resolved = prosody.resolve_curves([int(p.shape[0]) for p in phones], prosody_curves)
        if resolved is not None:
            local = np.zeros((len(resolved[1]), 8), dtype=np.float32)
            out["prosody_span_stats"] = prosody.split_span_stats((local, local), resolved[2])
        return out


class StubMeter:
    """Stands in for prominence.ProminenceMeter: the report of a variant holds its wave's first sample and its first duration."""

    def __init__(self):
        self.calls = []

    def measure(self, waves, sr, feats, durations=None, **kw):
        self.calls.append(dict(n=len(waves), sr=sr, kw=kw))
        assert len(feats) == len(durations) == len(waves) and all(len(d) == f.shape[0] for d, f in zip(durations, feats))
        return [np.array([[float(w[0]), float(d[0])]]) for w, d in zip(waves, durations)]


def test_grid_keyword_on_a_stub_pipeline(tts):
    feats = phones_to_features(PHONES_A)
    curves = [prosody.emphasis(feats, [k]) for k in range(len(prosody.word_spans(feats)))]
    tts.pipe, tts._prominence_obj = StubPipe(), StubMeter()
    res = tts.synthesize_grid(PHONES_A, (0.9, 1.1), curves=curves, word_prominence=True)
    assert len(res) == 4 and [r["curve"] for r in res] == [0, 0, 1, 1]
    assert [r["prominence"].tolist() for r in res] == [[[float(k), float(k + 1)]] for k in range(4)]  # its own wave, its own durations
    assert tts._prominence_obj.calls == [dict(n=4, sr=24000, kw={})]
    # more than one chunk: every chunk is measured with the durations of its own synthesis
    tts.pipe, tts._prominence_obj = StubPipe(), StubMeter()
    res = tts.synthesize_grid(PHONES_A, tuple(1.0 + 0.01 * k for k in range(40)), word_prominence=True)
    assert [c["n"] for c in tts._prominence_obj.calls] == [32, 8] and [r["prominence"][0, 1] for r in res] == [float(k + 1) for k in range(40)]
    # without the keyword the dicts are what they were and the meter is never asked
    tts.pipe, tts._prominence_obj = StubPipe(), StubMeter()
    res = tts.synthesize_grid(PHONES_A, (0.9, 1.1))
    assert all(set(r) == {"scales", "wave", "frames", "stats_before", "stats_after"} for r in res) and tts._prominence_obj.calls == []


def test_word_prominence_refuses_what_check_pronunciation_refuses(tts):
    for kw, word in ((dict(distributed=True), "distributed"), (dict(sample_rate=16000), "sample_rate"), (dict(pcm16=True), "pcm16"),
                     (dict(loudness=-23.0), "loudness"), (dict(speech_level=-26.0), "speech_level")):
        with pytest.raises(ValueError, match=word):
            tts.word_prominence([PHONES_A], **kw)
    with pytest.raises(ValueError, match="rate weight"):
        tts.word_prominence([PHONES_A], weights=(1.0, 1.0, -1.0))
    with pytest.raises(ValueError, match="outside 0 .. 5"):
        tts.word_prominence([PHONES_A], band=(2, 9))
    tts.pipe, tts._prominence_obj = StubPipe(), StubMeter()
    res = tts.word_prominence([PHONES_A, PHONES_C], keep_waves=True)
    assert [r["report"].tolist() for r in res] == [[[0.0, 1.0]], [[1.0, 2.0]]] and [len(r["words"]) for r in res] == [2, 4]
    assert all(r["synth"].shape == (768,) for r in res) and res[1]["durations"].tolist() == [2] * phones_to_features(PHONES_C).shape[0]
