"""STOI and ESTOI without a GPU: the band table against its formula, the float64 restatement (tests/intelligibility_ref.py) against
answers known in closed form or by construction, the gather form of the compacted frames against the materialised overlap-add,
header, binding and library against each other, and the additive keywords by their signatures."""
import ctypes
import inspect
import math
import os
import re

import numpy as np

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, fidelity, intelligibility, interface
from tests import intelligibility_ref as ir

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174),
         (174, 219))
N = 20000  # 2 s at 10 kHz: 155 frames, 126 segments


def header_text():
    raw = open(os.path.join(os.path.dirname(HERE), "include", "toucan_intelligibility.h"), encoding="utf-8").read()
    return re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


def test_band_table_is_the_formula_and_the_headers_constant():
    edges = [int(v) for v in re.search(r"#define\s+TTS_STOI_BAND_EDGES\s+([\d,\s]+?)\n", header_text()).group(1).split(",")]
    assert len(edges) == 16 and tuple(edges) == capi.STOI_BAND_EDGES
    from_header = tuple(zip(edges[:-1], edges[1:]))
    assert from_header == TABLE == ir.band_table() == ir.BANDS == intelligibility.band_table() == intelligibility.BANDS
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_STOI_[A-Z_]+)\s+(\d+)\s", header_text()) if k != "TTS_STOI_BAND_EDGES"}
    assert macros == {"TTS_STOI_RATE": capi.STOI_RATE, "TTS_STOI_FRAME": capi.STOI_FRAME, "TTS_STOI_HOP": capi.STOI_HOP, "TTS_STOI_BINS": capi.STOI_BINS,
                      "TTS_STOI_BANDS": capi.STOI_BANDS, "TTS_STOI_SEGMENT": capi.STOI_SEGMENT, "TTS_STOI_MAX_FRAMES": capi.STOI_MAX_FRAMES}
    assert (ir.FS, ir.N_FRAME, ir.HOP, ir.N_BINS, ir.N_BANDS, ir.SEG) == (capi.STOI_RATE, capi.STOI_FRAME, capi.STOI_HOP, capi.STOI_BINS, capi.STOI_BANDS,
                                                                         capi.STOI_SEGMENT)
    # the host tables the kernels are given are the restatement's, rounded once
    assert np.array_equal(intelligibility.window(), ir.window(np.float32)) and np.array_equal(intelligibility.dft_basis()[0], ir.basis_f32())
    w = ir.window()
    assert w.min() > 0.0 and np.allclose(w, np.hanning(258)[1:-1], rtol=0, atol=1e-15)


def test_known_answers_of_the_restatement():
    """A signal against itself and against its half scores 1 in both measures (1e-12); white noise at 20, 10, 0 and -10 dB SNR
    scores strictly less at every step; an independent signal scores below 0.1 in absolute value."""
    x = ir.speech_like(N, 1)
    for y in (x, (0.5 * x).astype(np.float32)):
        r = ir.score(x, y)
        assert r["status"] == "ok" and (r["frames"], r["kept_frames"], r["segments"]) == (155, 155, 126)
        assert abs(r["stoi"] - 1.0) < 1e-12 and abs(r["estoi"] - 1.0) < 1e-12
    ladder = [ir.score(x, ir.at_snr(x, snr, 50)) for snr in (20, 10, 0, -10)]
    print([(round(r["stoi"], 3), round(r["estoi"], 3)) for r in ladder])
    for hi, lo in zip([{"stoi": 1.0, "estoi": 1.0}] + ladder, ladder):
        assert lo["stoi"] < hi["stoi"] and lo["estoi"] < hi["estoi"]
    r = ir.score(x, ir.speech_like(N, 101))  # (its own noise and its own envelope: what is left is the chance correlation of 2 s)
    print("independent", r["stoi"], r["estoi"])
    assert abs(r["stoi"]) < 0.1 and abs(r["estoi"]) < 0.1
    assert ir.threshold_margin(x) > 26.0
    # the float32 stand-in agrees to float32 accuracy, the long double arbiter to float64 accuracy
    y = ir.at_snr(x, 10, 50)
    f64, f32 = ir.score(x, y), ir.score(x, y, np.float32)
    assert 0.0 < abs(f32["stoi"] - f64["stoi"]) < 1e-5 and 0.0 < abs(f32["estoi"] - f64["estoi"]) < 1e-5
    wide = ir.tail(*f64["bands"], np.longdouble)
    assert abs(float(wide[2]) - f64["stoi"]) < 1e-14 and abs(float(wide[3]) - f64["estoi"]) < 1e-14


def test_a_gap_of_exact_zeros_drops_its_whole_frames():
    """128 q zeros from a multiple of 128 on: the q - 1 frames that lie inside the gap are dropped, no other."""
    x = ir.speech_like(70 * 128 + 128, 4)
    assert ir.n_frames(x.size) == 70
    for first, q in ((20, 12), (0, 3), (5, 2), (40, 1)):
        g = ir.with_gap(x, first, q)
        kept = ir.kept_frames(g)
        assert len(kept) == 70 - (q - 1)
        assert sorted(set(range(70)) - set(kept.tolist())) == list(range(first, first + q - 1))
        assert ir.threshold_margin(g) > 26.0
    r = ir.score(ir.with_gap(x, 20, 12), x)
    assert r["kept_frames"] == 59 and r["segments"] == 30 and r["status"] == "ok"


def test_segment_count_and_too_short():
    x = ir.speech_like(4096, 5)
    one = ir.score(x[:3968], x[:3968])
    assert (one["frames"], one["kept_frames"], one["segments"], one["status"]) == (30, 30, 1, "ok") and abs(one["stoi"] - 1.0) < 1e-12
    short = ir.score(x[:3967], x[:3967])
    assert (short["frames"], short["segments"], short["status"]) == (29, 0, "too_short") and math.isnan(short["stoi"]) and math.isnan(short["estoi"])
    assert ir.score(x, x)["segments"] == 2
    tiny = ir.score(x[:255], x[:255])
    assert tiny["frames"] == 0 and tiny["status"] == "too_short" and math.isnan(tiny["stoi"])
    # frames enough, but too few of them left: 40 frames, 12 inside a gap
    g = ir.with_gap(ir.speech_like(41 * 128, 6), 10, 13)
    r = ir.score(g, g)
    assert (r["frames"], r["kept_frames"], r["status"]) == (40, 28, "too_short") and math.isnan(r["estoi"])
    # unequal lengths are cut to the shorter
    assert ir.score(x, x[:3968])["frames"] == 30 and ir.score(x, x[:3968])["lengths"] == (4096, 3968)
    # a NaN sample: in the generated signal the measures are NaN; in the recording nothing passes the comparison
    bad = x.copy()
    bad[2000] = np.nan
    r = ir.score(x, bad)
    assert r["status"] == "ok" and math.isnan(r["stoi"]) and math.isnan(r["estoi"])
    r = ir.score(bad, x)
    assert r["kept_frames"] == 0 and r["status"] == "too_short" and math.isnan(r["stoi"])
    # silence: every frame is kept and every d is 0 through the eps divisors
    z = np.zeros(4096, dtype=np.float32)
    r = ir.score(z, z)
    assert (r["kept_frames"], r["stoi"], r["estoi"]) == (31, 0.0, 0.0)


def test_gather_form_equals_the_materialised_overlap_add():
    """Row m from the source and the kept list alone (at most two windowed kept frames a sample) equals frame m of the overlap-add
    that is written out - exactly, in float64 and in float32: the two forms differ in nothing but which zero the sum starts from."""
    x = ir.with_gap(ir.with_gap(ir.speech_like(70 * 128 + 128, 7), 20, 12), 50, 3)
    kept = ir.kept_frames(x)
    assert len(kept) == 70 - 11 - 2
    for dtype in (np.float64, np.float32):
        comp = ir.compacted(x, kept, dtype)
        assert comp.size == 128 * (len(kept) - 1) + 256 and comp.dtype == dtype
        want = np.stack([comp[128 * m: 128 * m + 256] for m in range(len(kept))]) * ir.window(dtype)
        got = ir.gathered_rows(x, kept, dtype)
        assert got.dtype == dtype and np.array_equal(got, want)
    # the compacted signal of a signal that keeps every frame is the signal under the window's overlap sum
    y = ir.speech_like(1024, 8)
    w = ir.window()
    assert np.allclose(ir.compacted(y, np.arange(7))[128:-128], y[128:-128] * np.tile(w[:128] + w[128:], 6), rtol=0, atol=1e-12)


def test_intelligibility_header_binding_and_library_agree():
    """include/toucan_intelligibility.h, capi.INTELLIGIBILITY_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set,
    disjoint from every other table; argument counts agree; the ABI version is still 15; the entries find bad pairs and rows before
    anything touches a device, and name the pair."""
    root = os.path.dirname(HERE)
    text = header_text()
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.INTELLIGIBILITY_PROTOTYPES) == ["tts_stoi_bands", "tts_stoi_frame_energy", "tts_stoi_gather", "tts_stoi_reduce",
                                                                   "tts_stoi_segments", "tts_stoi_segments_per_group", "tts_stoi_select",
                                                                   "tts_stoi_select_sweep"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "INTELLIGIBILITY_PROTOTYPES"]
    assert len(tables) >= 14 and all(not set(declared) & set(t) for t in tables)
    for other in sorted(os.listdir(os.path.join(root, "include"))):
        if other != "toucan_intelligibility.h":
            abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", other), encoding="utf-8").read(), flags=re.S)
            assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", abi)), other
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(capi.INTELLIGIBILITY_PROTOTYPES[name][1]), name
    assert "intelligibility.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.INTELLIGIBILITY_PROTOTYPES[n][1] and fn.restype == capi.INTELLIGIBILITY_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15 == capi.ABI_VERSION
    assert handle.tts_stoi_select_sweep() == 256 and handle.tts_stoi_segments_per_group() == 32
    err = lambda: handle.tts_last_error().decode()
    pairs = np.array([[0, 5000, 5000], [10000, 14000, 4000]], dtype=np.int64)
    energy = lambda pr=pairs, n=2, total=18000, mf=38: handle.tts_stoi_frame_energy(None, total, None, pr.ctypes.data, n, None, mf, None, None)
    assert energy(total=17999) == -1 and "pair 1" in err() and "does not lie inside the wave of 17999 samples" in err()
    assert energy(mf=37) == -1 and "pair 0 has 38 frames, max_frames is 37" in err()
    assert energy(mf=0) == -1 and "max_frames 0" in err()
    assert energy() == -1 and "null pointer" in err()  # every check passed: the pointers are looked at last
    assert energy(n=0) == 0
    select = lambda n=2, mf=38: handle.tts_stoi_select(None, None, pairs.ctypes.data, n, 18000, mf, None, None, None)
    assert select(mf=30) == -1 and "pair 0 has 38 frames" in err()
    assert select() == -1 and "null pointer" in err()
    rb = np.array([[0, 38], [76, 106]], dtype=np.int64)
    gather = lambda total=136, r=rb: handle.tts_stoi_gather(None, 18000, None, pairs.ctypes.data, 2, None, 38, None, None, None, r.ctypes.data, total, None, None)
    assert gather(total=135) == -1 and "pair 1 (rows 106 .. 136) does not lie inside the 135 rows" in err()
    assert gather() == -1 and "null pointer" in err()
    frames = np.array([38, 30], dtype=np.int64)
    seg = lambda total=136, mf=38: handle.tts_stoi_segments(None, total, None, rb.ctypes.data, frames.ctypes.data, None, 2, mf, None, None)
    assert seg(total=135) == -1 and "pair 1 (rows 106 .. 136)" in err()
    assert seg(mf=37) == -1 and "pair 0 has 38 frames, max_frames is 37" in err()
    assert seg() == -1 and "null pointer" in err()
    assert handle.tts_stoi_bands(None, 513, 4, None, None) == -1 and "ld 513" in err()
    assert handle.tts_stoi_bands(None, 514, 4, None, None) == -1 and "null pointer" in err()
    assert handle.tts_stoi_bands(None, 514, 0, None, None) == 0
    assert handle.tts_stoi_reduce(None, None, 2, 0, None, None) == -1 and "max_frames 0" in err()
    assert handle.tts_stoi_reduce(None, None, 2, 38, None, None) == -1 and "null pointer" in err()
    assert handle.tts_stoi_reduce(None, None, 0, 38, None, None) == 0


def test_the_keywords_are_additive_and_default_to_off():
    for fn in (fidelity.CopySynthesis.run, fidelity.VocoderScorer.score_waves, fidelity.VocoderScorer.score,
               interface.ToucanTTSInterface.vocoder_fidelity):
        par = inspect.signature(fn).parameters
        assert "intelligibility" in par and par["intelligibility"].default is False, fn
    assert inspect.signature(fidelity.VocoderScorer.score).parameters["rank_by"].default == "mel_l1"
    par = inspect.signature(intelligibility.Intelligibility.score).parameters
    assert list(par) == ["self", "waves_a", "waves_b", "sr_a", "sr_b", "keep_segments"] and par["sr_b"].default is None and par["keep_segments"].default is False
    from Utility import Scorer
    assert Scorer.VocoderScorer is fidelity.VocoderScorer
