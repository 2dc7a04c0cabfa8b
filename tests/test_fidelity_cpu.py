"""The spectral distances without a GPU: the float64 restatement (tests/fidelity_ref.py) against the reference's stored values and
against answers known in closed form, the host side of fidelity.py (filterbank runs, DFT basis, the copy-synthesis plan, the
scorer's bookkeeping), and header, binding and library against each other."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, fidelity, resample, style
from tests import fidelity_ref as fr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fidelity", "mel_loss.npz")


def noise(n, seed):
    return fr.golden_wave(n, seed)


def test_restatement_reproduces_the_reference_golden():
    """Every stored loss of the reference's MelSpectrogramLoss within one float32 ulp of a logarithm of magnitude 1 (1.2e-7: the
    reference computes in float32), the stored log-mel frames within the float32 error of a 1536-term sum; the cases are the ones
    tests/golden/make_fidelity_golden.py ran."""
    g = np.load(GOLDEN)
    cases = fr.golden_cases()
    assert [(int(n), str(k), int(s)) for n, k, s in zip(g["lengths"], g["kinds"], g["seeds"])] == cases
    assert tuple(g["kept_frames"]) == (0, 1, -2, -1) and g["log_mel"].shape == (len(cases), 4, fr.N_MELS)
    for i, (n, kind, seed) in enumerate(cases):
        a, b = fr.golden_pair(n, kind, seed)
        d = fr.distance(a, b, resolutions=((fr.N_REF, fr.HOP_REF),))
        assert abs(d["mel_l1"] - g["mel_loss"][i]) <= 1.2e-7, (n, kind)
        assert d["frame_mel_l1"].shape == (1 + n // 384,) and abs(d["frame_mel_l1"].mean() - d["mel_l1"]) < 1e-15
        lm = fr.log_mel(b)[[0, 1, -2, -1]]
        # log10 of a float32 sum of 1536 products: relative error of the amplitude a few sqrt(1536) 2^-24 = 2e-6, 1e-6 in log10
        assert np.abs(lm - g["log_mel"][i]).max() <= 2e-5, (n, kind, np.abs(lm - g["log_mel"][i]).max())


@pytest.mark.parametrize("n", [769, 5000])
def test_known_answers_of_a_scaled_pair(n):
    """generated = recording / 2 on noise (no clamp is reached): mel_l1 = log10 2 and log_magnitude_l1 = ln 2 at every resolution
    that admits the length; the spectral convergence, whose denominator is the RECORDING, is 1/2 - and 1 with the two swapped
    (generated = 2 x recording), the value the issue quotes."""
    b = noise(n, 7)
    a = (0.5 * b).astype(np.float32)  # exact in float32
    res = [r for r in fr.RESOLUTIONS if n > r[0] // 2]
    for gen, rec, sc in ((a, b, 0.5), (b, a, 1.0)):
        d = fr.distance(gen, rec, res)
        assert abs(d["mel_l1"] - math.log10(2.0)) < 1e-12
        assert np.abs(d["frame_mel_l1"] - math.log10(2.0)).max() < 1e-12
        for r in res:
            assert abs(d[r]["spectral_convergence"] - sc) < 1e-12
            assert abs(d[r]["log_magnitude_l1"] - math.log(2.0)) < 1e-12
    # the float32 stand-in (DFT as a float32 matrix product, float32 tail) agrees to float32 accuracy: it is what sets the GPU tolerances
    s = fr.distance(a, b, res, f32=True)
    assert abs(s["mel_l1"] - math.log10(2.0)) < 1e-5


def test_identical_signals_and_silence_give_exact_zeros():
    x = noise(5000, 3)
    z = np.zeros(5000, dtype=np.float32)
    for a, b in ((x, x), (z, z)):
        d = fr.distance(a, b)
        assert d["mel_l1"] == 0.0 and not d["frame_mel_l1"].any()
        for r in fr.RESOLUTIONS:
            assert d[r]["spectral_convergence"] == 0.0 and d[r]["log_magnitude_l1"] == 0.0
    # silence: every amplitude is the clamp's 1e-5, the denominator sqrt(frames bins 1e-10) > 0
    sums = fr.frame_sums(fr.spectrum(z, 1536), fr.spectrum(z, 1536), fr.mel_matrix())
    assert np.allclose(sums[:, 2], 769 * 1e-10, rtol=1e-12) and np.isfinite(fr.measures(sums, 769)["spectral_convergence"])
    # silence against noise: both clamps on one side only, everything finite
    d = fr.distance(z, x, ((1536, 384),))
    assert np.isfinite(d["mel_l1"]) and d["mel_l1"] > 1.0 and np.isfinite(d[(1536, 384)]["log_magnitude_l1"])


def test_band_runs_equal_the_dense_filterbank():
    mel = fr.mel_matrix()
    assert mel.shape == (100, 769) and mel.dtype == np.float32
    bands, weights = fidelity.band_runs(mel)
    assert bands.dtype == np.int32 and bands.shape == (100, 2) and weights.dtype == np.float32 and weights.size == bands[:, 1].sum()
    assert bands[:, 1].min() >= 4 and bands[:, 1].max() <= 50 and weights.size <= 4096 and (weights > 0).all()
    dense, at = np.zeros_like(mel), 0
    for m, (first, count) in enumerate(bands):
        dense[m, first: first + count] = weights[at: at + count]
        at += count
    assert np.array_equal(dense, mel)
    amp = np.abs(noise(769, 11)).astype(np.float64)
    runs = np.array([weights[o: o + c].astype(np.float64) @ amp[f: f + c] for (f, c), o in zip(bands, np.cumsum(bands[:, 1]) - bands[:, 1])])
    assert np.allclose(runs, mel.astype(np.float64) @ amp, rtol=1e-13, atol=0)
    gap = mel.copy()
    gap[5, bands[5, 0] + 1] = 0.0
    with pytest.raises(ValueError, match="band 5"):
        fidelity.band_runs(gap)
    assert fidelity.DEFAULT_RESOLUTIONS == fr.RESOLUTIONS and fidelity.REFERENCE_RESOLUTION == (fr.N_REF, fr.HOP_REF)
    assert (fidelity.SR, fidelity.N_MELS, fidelity.FMIN, fidelity.FMAX) == (fr.SR, fr.N_MELS, fr.FMIN, fr.FMAX)


def test_dft_basis_is_the_windowed_dft_in_four_rows():
    for n_fft, hop in fr.RESOLUTIONS:
        w = fidelity.dft_basis(n_fft)
        assert w.shape == (4, hop, n_fft + 2) and w.dtype == np.float32
        assert np.array_equal(w.reshape(n_fft, -1), fr.basis(n_fft).astype(np.float32))
    x = noise(5000, 5)
    re, im = fr.spectrum(x, 768)
    z = fr.frames(x, 768) @ fr.basis(768)
    assert np.abs(z[:, :385] - re).max() < 1e-10 and np.abs(z[:, 385:] - im).max() < 1e-10
    for bad in ((1536, 383), (1536, 512), (770, 192.5), (8192, 2048), (24, 6)):
        with pytest.raises(ValueError, match="resolution"):
            fidelity.check_resolution(*bad)


def test_framing_counts_and_the_copy_synthesis_plan():
    """Frames and rows of the centred STFT; the cut of the copy-synthesis: 384 F and 384 F + 1 samples both give F frames, 384 F
    samples at 24 kHz, 256 F at 16 kHz, whose front end has F + 1 frames."""
    for n, hop in ((769, 384), (1152, 384), (1153, 384), (5000, 384), (5000, 192), (6145, 768)):
        F = fidelity.frame_count(n, hop)
        assert F == 1 + n // hop == fr.frames(np.zeros(n), 4 * hop).shape[0]
        buf = fr.row_buffer(noise(n, 1), hop)
        assert buf.shape == (fidelity.padded_rows(n, hop), hop) and fidelity.padded_rows(n, hop) >= F + 3
        assert not buf.reshape(-1)[n + 4 * hop:].any()
    for F in (5, 6, 27):
        for n in (384 * F, 384 * F + 1, 384 * F + 383):
            assert fidelity.copy_synthesis_plan(n) == (F, 384 * F, 256 * F)
        assert resample.out_length(384 * F, 24000, 16000) == 256 * F
        assert fidelity.frame_count(256 * F, style.HOP) == F + 1
    assert fidelity.copy_synthesis_plan(384 * 3, ((1536, 384),))[0] == 3
    with pytest.raises(ValueError, match="needs more than 1536"):
        fidelity.copy_synthesis_plan(384 * 4)  # 1536 samples: not longer than half of 3072
    with pytest.raises(ValueError, match="needs more than 768"):
        fidelity.copy_synthesis_plan(384 * 2 + 100, ((1536, 384),))


def test_a_signal_of_half_a_window_raises():
    for n_fft in (768, 1536, 3072):
        with pytest.raises(ValueError, match=f"needs more than {n_fft // 2}"):
            fidelity.check_length(n_fft // 2, n_fft)
        fidelity.check_length(n_fft // 2 + 1, n_fft)
        with pytest.raises(ValueError):
            fr.padded(np.zeros(n_fft // 2), n_fft)
        assert fr.padded(np.zeros(n_fft // 2 + 1), n_fft).size == n_fft // 2 + 1 + n_fft


def test_score_book_lists_and_removes_like_the_corpus_scorers(capsys):
    """Scripted scores: the listing is sorted, NaNs are always shown; removal takes the NaNs and the n worst, a NaN that is also
    among the worst once (INTEGRATION.md's deviation row); a second removal is refused until the scoring is run again."""
    book = fidelity.ScoreBook()
    book.remove_samples_with_highest_loss(1)
    assert "Please run the scoring first." in capsys.readouterr().out
    keys = ["a.wav", "b.wav", "c.wav", "d.wav", "e.wav"]
    book.record_scores(keys, [0.2, float("nan"), 0.9, 0.1, 0.5], records=[{"k": k} for k in keys])
    out = capsys.readouterr().out
    assert "NaNs detected during scoring!" in out and "b.wav" in out
    assert book.nans == ["b.wav"] and book.nan_indexes == [1] and book.path_to_id["e.wav"] == 4 and book.path_to_record["c.wav"] == {"k": "c.wav"}
    assert math.isnan(book.path_to_score["b.wav"]) and book.path_to_score["c.wav"] == 0.9
    book.show_samples_with_highest_loss(2)
    out = capsys.readouterr().out
    assert "The following filepaths had an infinite loss:" in out and out.count("Loss:") == 2
    book.show_samples_with_highest_loss()
    assert capsys.readouterr().out.count("Loss:") == 5
    # sorted() by score, descending, leaves the NaN where it stood - first, here: it is "among the worst 2" and listed as a NaN too
    worst = sorted(book.path_to_score, key=book.path_to_score.get, reverse=True)[:2]
    book.remove_samples_with_highest_loss(2)
    left = [k for k in keys if k not in set(worst) | {"b.wav"}]
    assert book.current_dset.datapoints == left and len(book.current_dset) == len(left) and book.nans_removed
    before = list(book.current_dset.datapoints)
    book.remove_samples_with_highest_loss(1)
    assert "Indexes are no longer accurate" in capsys.readouterr().out and book.current_dset.datapoints == before
    book.record_scores(["x", "y"], [1.0, 2.0])
    assert not book.nans and not book.nans_removed and book.current_dset.datapoints == ["x", "y"]
    book.remove_samples_with_highest_loss(1)
    assert book.current_dset.datapoints == ["x"]
    from Utility import Scorer
    assert Scorer.VocoderScorer is fidelity.VocoderScorer and issubclass(fidelity.VocoderScorer, fidelity.ScoreBook)
    with pytest.raises(capi.ToucanHipError):
        fidelity.SpectralDistance("cpu")


def test_fidelity_header_binding_and_library_agree():
    """include/toucan_fidelity.h, capi.FIDELITY_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set, disjoint from
    every other table and from toucan_tts.h, with the constants the binding mirrors; the entries find bad spans, rows, pairs and
    bands before anything touches a device, and name the utterance or pair."""
    root = os.path.dirname(HERE)
    raw = open(os.path.join(root, "include", "toucan_fidelity.h"), encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.FIDELITY_PROTOTYPES) == ["tts_frame_reflect", "tts_spectral_distance", "tts_spectral_frames_per_group",
                                                            "tts_spectral_reduce", "tts_spectral_reduce_sweep"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "FIDELITY_PROTOTYPES"]
    assert len(tables) >= 13 and all(not set(declared) & set(t) for t in tables)
    for other in ("toucan_tts.h", "toucan_truepeak.h", "toucan_compare.h"):
        abi = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", other), encoding="utf-8").read(), flags=re.S)
        assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", abi))
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TTS_FIDELITY_SUMS": capi.FIDELITY_SUMS, "TTS_FIDELITY_MAX_BINS": capi.FIDELITY_MAX_BINS,
                      "TTS_FIDELITY_MAX_BANDS": capi.FIDELITY_MAX_BANDS, "TTS_FIDELITY_MAX_HOP": capi.FIDELITY_MAX_HOP}
    assert len(fidelity.SUM_COLUMNS) == capi.FIDELITY_SUMS and fidelity.SUM_COLUMNS == fr.SUMS
    for name in declared:
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        n_args = 0 if args.strip() == "void" else len(args.split(","))
        assert n_args == len(capi.FIDELITY_PROTOTYPES[name][1]), name
    assert "fidelity.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.FIDELITY_PROTOTYPES[n][1] and fn.restype == capi.FIDELITY_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15
    assert handle.tts_spectral_frames_per_group() == 4 and handle.tts_spectral_reduce_sweep() == 256
    err = lambda: handle.tts_last_error().decode()
    spans = np.array([[0, 900], [900, 769], [1669, 768]], dtype=np.int64)
    rb = np.array([0, 7, 14], dtype=np.int64)
    frame = lambda sp=spans, b=3, n=2437, mc=900, hop=384, r=rb, total=20: handle.tts_frame_reflect(None, n, None, sp.ctypes.data, b, mc, hop, None,
                                                                                                  r.ctypes.data, total, None, None)
    assert frame() == -1 and "utterance 2 has 768 samples" in err()
    assert frame(b=2, n=1000) == -1 and "utterance 1" in err() and "does not lie inside the wave" in err()
    assert frame(b=2, total=13) == -1 and "utterance 1 (rows 7 .. 14) does not lie inside the 13 rows" in err()
    assert frame(b=2, mc=800) == -1 and "max_count" in err()
    assert frame(b=2, hop=190) == -1 and "hop 190" in err()
    assert frame(b=2, hop=8192) == -1 and "hop 8192" in err()
    assert frame(b=2) == -1 and "null pointer" in err()  # every check passed: the pointers are looked at last
    assert frame(b=0) == 0
    pairs = np.array([[0, 10, 5], [20, 30, 9]], dtype=np.int64)
    bands = np.array([[0, 4], [3, 5]], dtype=np.int32)
    dist = lambda ld=1538, bins=769, rows=40, pr=pairs, n=2, mf=9, bd=bands, nb=2, nw=9: handle.tts_spectral_distance(
        None, ld, bins, rows, None, pr.ctypes.data, n, mf, None, bd.ctypes.data if bd is not None else None, nb, None, nw, None, None)
    assert dist(rows=38) == -1 and "pair 1 (rows 20 and 30, 9 frames) does not lie inside the spectrum of 38 rows" in err()
    assert dist(mf=8) == -1 and "pair 1 has 9 frames, max_frames is 8" in err()
    assert dist(bins=2050, ld=4100) == -1 and "bins 2050" in err()
    assert dist(ld=1537) == -1 and "ld 1537" in err()
    assert dist(nw=8) == -1 and "the bands hold 9 weights, n_weights is 8" in err()
    assert dist(bins=7, ld=14) == -1 and "band 1 (bins 3 .. 8) does not lie inside the 7 bins" in err()
    assert dist(nb=257) == -1 and "n_bands 257" in err()
    assert dist() == -1 and "null pointer" in err()
    assert dist(n=0) == 0
    red = lambda n=2, mf=9: handle.tts_spectral_reduce(None, None, n, mf, None, None)
    assert red(mf=0) == -1 and "max_frames 0" in err()
    assert red() == -1 and "null pointer" in err()
    assert red(n=0) == 0
