"""The prominence meter's kernels (csrc/prominence.hip) on the MI355X against the float64 restatement in tests/prominence_ref.py, on
the ragged batch of tests/prominence_cases.py: the channels and the transform within their rounding bounds, the discrete decisions
exactly, every utterance alone with the bits it has in the batch, a waveform end to end, and the interface."""
import math

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import interface, prominence, prosody
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from tests import pitch_ref, prominence_cases as cases, prominence_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
WEIGHTS, BAND = (1.0, 1.0, 0.5), (1, 3)


@pytest.fixture(scope="module")
def meter():
    return prominence.ProminenceMeter(DEV)


@pytest.fixture(scope="module")
def measured(meter):
    """The batch through ``measure_tracks`` once: (reports, scalograms)."""
    f0, e, ph, un = zip(*cases.batch())
    return meter.measure_tracks(list(f0), list(e), list(ph), list(un), return_scalogram=True)


def channel_bound(ref, c):
    """Per frame, what x of channel c may differ by.  With n frames, v the gap-filled values, S = sum |v|, V = max |v|, sd their spread
    and u = 2^-53: the mean is a sum of n terms in another order than the restatement's, off by at most (n + 6) u S / n (the rounding
    bound of a sum, with the division and the restatement's own rounding in the 6); a value itself differs by the two logarithms
    (1 ulp = 2 u each side) and the roundings of the interpolation (its difference, quotient, product and sum on values up to 2 V,
    both sides): 20 u V at most; so d = v - mean is off by dd = ((n + 6) S / n + 20 V) u.  The variance is a sum of n squares,
    (n + 6) u relative, and moves with d: sd is off by (n + 6) u / 2 + dd / sd relative.  x = d / sd:
    |dx| <= dd / sd (1 + |x|) + (n + 6) u |x|."""
    v, x, sd = ref["filled"][c], ref["x"][c], ref["std"][c]
    n = len(v)
    if not x.any():
        return np.zeros(n)  # a flat channel is zeros on both sides
    dd = ((n + 6) * np.abs(v).sum() / n + 20.0 * np.abs(v).max()) * U
    return dd / sd * (1.0 + np.abs(x)) + (n + 6) * U * np.abs(x)


def transform_bound(A):
    """(taps + 2) 2^-52 s^(-1/2) sum |x| |psi| per element: a chain of `taps` fused multiply-adds and the product with s^(-1/2) against
    the restatement's exact sum of rounded products."""
    taps = np.array([16 * s + 3 for s in pr.SCALES], dtype=np.float64)
    return taps[None, :, None] * 2.0 ** -52 * A


def test_channels_within_the_rounding_bound_of_their_sums(measured):
    worst = 0.0
    for u, (ref, got) in enumerate(zip(cases.restated(), measured[1])):
        assert got["x"].shape == ref["x"].shape and np.isfinite(got["x"]).all()
        for c in range(3):
            tol = channel_bound(ref, c)
            err = np.abs(got["x"][c] - ref["x"][c])
            if tol.any():
                worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (u, c, float(err.max()), float(tol.min()))
    print("channels: largest error / bound", worst)
    assert not measured[1][cases.UNVOICED]["x"][0].any()  # no voiced frame: the pitch channel is all 0
    assert not measured[1][0]["x"].any()  # T = 1


def test_transform_of_the_restated_channels_within_its_bound(meter):
    """tts_prominence_cwt on the restatement's own channels, uploaded: the transform alone."""
    refs = cases.restated()
    frames = list(cases.FRAMES)
    utts, _, _ = meter.layout(frames, [np.zeros((0, 3), dtype=np.int32)] * len(frames), [np.zeros((0, 2), dtype=np.int32)] * len(frames))
    x = torch.from_numpy(np.ascontiguousarray(np.concatenate([r["x"] for r in refs], axis=1))).to(DEV)
    w = meter.cwt(x, utts).cpu().numpy()
    worst, at = 0.0, 0
    for u, (ref, T) in enumerate(zip(refs, frames)):
        got, tol = w[:, :, at:at + T], transform_bound(ref["A"])
        err = np.abs(got - ref["W"])
        assert np.all(err <= tol), (u, float(err.max()))
        if tol.any():
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
        at += T
    print("transform: largest error / bound", worst)


def test_decisions_are_the_restatements_and_values_within_the_band_sum_of_the_bound(measured):
    """peak_frame and valley_frame exactly (every decision of these cases has a relative margin of 1e-9:
    tests/test_prominence_cpu.py); the values within the transform's bound summed over the band and the channels with their weights,
    to which the channels' own bound adds max |dx| s^(-1/2) sum |psi| per scale."""
    worst = 0.0
    for u, (ref, rows, got) in enumerate(zip(cases.restated(), measured[0], measured[1])):
        want = ref["rows"]
        assert rows.shape == want.shape and np.array_equal(rows[:, 1], want[:, 1]) and np.array_equal(rows[:, 7], want[:, 7]), u
        assert np.array_equal(np.isnan(rows), np.isnan(want)), u
        tol_w = transform_bound(ref["A"])
        for c in range(3):
            dx = channel_bound(ref, c).max()
            for j, s in enumerate(pr.SCALES):
                tol_w[c, j] += dx * s ** -0.5 * np.abs(pr.taps(j)).sum()
        tol_c = np.stack([WEIGHTS[c] * tol_w[c, BAND[0]:BAND[1] + 1].sum(axis=0) for c in range(3)])
        tol_p = tol_c.sum(axis=0) + 8 * U * np.abs(ref["P"])
        assert np.all(np.abs(got["p"] - ref["P"]) <= tol_p), (u, float(np.abs(got["p"] - ref["P"]).max()))
        worst = max(worst, float((np.abs(got["p"] - ref["P"]) / np.where(tol_p > 0, tol_p, 1.0)).max()))
        for k in np.flatnonzero(want[:, 1] >= 0):
            pk = int(want[k, 1])
            b, e = cases.batch()[u][3][k]
            assert abs(rows[k, 0] - want[k, 0]) <= tol_p[pk] and abs(rows[k, 2] - want[k, 2]) <= tol_p[b:e].max() * (1 + 1e-9) + (e - b + 2) * U * np.abs(ref["P"][b:e]).max()
            assert np.all(np.abs(rows[k, 3:6] - want[k, 3:6]) <= tol_c[:, pk] + 8 * U * np.abs(want[k, 3:6]))
            if want[k, 7] >= 0:
                assert abs(rows[k, 6] - want[k, 6]) <= tol_p[int(want[k, 7])]
    print("composite: largest error / bound", worst)
    # the fixture's special units
    rows = measured[0][7]
    units = cases.batch()[7][3].tolist()
    assert math.isnan(rows[units.index([262, 262]), 0]) and rows[units.index([262, 262]), 1] == -1
    assert rows[units.index([1280, 1281]), 1] == 1280 and math.isnan(measured[0][0][0, 0]) and measured[0][0][1, 1] == 0


def test_every_utterance_alone_has_the_bits_of_the_batch(meter, measured):
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    for u, case in enumerate(cases.batch()):
        rows, extra = meter.measure_tracks(*[[part] for part in case], return_scalogram=True)
        assert np.array_equal(bits(rows[0]), bits(measured[0][u])), u
        for key in ("x", "w", "p"):
            assert np.array_equal(bits(extra[0][key]), bits(measured[1][u][key])), (u, key)
    # other weights and another band move the rows, not the transform
    rows, extra = meter.measure_tracks(*[[part] for part in cases.batch()[5]], weights=(0.0, 2.0, 1.0), band=(0, 5), return_scalogram=True)
    assert np.array_equal(bits(extra[0]["w"]), bits(measured[1][5]["w"])) and not np.array_equal(bits(rows[0]), bits(measured[0][5]))
    W = measured[1][5]["w"]
    assert np.allclose(extra[0]["p"], 2.0 * W[1].sum(axis=0) + W[2].sum(axis=0), rtol=0, atol=1e-12 * np.abs(W).max())


def test_refusals_reach_the_caller(meter):
    f0, e, ph, un = (list(v) for v in zip(*cases.batch()[2:4]))
    with pytest.raises(ValueError, match="utterance 1, unit 1 begins"):
        meter.measure_tracks(f0, e, ph, [un[0], np.array([[0, 9], [5, 20]])])
    with pytest.raises(ValueError, match="weight"):
        meter.measure_tracks(f0, e, ph, un, weights=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="outside 0 .. 5"):
        meter.measure_tracks(f0, e, ph, un, band=(0, 6))
    assert meter.max_frames == prominence.MAX_FRAMES


def five_words_wave(stressed, seed=3):
    """16 kHz: five words of 25 frames of a 120 Hz voice, 6 quiet frames around and between them; the stressed word is 30 % higher
    and 1.5 times louder.  -> (wave, feats [11, 62], durations [11])."""
    rng = np.random.default_rng(seed)
    durations = [6] + [25, 6] * 5
    hz, level = [], []
    for k, d in enumerate(durations):
        word = (k - 1) // 2 if k % 2 == 1 else None
        hz += [120.0 * (1.3 if word == stressed else 1.0)] * (256 * d)
        level += [0.0 if word is None else (1.5 if word == stressed else 1.0)] * (256 * d)
    wave = pitch_ref.harmonic(np.asarray(hz), rng, noise=0.0) * np.asarray(level) + 0.0005 * rng.standard_normal(len(hz))
    feats = np.zeros((len(durations), 62), dtype=np.float32)
    feats[1::2, prosody.F_PHONEME] = 1.0
    return wave.astype(np.float32), feats, np.asarray(durations)


def test_end_to_end_the_stressed_word_of_a_waveform_is_the_most_prominent(meter):
    wave, feats, durations = five_words_wave(stressed=3)
    assert prosody.word_spans(feats) == [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10)]
    report = meter.measure([wave], 16000, [feats], durations=[durations])[0]
    print(np.round(report[:, 0], 3), np.round(report[:, 6], 3))
    assert report.shape == (5, 8) and np.isfinite(report[:, :6]).all() and int(np.argmax(report[:, 0])) == 3
    assert meter.last["units"][0].tolist() == [[6, 31], [37, 62], [68, 93], [99, 124], [130, 155]] and len(meter.last["f0"][0]) == 1 + len(wave) // 256
    spans = prominence.to_emphasis(feats, report, pitch=1.4)
    assert [(s.start, s.stop, s.pitch) for s in spans] == [(7, 8, 1.4)]
    # at 24 kHz through the device resampler: the same word
    from ims_toucan_prosody_variance_amd import resample
    wave24, spans24 = resample.Resampler(DEV).resample(torch.from_numpy(wave).to(DEV), [(0, len(wave))], 16000, 24000)
    report24 = meter.measure([wave24.cpu().numpy()[:spans24[0][1]]], 24000, [feats], durations=[durations])[0]
    assert int(np.argmax(report24[:, 0])) == 3


# ---- the interface ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    """Fixture weights in the bf16 configuration: a 16-bit configuration synthesises an utterance bit for bit whatever the batch."""
    models = tmp_path_factory.mktemp("prominence_models") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(interface, "MODELS_DIR", str(models))
        mp.setenv("TOUCAN_PRECISION", "bf16")
        mp.delenv("TOUCAN_PY_SEQUENCER", raising=False)
        yield interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)


PHONES = ["~wˈɜːld tˈu~#", "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#"]


def expected_finite(report, words, durations):
    """A word with frames has a finite row, bar the boundary behind the last of them."""
    cum = np.concatenate([[0], np.cumsum(durations)])
    full = [k for k, (a, b) in enumerate(words) if cum[b] > cum[a]]
    assert report.shape == (len(words), 8) and len(full) >= 1
    assert np.isfinite(report[full, :6]).all() and np.isfinite(report[full[:-1], 6:]).all() and math.isnan(report[full[-1], 6])


def test_word_prominence_is_measure_on_the_waves_and_durations_it_used(tts):
    res = tts.word_prominence(PHONES, keep_waves=True)
    feats = [phones_to_features(p) for p in PHONES]
    again = tts._prominence().measure([r["synth"] for r in res], tts.SAMPLE_RATE, feats, durations=[r["durations"] for r in res])
    for u, (r, a, f) in enumerate(zip(res, again, feats)):
        assert np.array_equal(r["report"].view(np.uint64), a.view(np.uint64)) and r["words"] == prosody.word_spans(f)
        assert np.array_equal(r["durations"], tts.last_durations[u].cpu().numpy())
        expected_finite(r["report"], r["words"], r["durations"])
        print(np.round(r["report"][:, 0], 3))


def test_grid_with_the_emphasis_sweep_returns_the_matrix(tts):
    """One row per word and variant.  With the fixture's seeded weights the diagonal of "word stressed x word measured" need not
    dominate: this is plumbing, not quality."""
    feats = phones_to_features(PHONES[1])
    words = prosody.word_spans(feats)
    sweep = [prosody.emphasis(feats, [k]) for k in range(len(words))]
    frames = [v["frames"] for v in tts.synthesize_grid(PHONES[1], curves=sweep)]
    gen = torch.Generator().manual_seed(24)
    zs = [0.8 * torch.randn((80, f), generator=gen) for f in frames]  # the PostFlow's noise, given: a variant has the same bits in every call
    res = tts.synthesize_grid(PHONES[1], curves=sweep, z_noise=zs, word_prominence=True)
    assert len(res) == len(words) == 4
    for r in res:
        assert r["prominence"].dtype == np.float64 and r["prominence"].shape == (4, 8) and np.isfinite(r["prominence"][:, :6]).all()
    matrix = np.stack([r["prominence"][:, 0] for r in res])
    print(np.round(matrix, 3))
    plain = tts.synthesize_grid(PHONES[1], curves=sweep, z_noise=zs)
    assert all(set(p) == set(r) - {"prominence"} for p, r in zip(plain, res))
    assert all(torch.equal(p["wave"], r["wave"]) for p, r in zip(plain, res))
    assert set(tts.synthesize_grid(PHONES[1], (0.9, 1.1))[0]) == {"scales", "wave", "frames", "stats_before", "stats_after"}
    # every variant's report is the one its wave and its durations give alone
    alone = tts.word_prominence([PHONES[1]], prosody_curves=[sweep[2]], z_noise=[zs[2]])[0]
    assert np.array_equal(alone["report"].view(np.uint64), res[2]["prominence"].view(np.uint64))
    expected_finite(alone["report"], alone["words"], alone["durations"])


def test_cloner_measures_a_recording_with_the_aligners_durations(tmp_path_factory, monkeypatch):
    """``UtteranceCloner.word_prominence``: the aligner and MAS lay the transcript onto the frames of the recording's own STFT; the
    report is the one ``measure`` gives on the normalised wave with those durations, bit for bit.  The fixture aligner's seeded
    weights align arbitrarily: plumbing and determinism, not quality."""
    import os
    from ims_toucan_prosody_variance_amd import fixture_weights as fw, style
    models = tmp_path_factory.mktemp("prominence_cloner") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    monkeypatch.setenv("TOUCAN_PRECISION", "bf16")
    monkeypatch.delenv("TOUCAN_PY_SEQUENCER", raising=False)
    from InferenceInterfaces.UtteranceCloner import UtteranceCloner
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner", "aligner.npz"))
    phones = str(G["clone_phones"][1])
    path = str(models.parent / "recording.wav")
    interface.write_wav(path, fw.reference_wave(int(G["clone1_seed"]), int(G["clone1_samples"])), 16000)
    cl = UtteranceCloner(model_id=str(models / "ToucanTTS_Meta" / "best.pt"), device=DEV, language="en")
    res = cl.word_prominence(phones, path)
    feats = np.asarray(phones_to_features(phones, handle_missing=False), dtype=np.float32)
    data, sr = style.read_audio(path)
    norm = style.normalize_reference_audio(data, sr)
    frames = 1 + len(norm) // 256
    assert res["words"] == prosody.word_spans(feats) and len(res["durations"]) == feats.shape[0] and 0 < res["durations"].sum() <= frames
    expected_finite(res["report"], res["words"], res["durations"])
    again = cl._prominence_obj.measure([norm], 16000, [feats], durations=[res["durations"]])[0]
    assert np.array_equal(again.view(np.uint64), res["report"].view(np.uint64))
    assert cl._prominence_obj.extractor is cl.extractor and cl._prominence_obj.ops is cl.extractor.ops  # one front end
    cut = cl.word_prominence(phones, path, speech_bounds=(1600, len(norm) - 1600))
    assert cut["report"].shape == res["report"].shape and cut["durations"].sum() <= 1 + (len(norm) - 3200) // 256
    with pytest.raises(ValueError, match="speech_bounds"):
        cl.word_prominence(phones, path, speech_bounds="guess")
    with pytest.raises(ValueError, match="needs the aligner"):
        prominence.ProminenceMeter(DEV).measure([norm], 16000, [feats])
