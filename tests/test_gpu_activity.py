"""The speech-activity meter (csrc/activity.hip) on the MI355X against the float64 restatement (tests/activity_ref.py): the active
counts at all 15 thresholds, the runs, their number and both bounds exactly (tests/test_activity_cpu.py asserts the condition
under which they may be demanded: no envelope sample within 1e-9 of a threshold), the sum of squares within n 2^-53, the peak
exactly, the segment start states within the derived bound, the three dB columns within 1e-6 dB; a ragged batch against its
utterances alone bit for bit; the normalised wave; and the places the meter plugs into: ``speech_bounds="detect"`` of the cloner,
``trim_silence`` of the style embedding, ``speech_level`` of the interface's calls.

Worst errors per rate measured on the MI355X are recorded in DESIGN.md section 18."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import activity, align, capi, fixture_weights as fw, interface, style
from tests import activity_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
TARGET, CEILING = -26.0, -1.0
CEIL_LIN = 10.0 ** (CEILING / 20.0)
COL = {name: i for i, name in enumerate(activity.ACTIVITY_COLUMNS)}
DB = ("active_db", "long_term_db", "threshold_db")


@functools.lru_cache(maxsize=None)
def meter():
    return activity.SpeechActivity(DEV)


def tile():
    return int(capi.lib().tts_activity_tile_segments())


def run(m, waves, sr):
    """Measure and normalise the waves as ONE ragged launch -> per wave dict(stats, counts, runs, sums, states, norm, y)."""
    S = sr // 10
    begins = np.concatenate([[0], np.cumsum([len(x) for x in waves])[:-1]]).astype(np.int64)
    spans = [(int(b), len(x)) for b, x in zip(begins, waves)]
    packed = torch.from_numpy(np.concatenate(waves).astype(np.float32)).to(DEV)
    stats = m.measure(packed, spans, sr, max_runs=ar.MAX_RUNS).cpu().numpy()
    counts, runs, sums, states = (t.cpu().numpy() for t in (m.last_counts, m.last_runs, m.last_sums, m.last_states))
    y, norm = m.normalize(packed, spans, sr, TARGET, CEILING, max_runs=ar.MAX_RUNS)
    y, norm = y.cpu().numpy(), norm.cpu().numpy()
    assert np.array_equal(counts, m.last_counts.cpu().numpy()) and np.array_equal(runs, m.last_runs.cpu().numpy())
    assert stats.dtype == norm.dtype == np.float64 and stats.shape == norm.shape == (len(waves), 8) and y.dtype == np.float32
    assert counts.shape == (len(waves), 16) and runs.shape == (len(waves), ar.MAX_RUNS, 2) and counts.dtype == runs.dtype == np.int64
    return [{"stats": stats[u], "counts": counts[u], "runs": runs[u], "sums": sums[u], "states": states[u, :-(-n // S)].copy(), "norm": norm[u],
             "y": y[b:b + n].copy()} for u, (b, n) in enumerate(spans)]


@functools.lru_cache(maxsize=None)
def batch_on_device(sr, reverse=False):
    cases = ar.cases(sr, tile())
    order = list(reversed(range(len(cases)))) if reverse else list(range(len(cases)))
    got = run(meter(), [cases[i]["x"] for i in order], sr)
    return [got[order.index(i)] for i in range(len(cases))]


def close_db(a, b, tol):
    return a == b if not (math.isfinite(a) and math.isfinite(b)) else abs(a - b) <= tol


def test_the_tile_and_the_lengths_aim_at_its_edges():
    T = tile()
    assert T == 64 and meter().tile_segments == T
    names = {c["name"]: c["n"] for c in ar.cases(8000, T)}
    assert names["one_workgroup"] == T * 800 and -(-names["across_workgroups"] // 800) == T + 3 and names["past_two_workgroups"] == (2 * T + 3) * 800


@pytest.mark.parametrize("sr", ar.RATES)
def test_kernel_against_the_float64_restatement(sr):
    """a_0 .. a_14, the runs (the first MAX_RUNS of them), their true number and both bounds exact; sq within n 2^-53 relative, the
    peak exact; the start state of every segment within the derived bound; the three dB columns within 1e-6 dB (-inf where the
    restatement says -inf); measuring alone leaves gain = 1."""
    worst_state = worst_db = worst_sq = 0.0
    for c, got in zip(ar.cases(sr, tile()), batch_on_device(sr)):
        name, s = c["name"], got["stats"]
        assert got["counts"][:15].tolist() == c["a"], (name, got["counts"][:15].tolist(), c["a"])
        assert int(got["counts"][15]) == len(c["runs"]), (name, got["counts"][15], c["runs"])
        kept = c["runs"][:ar.MAX_RUNS]
        assert got["runs"][:len(kept)].tolist() == [list(r) for r in kept] and not got["runs"][len(kept):].any(), (name, got["runs"], c["runs"])
        assert (int(s[COL["speech_begin"]]), int(s[COL["speech_end"]])) == (c["speech_begin"], c["speech_end"]), name
        sq_err = abs(got["sums"][0] - c["sq"])
        assert sq_err <= c["n"] * ar.U * c["sq"], (name, got["sums"][0], c["sq"])
        assert got["sums"][1] == c["peak"], name
        if c["sq"] > 0:
            worst_sq = max(worst_sq, sq_err / c["sq"])
        assert got["states"].shape == c["starts"].shape, name
        err = np.abs(got["states"] - c["starts"]).max(initial=0.0)
        assert err <= c["state_bound"], (name, err, c["state_bound"])
        if c["state_bound"] > 0:
            worst_state = max(worst_state, float(err / c["state_bound"]))
        for k in DB:
            assert close_db(float(s[COL[k]]), c[k], 1e-6), (name, k, s[COL[k]], c[k])
            if math.isfinite(c[k]):
                worst_db = max(worst_db, abs(float(s[COL[k]]) - c[k]))
        assert abs(s[COL["activity"]] - c["activity"]) <= 1e-9, name
        assert s[COL["gain"]] == 1.0 and s[COL["active_db_after"]] == s[COL["active_db"]], name
    print(f"{sr} Hz (S {sr // 10}): worst |state error| / bound {worst_state:.3e}, worst relative sq error {worst_sq:.3e}, worst dB error {worst_db:.3e}")


@pytest.mark.parametrize("sr", ar.RATES)
def test_ragged_batch_equals_each_utterance_alone(sr):
    """Bit for bit in every output, the normalised wave included; the same with the batch reversed."""
    m = meter()
    forward, backward = batch_on_device(sr), batch_on_device(sr, True)
    for c, a, b in zip(ar.cases(sr, tile()), forward, backward):
        alone = run(m, [c["x"]], sr)[0]
        for other in (a, b):
            for key in ("stats", "norm", "counts", "runs", "sums", "states", "y"):
                assert np.array_equal(alone[key], other[key], equal_nan=True), (c["name"], key)


@functools.lru_cache(maxsize=None)
def scaled_reference(sr):
    """The restatement's level of every normalised wave of the batch (the device's output, measured on the host)."""
    return tuple(ar.measure(g["y"], sr)["active_db"] for g in batch_on_device(sr))


@pytest.mark.parametrize("sr", ar.RATES)
def test_normalize_reaches_the_target_or_the_ceiling(sr):
    """The output is x float32(gain) exactly and the gain is the definition's, rounded to float32.  Re-measured on the device, the
    output reads active_db_after within 1e-5 dB, and so does the restatement of the scaled wave, within 1e-6 dB: the column is
    the level MEASURED on the output, because P.56 does not follow a gain that is no power of two exactly (the ladder stays where
    it is; include/toucan_activity.h, 5).  How far the level reached lies from the target is printed and recorded in DESIGN.md
    section 18; it is a property of the method, so no tolerance of this test.  The click stops at the ceiling; an utterance
    without a level comes back bit for bit with gain 1."""
    cases, got = ar.cases(sr, tile()), batch_on_device(sr)
    again = run(meter(), [g["y"] for g in got], sr)
    limited, off = [], 0.0
    for c, g, a, ref_after in zip(cases, got, again, scaled_reference(sr)):
        n = g["norm"]
        assert np.array_equal(n[:6], g["stats"][:6], equal_nan=True), c["name"]  # what was measured does not depend on the target
        gain = float(n[COL["gain"]])
        assert gain == float(np.float32(gain)) and np.array_equal(g["y"], c["x"] * np.float32(gain)), c["name"]
        if not math.isfinite(c["active_db"]):
            assert gain == 1.0 and n[COL["active_db_after"]] == -math.inf and np.array_equal(g["y"].view(np.uint32), c["x"].view(np.uint32)), c["name"]
            continue
        want, lim = ar.gain(c["active_db"], c["peak"], TARGET, CEILING)
        assert abs(gain / want - 1.0) <= 2.0 ** -24 + 2e-7, (c["name"], gain, want)  # 1e-6 dB of the level are 1.2e-7 of the gain
        assert abs(a["stats"][COL["active_db"]] - n[COL["active_db_after"]]) <= 1e-5, (c["name"], a["stats"][COL["active_db"]], n[COL["active_db_after"]])
        assert abs(n[COL["active_db_after"]] - ref_after) <= 1e-6, (c["name"], n[COL["active_db_after"]], ref_after)
        assert float(np.abs(g["y"]).max()) <= CEIL_LIN and g["sums"][1] * gain <= CEIL_LIN, c["name"]
        if lim:
            limited.append(c["name"])
            assert g["sums"][1] * gain > CEIL_LIN * (1.0 - 2.0 ** -22) and n[COL["active_db_after"]] < TARGET - 1.0, c["name"]
        else:
            off = max(off, abs(n[COL["active_db_after"]] - TARGET))
    print(f"{sr} Hz: the level reached lies at most {off:.3e} dB from the target where the ceiling does not limit the gain")
    assert "click" in limited and "bursts_far" not in limited and "three_runs" not in limited
    assert sum(1 for c in cases if not math.isfinite(c["active_db"])) == 4 and any(c["n"] == 0 for c in cases)


def test_apply_gain_in_place_equals_out_of_place():
    sr, m = 24000, meter()
    cases = [c for c in ar.cases(sr, tile()) if c["name"] in ("noise_S+1", "empty", "zeros", "click", "bursts_close")]
    begins = np.concatenate([[0], np.cumsum([c["n"] for c in cases])[:-1]])
    spans = [(int(b) + 3, c["n"]) for b, c in zip(begins, cases)]  # three samples in front and five behind belong to no utterance
    host = np.concatenate([np.full(3, 0.25, dtype=np.float32)] + [c["x"] for c in cases] + [np.full(5, -0.25, dtype=np.float32)])
    packed = torch.from_numpy(host).to(DEV)
    out, stats = m.normalize(packed, spans, sr, TARGET, CEILING)
    assert torch.equal(packed.cpu(), torch.from_numpy(host))  # the input is left alone
    other = torch.full_like(packed, 7.0)
    out2, stats2 = m.normalize(packed, spans, sr, TARGET, CEILING, out=other)
    assert out2 is other and torch.equal(stats, stats2)
    inplace = packed.clone()
    out3, stats3 = m.normalize(inplace, spans, sr, TARGET, CEILING, out=inplace)
    assert out3 is inplace and torch.equal(stats, stats3)
    lo, hi = 3, len(host) - 5
    assert torch.equal(out[lo:hi], out2[lo:hi]) and torch.equal(out, out3)
    assert torch.equal(out[:lo], packed[:lo]) and torch.equal(out[hi:], packed[hi:]) and bool((out2[:lo] == 7.0).all()) and bool((out2[hi:] == 7.0).all())
    gains = stats.cpu().numpy()[:, COL["gain"]]
    assert [c["name"] for c in cases][:2] == ["empty", "noise_S+1"] and gains[0] == 1.0 and len(set(gains.tolist())) == 4


def test_the_entries_refuse_spans_outside_the_wave():
    m = meter()
    x = torch.zeros(100, device=DEV)
    with pytest.raises(capi.ToucanHipError, match="utterance 1"):
        m.measure(x, [(0, 50), (60, 41)], 24000)
    with pytest.raises(capi.ToucanHipError, match="utterance 0"):
        m.normalize(x, [(-1, 50)], 24000)
    with pytest.raises(ValueError, match="multiple of 10"):
        m.measure(x, [(0, 100)], 22055)
    with pytest.raises(ValueError, match="above full scale"):
        m.normalize(x, [(0, 100)], 24000, -26.0, 3.0)
    assert m.measure(x, [], 24000).shape == (0, 8) and m.last_counts.shape == (0, 16)
    assert m.measure(x, [(0, 100)], 24000, max_runs=0).shape == (1, 8) and m.last_runs.shape == (1, 0, 2)


# ---- where it plugs in --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("activity_models") / "Models"
    interface.write_fixture_checkpoints(str(d), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(d))
    return d


@pytest.fixture(scope="module")
def tts(models):
    """Fixture weights in the bf16 configuration: a 16-bit configuration synthesises an utterance bit for bit whatever the batch."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(interface, "MODELS_DIR", str(models))
        mp.setenv("TOUCAN_PRECISION", "bf16")
        mp.delenv("TOUCAN_PY_SEQUENCER", raising=False)
        yield interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)


@pytest.fixture(scope="module")
def padded(tmp_path_factory):
    """A 16 kHz stand-in recording with 0.5 s of zeros at both ends, as a file; (path, normalised 16 kHz wave, phonemes, an f0
    track: the stored one of the recording, which the extractor fits to the frames of whatever span it is given)."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner", "aligner.npz"))
    wave = fw.reference_wave(int(G["clone1_seed"]), int(G["clone1_samples"]))
    wave = np.concatenate([np.zeros(8000), wave, np.zeros(8000)])
    path = str(tmp_path_factory.mktemp("activity_wave") / "padded.wav")
    interface.write_wav(path, wave, 16000)
    data, sr = style.read_audio(path)
    return path, style.normalize_reference_audio(data, sr), str(G["clone_phones"][1]), G["clone1_f0"]


def detected(wave16, lead):
    m = meter()
    x = torch.from_numpy(np.asarray(wave16, dtype=np.float32)).to(DEV)
    return activity.bounds(m.measure(x, [(0, x.numel())], 16000), lead=lead)[0]


PHONES = ["~həlˈoʊ~#", "~wˈɜːld tˈu~#", "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#"]


def gold(tts, phones, frames=6, seed=3):
    L = int(tts.text2phone.string_to_tensor(phones, input_phonemes=True).shape[0])
    z = torch.randn(80, frames * L, generator=torch.Generator().manual_seed(seed)) * 0.8
    return torch.full((L,), frames, dtype=torch.long), z


def test_cloner_detects_the_speech_bounds(models, padded, monkeypatch):
    """speech_bounds="detect" equals the same call with the bounds from ``bounds(..., lead=480)``, bit for bit; both silences are
    those of the padding, within the envelope's delays; a recording without speech is refused by name."""
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    from InferenceInterfaces.UtteranceCloner import UtteranceCloner
    monkeypatch.setattr(UtteranceCloner, "_warned_fine_tune", False)  # the notice is given once per process: leave it as it was found
    path, wave16, phones, f0 = padded
    found = detected(wave16, align.DETECT_LEAD)
    # (the stand-in recording sets in under a random envelope, so its onset is found later than a tone's: within 100 ms)
    assert found is not None and 8000 - 480 <= found[0] <= 8000 + 1600 - 480 and len(wave16) - 8000 <= found[1] <= len(wave16) - 8000 + 1920, found
    cl = UtteranceCloner(model_id=str(models / "ToucanTTS_Meta" / "best.pt"), device=DEV, language="en")
    with pytest.warns(UserWarning):
        want = cl.extract_prosody(phones, path, lang="en", f0=f0, speech_bounds=found)
    got = cl.extract_prosody(phones, path, lang="en", f0=f0, speech_bounds="detect")
    assert got[3] == want[3] == found[0] > 0 and got[4] == want[4] == len(wave16) - found[1] > 0
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    plain = cl.extract_prosody(phones, path, lang="en", f0=f0)
    assert plain[3] == plain[4] == 0 and int(plain[0].sum()) > int(got[0].sum())  # (the default is the path as it was)
    data, sr = style.read_audio(path)
    batch = cl.extract_prosody_batch([phones, phones], [data, data], sr, f0=[f0, f0], speech_bounds=["detect", found])
    for row in batch:
        assert row[3:] == got[3:] and all(torch.equal(a, b) for a, b in zip(row[:3], got[:3]))
    z = torch.randn(80, int(got[0].sum()), generator=torch.Generator().manual_seed(5)) * 0.8
    a = cl.clone_utterance(path, path, phones, lang="en", f0=f0, speech_bounds="detect", z_noise=z)
    b = cl.clone_utterance(path, path, phones, lang="en", f0=f0, speech_bounds=found, z_noise=z)
    assert np.array_equal(a, b) and not a[:3 * got[3]].any() and not a[len(a) - 3 * got[4]:].any()
    with pytest.raises(ValueError, match="utterance 1"):
        cl.extract_prosody_batch([phones, phones], [data, np.zeros(16000)], sr, f0=[f0, f0], speech_bounds="detect")


def test_style_embedding_of_the_trimmed_wave(tts, padded, tmp_path, monkeypatch):
    """set_utterance_embedding(trim_silence=True) equals the embedding of the hand-cut wave; the default is the call as it was; a
    recording without speech stays uncut, with a warning."""
    path, wave16, _, _ = padded
    before = tts.default_utterance_embedding.clone()
    try:
        found = detected(wave16, 480)
        cut = str(tmp_path / "cut.wav")
        # (the hand-cut wave goes through the embedding's own path: as a tensor it would skip the log-mel)
        logmel, gst = (tts.set_utterance_embedding(path), tts._style)[1]
        uncut = tts.default_utterance_embedding.clone()
        want = gst.forward([logmel.forward(wave16[found[0]:found[1]])])[0].to(tts.device)
        tts.set_utterance_embedding(path, trim_silence=True)
        assert torch.equal(tts.default_utterance_embedding, want) and not torch.equal(want, uncut)
        tts.set_utterance_embedding(path, trim_silence=False)
        assert torch.equal(tts.default_utterance_embedding, uncut)
        interface.write_wav(cut, np.zeros(16000), 16000)
        tts.set_utterance_embedding(cut)
        silent = tts.default_utterance_embedding.clone()
        monkeypatch.setattr(interface.ToucanTTSInterface, "_warned_trim", False)  # (once per process: left as it was found)
        with pytest.warns(UserWarning, match="uncut"):
            tts.set_utterance_embedding(cut, trim_silence=True)
        assert torch.equal(tts.default_utterance_embedding, silent)
    finally:
        tts.default_utterance_embedding = before


def test_interface_speech_level_is_normalize_of_the_plain_call(tts):
    """forward(speech_level=-26, z_noise=z) equals normalize of forward(z_noise=z); None keeps the bits and makes no launch."""
    d, z = gold(tts, PHONES[2])
    kw = dict(input_is_phones=True, durations=d, z_noise=z)
    tts.last_speech_activity = None
    plain = tts(PHONES[2], **kw)
    before = capi.CALLS
    assert torch.equal(tts(PHONES[2], **kw), plain)
    calls = capi.CALLS - before
    before = capi.CALLS
    assert torch.equal(tts(PHONES[2], speech_level=None, peak_ceiling=-3.0, **kw), plain)
    assert capi.CALLS - before == calls and tts.last_speech_activity is None  # no launch is added
    before = capi.CALLS
    level = tts(PHONES[2], speech_level=TARGET, **kw)
    assert capi.CALLS - before == calls + 6 and level.shape == plain.shape and level.dtype == torch.float32
    want, rows = meter().normalize(plain.contiguous(), [(0, plain.numel())], 24000, TARGET, CEILING)
    stats, runs, counts = tts.last_speech_activity
    assert torch.equal(level, want) and torch.equal(stats, rows) and stats.shape == (1, 8) and stats.is_cuda
    assert runs.shape == (1, 64, 2) and counts.shape == (1, 16) and torch.equal(runs, meter().last_runs) and torch.equal(counts, meter().last_counts)
    row = stats.cpu().numpy()[0]
    print("forward:", dict(zip(activity.ACTIVITY_COLUMNS, row.tolist())), "runs", int(counts[0, 15]))
    assert math.isfinite(row[COL["active_db"]]), "the fixture voice is expected to be audible"
    assert torch.equal(level, plain * torch.tensor(row[COL["gain"]], dtype=torch.float32, device=plain.device))
    again = meter().measure(level.contiguous(), [(0, level.numel())], 24000).cpu().numpy()[0]
    assert abs(again[COL["active_db"]] - row[COL["active_db_after"]]) <= 1e-5
    with pytest.raises(ValueError, match="give one of them"):
        tts(PHONES[2], speech_level=TARGET, loudness=-23.0, **kw)


def test_interface_batch_grid_and_file_carry_the_rows(tts, tmp_path):
    dz = [gold(tts, p, seed=s) for s, p in enumerate(PHONES)]
    batch = tts.synthesize_batch(PHONES, durations=[d for d, _ in dz], z_noise=[z for _, z in dz], speech_level=TARGET)
    stats, runs, counts = (t.clone() for t in tts.last_speech_activity)
    assert stats.shape == (3, 8) and runs.shape == (3, 64, 2) and counts.shape == (3, 16)
    for u, (p, (d, z)) in enumerate(zip(PHONES, dz)):
        one = tts(p, input_is_phones=True, durations=d, z_noise=z, speech_level=TARGET)
        assert torch.equal(one, batch[u]) and torch.equal(tts.last_speech_activity[0][0], stats[u]), u
        assert torch.equal(tts.last_speech_activity[1][0], runs[u]) and torch.equal(tts.last_speech_activity[2][0], counts[u]), u
    d, z = dz[2]
    plain = tts.synthesize_grid(PHONES[2], energy_variance_scales=(1.0, 2.5), durations=d, z_noise=[z, z])
    grid = tts.synthesize_grid(PHONES[2], energy_variance_scales=(1.0, 2.5), durations=d, z_noise=[z, z], speech_level=TARGET)
    assert len(grid) == 2 and all("speech_activity" not in v for v in plain) and tts.last_speech_activity[0].shape == (2, 8)
    for i, (v, p) in enumerate(zip(grid, plain)):
        row, r, c = v["speech_activity"]
        assert torch.equal(row, tts.last_speech_activity[0][i]) and r.shape == (64, 2) and c.shape == (16,)
        assert torch.equal(v["wave"], p["wave"] * row[COL["gain"]].to(torch.float32))
    d0 = gold(tts, PHONES[0])[0]
    tts.read_to_file([PHONES[0], "", PHONES[2]], str(tmp_path / "level.wav"), silent=True, input_is_phones=True, dur_list=[d0, None, d],
                     speech_level=TARGET)
    assert tts.last_speech_activity[0].shape == (2, 8) and tts.last_speech_activity[1].shape == (2, 64, 2)
    with pytest.raises(ValueError, match="whole utterance"):
        next(tts.stream(PHONES[0], input_is_phones=True, speech_level=TARGET))
