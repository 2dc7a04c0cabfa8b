"""The loudness meter (csrc/loudness.hip) on the MI355X: segment energies, peaks, gate counts and loudness against the float64
restatement (tests/loudness_ref.py: the energies within its derived bound, the loudness within 1e-6 LU, everything countable
exactly), a ragged batch against its utterances alone bit for bit, the normalised wave re-measured, the peak ceiling, in place
against out of place, and the interface's ``loudness`` / ``peak_ceiling`` keywords.

Worst error / bound per rate measured on the MI355X is recorded in DESIGN.md section 17."""
import functools
import math
import wave

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, interface, loudness, resample
from tests import loudness_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
TARGET, CEILING = -23.0, -1.0
CEIL_LIN = 10.0 ** (CEILING / 20.0)
COL = {name: i for i, name in enumerate(loudness.LOUDNESS_COLUMNS)}


@functools.lru_cache(maxsize=None)
def meter():
    return loudness.LoudnessMeter(DEV)


def tile():
    return int(capi.lib().tts_loudness_tile_segments())


def run(m, waves, sr):
    """Measure and normalise the waves as ONE ragged launch -> per wave dict(stats, e, peaks, norm = stats of normalize, y)."""
    S = sr // 10
    begins = np.concatenate([[0], np.cumsum([len(x) for x in waves])[:-1]]).astype(np.int64)
    spans = [(int(b), len(x)) for b, x in zip(begins, waves)]
    packed = torch.from_numpy(np.concatenate(waves).astype(np.float32)).to(DEV)
    stats = m.measure(packed, spans, sr).cpu().numpy()
    energy, peak = (t.cpu().numpy() for t in m.last_segments)
    y, norm = m.normalize(packed, spans, sr, TARGET, CEILING)
    y, norm = y.cpu().numpy(), norm.cpu().numpy()
    assert stats.dtype == norm.dtype == np.float64 and stats.shape == norm.shape == (len(waves), 8) and y.dtype == np.float32
    return [{"stats": stats[u], "e": energy[u, :n // S].copy(), "peaks": peak[u, :-(-n // S)].copy(), "norm": norm[u], "y": y[b:b + n].copy()}
            for u, (b, n) in enumerate(spans)]


@functools.lru_cache(maxsize=None)
def batch_on_device(sr, reverse=False):
    cases = lr.cases(sr, tile())
    order = list(reversed(range(len(cases)))) if reverse else list(range(len(cases)))
    got = run(meter(), [cases[i]["x"] for i in order], sr)
    return [got[order.index(i)] for i in range(len(cases))]


def close_lufs(a, b, tol):
    return a == b if not (math.isfinite(a) and math.isfinite(b)) else abs(a - b) <= tol


def test_the_tile_and_the_lengths_aim_at_its_edges():
    T = tile()
    assert T == 64 and meter().tile_segments == T
    names = {c["name"]: c["n"] for c in lr.cases(8000, T)}
    assert -(-names["past_one_workgroup"] // 800) == T + 3 and -(-names["past_two_workgroups"] // 800) == 2 * T + 3


@pytest.mark.parametrize("sr", lr.RATES)
def test_kernel_against_the_float64_restatement(sr):
    """e_k within the derived bound of tests/loudness_ref.py, peaks and the three block counts exact, the loudness and the loudest
    block within 1e-6 LU (-inf where the restatement says -inf); measuring alone leaves gain = 1."""
    worst = worst_lufs = 0.0
    for c, got in zip(lr.cases(sr, tile()), batch_on_device(sr)):
        assert got["e"].shape == c["e"].shape and got["peaks"].shape == c["peaks"].shape, c["name"]
        err = np.abs(got["e"] - c["e"])
        pos = c["bound"] > 0
        worst = max(worst, float((err[pos] / c["bound"][pos]).max(initial=0.0)))
        bad = np.flatnonzero(err > c["bound"])
        assert bad.size == 0, (c["name"], bad[:5], err[bad[:5]], c["bound"][bad[:5]])
        assert np.array_equal(got["peaks"], c["peaks"]), c["name"]
        s = got["stats"]
        assert s[COL["peak"]] == c["peak"], c["name"]
        assert [int(s[COL[k]]) for k in ("blocks", "blocks_abs", "blocks_both")] == [c["blocks"], c["blocks_abs"], c["blocks_both"]], c["name"]
        assert close_lufs(float(s[COL["lufs"]]), c["lufs"], 1e-6), (c["name"], s[COL["lufs"]], c["lufs"])
        assert close_lufs(float(s[COL["momentary_max_lufs"]]), c["momentary_max_lufs"], 1e-6), (c["name"], s, c["momentary_max_lufs"])
        assert s[COL["gain"]] == 1.0 and (s[COL["lufs_after"]] == s[COL["lufs"]]), c["name"]
        if math.isfinite(c["lufs"]):
            worst_lufs = max(worst_lufs, abs(float(s[COL["lufs"]]) - c["lufs"]))
    r = lr.pole_radius(sr)[0]
    print(f"{sr} Hz (S {sr // 10}, r {r:.5f}): worst |e_k error| / bound {worst:.3e}, worst loudness error {worst_lufs:.3e} LU")


@pytest.mark.parametrize("sr", lr.RATES)
def test_ragged_batch_equals_each_utterance_alone(sr):
    """Bit for bit in the statistics, the segment energies, the peaks and the scaled wave; the same with the batch reversed."""
    m = meter()
    forward, backward = batch_on_device(sr), batch_on_device(sr, True)
    for c, a, b in zip(lr.cases(sr, tile()), forward, backward):
        alone = run(m, [c["x"]], sr)[0]
        for other in (a, b):
            for key in ("stats", "norm", "e", "peaks", "y"):
                assert np.array_equal(alone[key], other[key], equal_nan=True), (c["name"], key)


@pytest.mark.parametrize("sr", lr.RATES)
def test_normalize_reaches_the_target_or_the_ceiling(sr):
    """Re-measuring the output gives lufs_after within 1e-5 LU (one fp32 rounding per sample moves the loudness by at most
    20 log10(1 + 2^-24) = 5e-7 LU); the gain is the definition's, rounded to float32; the click ends at the ceiling and reports the
    loudness it really reached; an utterance without a loudness comes back bit for bit with gain 1."""
    cases, got = lr.cases(sr, tile()), batch_on_device(sr)
    again = run(meter(), [g["y"] for g in got], sr)
    limited = []
    for c, g, a in zip(cases, got, again):
        n = g["norm"]
        assert np.array_equal(n[:6], g["stats"][:6], equal_nan=True), c["name"]  # what was measured does not depend on the target
        gain = float(n[COL["gain"]])
        assert gain == float(np.float32(gain)) and np.array_equal(g["y"], c["x"] * np.float32(gain)), c["name"]
        if not math.isfinite(c["lufs"]):
            assert gain == 1.0 and n[COL["lufs_after"]] == -math.inf and np.array_equal(g["y"].view(np.uint32), c["x"].view(np.uint32)), c["name"]
            continue
        want, lim = lr.gain(c["lufs"], c["peak"], TARGET, CEILING)
        assert abs(gain / want - 1.0) <= 2.0 ** -24 + 2e-7, (c["name"], gain, want)  # 1e-6 LU of the loudness are 1.2e-7 of the gain
        assert abs(n[COL["lufs_after"]] - (n[COL["lufs"]] + 20.0 * math.log10(gain))) < 1e-12
        assert abs(a["stats"][COL["lufs"]] - n[COL["lufs_after"]]) <= 1e-5, (c["name"], a["stats"][COL["lufs"]], n[COL["lufs_after"]])
        assert float(np.abs(g["y"]).max()) <= CEIL_LIN and n[COL["peak"]] * gain <= CEIL_LIN, c["name"]
        if lim:
            limited.append(c["name"])
            assert n[COL["peak"]] * gain > CEIL_LIN * (1.0 - 2.0 ** -22) and n[COL["lufs_after"]] < TARGET - 1.0, c["name"]
        else:
            assert abs(n[COL["lufs_after"]] - TARGET) <= 1e-6, (c["name"], n[COL["lufs_after"]])
    # (the DC case too: its offset is in the sample peak and would be scaled with the tone)
    assert "click" in limited and "dc" in limited and "gates" not in limited and "noise_5S" not in limited and "sine" not in limited
    assert sum(1 for c in cases if not math.isfinite(c["lufs"])) == 4 and any(c["n"] == 0 for c in cases)


def test_apply_gain_in_place_equals_out_of_place():
    sr, m = 24000, meter()
    cases = [c for c in lr.cases(sr, tile()) if c["name"] in ("noise_5S-1", "empty", "click", "dc", "zeros")]
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
    # outside the spans: copied into a new tensor, untouched in a given one
    assert torch.equal(out[:lo], packed[:lo]) and torch.equal(out[hi:], packed[hi:]) and bool((out2[:lo] == 7.0).all()) and bool((out2[hi:] == 7.0).all())
    gains = stats.cpu().numpy()[:, COL["gain"]]
    assert [c["name"] for c in cases][1:3] == ["empty", "zeros"] and gains[1] == 1.0 and gains[2] == 1.0 and len(set(gains.tolist())) == 4


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
        m.normalize(x, [(0, 100)], 24000, -23.0, 3.0)
    assert m.measure(x, [], 24000).shape == (0, 8)


# ---- the interface ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    """Fixture weights in the bf16 configuration: a 16-bit configuration synthesises an utterance bit for bit whatever the batch."""
    models = tmp_path_factory.mktemp("loudness_models") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(interface, "MODELS_DIR", str(models))
        mp.setenv("TOUCAN_PRECISION", "bf16")
        mp.delenv("TOUCAN_PY_SEQUENCER", raising=False)
        yield interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)


PHONES = ["~həlˈoʊ~#", "~wˈɜːld tˈu~#", "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#"]


def gold(tts, phones, frames=6, seed=3):
    L = int(tts.text2phone.string_to_tensor(phones, input_phonemes=True).shape[0])
    z = torch.randn(80, frames * L, generator=torch.Generator().manual_seed(seed)) * 0.8
    return torch.full((L,), frames, dtype=torch.long), z


def check_rows(rows, waves, target=TARGET, ceiling=CEILING):
    """Every wave re-measured sits where its row says, and that is the target, or the ceiling where the row says so."""
    rows = rows.cpu().numpy()
    packed = torch.cat([w.float() for w in waves])
    spans, at = [], 0
    for w in waves:
        spans.append((at, w.numel()))
        at += w.numel()
    again = meter().measure(packed, spans, 24000).cpu().numpy()
    lin = 10.0 ** (ceiling / 20.0)
    for row, now in zip(rows, again):
        assert math.isfinite(row[COL["lufs"]]), "the fixture voice is expected to be audible"
        assert abs(now[COL["lufs"]] - row[COL["lufs_after"]]) <= 1e-5 and now[COL["peak"]] <= lin
        if row[COL["peak"]] * row[COL["gain"]] > lin * (1.0 - 2.0 ** -22):
            assert row[COL["lufs_after"]] < target  # at the ceiling, and the row says how far it got
        else:
            assert abs(row[COL["lufs_after"]] - target) <= 1e-5
    return rows


def test_interface_without_loudness_is_the_call_as_it_was(tts):
    d, z = gold(tts, PHONES[2])
    kw = dict(input_is_phones=True, durations=d, z_noise=z)
    tts.last_loudness = None
    plain = tts(PHONES[2], **kw)
    before = capi.CALLS
    assert torch.equal(tts(PHONES[2], **kw), plain)
    calls = capi.CALLS - before
    before = capi.CALLS
    assert torch.equal(tts(PHONES[2], loudness=None, peak_ceiling=-3.0, **kw), plain)
    assert capi.CALLS - before == calls and tts.last_loudness is None  # no launch is added
    before = capi.CALLS
    loud = tts(PHONES[2], loudness=TARGET, **kw)
    assert capi.CALLS - before == calls + 3 and loud.shape == plain.shape and loud.dtype == torch.float32
    assert tts.last_loudness.shape == (1, 8) and tts.last_loudness.dtype == torch.float64 and tts.last_loudness.is_cuda
    row = check_rows(tts.last_loudness, [loud])[0]
    print("forward:", dict(zip(loudness.LOUDNESS_COLUMNS, row.tolist())))
    assert torch.equal(loud, plain * torch.tensor(row[COL["gain"]], dtype=torch.float32, device=plain.device))


def test_interface_batch_equals_forward_per_utterance(tts):
    dz = [gold(tts, p, seed=s) for s, p in enumerate(PHONES)]
    batch = tts.synthesize_batch(PHONES, durations=[d for d, _ in dz], z_noise=[z for _, z in dz], loudness=TARGET)
    rows = tts.last_loudness.clone()
    assert rows.shape == (3, 8)
    check_rows(rows, batch)
    for u, (p, (d, z)) in enumerate(zip(PHONES, dz)):
        one = tts(p, input_is_phones=True, durations=d, z_noise=z, loudness=TARGET)
        assert torch.equal(one, batch[u]) and torch.equal(tts.last_loudness[0], rows[u]), u


def test_interface_16_khz_pcm16_is_the_resampler_on_the_normalised_wave(tts):
    dz = [gold(tts, p, seed=s) for s, p in enumerate(PHONES)]
    kw = dict(durations=[d for d, _ in dz], z_noise=[z for _, z in dz])
    norm24 = tts.synthesize_batch(PHONES, loudness=TARGET, peak_ceiling=-2.0, **kw)
    rows = tts.last_loudness.clone()
    got = tts.synthesize_batch(PHONES, sample_rate=16000, pcm16=True, loudness=TARGET, peak_ceiling=-2.0, **kw)
    assert torch.equal(tts.last_loudness, rows)
    spans, at = [], 0
    for w in norm24:
        spans.append((at, w.numel()))
        at += w.numel()
    want, out_spans = resample.Resampler(DEV).resample(torch.cat(norm24), spans, 24000, 16000, pcm16=True)
    for g, (b, n) in zip(got, out_spans):
        assert g.dtype == torch.int16 and torch.equal(g, want[b:b + n])
    # the ensemble normalises its mean
    d0, z0 = gold(tts, PHONES[0])
    voices = dict(utterance_embeddings=[tts.default_utterance_embedding, tts.default_utterance_embedding * 0.5], durations=d0, z_noise=[z0] * 2)
    mean = tts.synthesize_ensemble(PHONES[0], **voices)
    ens = tts.synthesize_ensemble(PHONES[0], loudness=-30.0, **voices)
    row = check_rows(tts.last_loudness, [ens], target=-30.0)[0]
    assert torch.equal(ens, mean * torch.tensor(row[COL["gain"]], dtype=torch.float32, device=mean.device))


def test_interface_grid_variants_come_out_at_the_target(tts):
    d, z = gold(tts, PHONES[2])
    kw = dict(durations=d, z_noise=[z, z])
    plain = tts.synthesize_grid(PHONES[2], energy_variance_scales=(1.0, 2.5), **kw)
    grid = tts.synthesize_grid(PHONES[2], energy_variance_scales=(1.0, 2.5), loudness=TARGET, **kw)
    assert len(grid) == 2 and all("loudness" not in v for v in plain) and tts.last_loudness.shape == (2, 8)
    rows = check_rows(torch.stack([v["loudness"] for v in grid]), [v["wave"] for v in grid])
    assert torch.equal(torch.stack([v["loudness"] for v in grid]), tts.last_loudness)
    for v, p, row in zip(grid, plain, rows):
        assert torch.equal(v["wave"], p["wave"] * torch.tensor(row[COL["gain"]], dtype=torch.float32, device=p["wave"].device))
    print("grid: loudness before", rows[:, COL["lufs"]].tolist(), "after", rows[:, COL["lufs_after"]].tolist(), "gain", rows[:, COL["gain"]].tolist())


def test_interface_read_to_file_normalises_every_sentence(tts, tmp_path):
    out = tmp_path / "loud.wav"
    texts = [PHONES[0], "", PHONES[2]]
    d = [gold(tts, PHONES[0])[0], None, gold(tts, PHONES[2])[0]]
    tts.read_to_file(texts, str(out), silent=True, input_is_phones=True, dur_list=d, loudness=TARGET, peak_ceiling=-1.0)
    rows = tts.last_loudness.cpu().numpy()
    assert rows.shape == (2, 8)
    with wave.open(str(out)) as f:
        assert f.getframerate() == 24000 and f.getsampwidth() == 2
        data = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.float32) / 32768.0
    gap, at, spans = tts.SILENCE_SAMPLES, tts.SILENCE_SAMPLES, []
    for w in tts.synthesize_batch([PHONES[0], PHONES[2]], durations=[d[0], d[2]]):  # (word boundaries get no frames)
        spans.append((at, w.numel()))
        at += spans[-1][1] + gap
    assert at == len(data)
    # the file holds 16-bit integers: a sentence read back sits within the quantisation of where its row says (far below 0.01 LU)
    again = meter().measure(torch.from_numpy(data).to(DEV), spans + [(0, len(data))], 24000).cpu().numpy()
    for row, now in zip(rows, again[:2]):
        assert math.isfinite(row[COL["lufs_after"]]) and abs(now[COL["lufs"]] - row[COL["lufs_after"]]) < 0.01
    print("read_to_file: sentences", rows[:, COL["lufs_after"]].tolist(), "file", again[2, COL["lufs"]])
    # the file as a whole: the silences are gated out, the blocks that straddle the edge of a sentence (a quarter, a half or three
    # quarters of their power) are not - they are less than 10 LU down - so the file reads somewhat below its sentences, and never
    # 10 LU below them: the relative gate drops what lies that far under the mean
    if all(abs(r[COL["lufs_after"]] - TARGET) < 1e-5 for r in rows):
        assert TARGET - 10.0 < again[2, COL["lufs"]] < TARGET + 1.0
    with pytest.raises(ValueError, match="increased_compatibility_mode"):
        tts.read_to_file(texts, str(out), silent=True, input_is_phones=True, increased_compatibility_mode=True, loudness=TARGET)
    assert all(r[COL["peak"]] * r[COL["gain"]] <= CEIL_LIN for r in rows)


def test_interface_refuses_what_cannot_be_normalised(tts):
    with pytest.raises(ValueError, match="whole utterance"):
        next(tts.stream(PHONES[0], input_is_phones=True, loudness=TARGET))
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch(PHONES, distributed=True, loudness=TARGET)
    with pytest.raises(ValueError, match="finite"):
        tts(PHONES[0], input_is_phones=True, loudness=float("nan"))
    with pytest.raises(ValueError, match="above full scale"):
        tts.synthesize_grid(PHONES[0], loudness=TARGET, peak_ceiling=1.0)
