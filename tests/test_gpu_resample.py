"""The sample-rate converter (csrc/resample.hip) on the MI355X: against the float64 restatement within the derived bound of
tests/resample_ref.py at every output (and the restatement with its phases rotated by one must miss that bound), a ragged batch
against its utterances alone, the streamer against the whole, PCM16 against float2pcm of the float32 result, and the interface's
``sample_rate`` / ``pcm16`` keywords.

Worst error / bound per conversion measured on the MI355X is recorded in DESIGN.md section 13."""
import functools
import wave

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, interface, resample
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = sorted(rr.RATIOS)


@functools.lru_cache(maxsize=None)
def resampler():
    return resample.Resampler(DEV)


def tile():
    return int(capi.lib().tts_resample_tile_outputs())


@functools.lru_cache(maxsize=None)
def batch_on_device(sr_in, sr_out, pcm16):
    """Every length of one conversion as ONE ragged launch -> the outputs per utterance on the host."""
    cases = rr.cases(sr_in, sr_out, tile())
    begins = np.concatenate([[0], np.cumsum([c["n"] for c in cases])[:-1]])
    wave_d = torch.from_numpy(np.concatenate([c["x"] for c in cases])).to(DEV)
    y, at = resampler().launch(wave_d, [(int(b), c["n"], 0, 0, c["count"]) for b, c in zip(begins, cases)], sr_in, sr_out, pcm16)
    y = y.cpu().numpy()
    assert y.dtype == (np.int16 if pcm16 else np.float32)
    return [y[a:a + c["count"]] for a, c in zip(at, cases)]


def test_the_tile_and_the_lengths_aim_at_its_edges():
    T = tile()
    assert T == 1024
    for sr_in, sr_out in ALL:
        counts = [c["count"] for c in rr.cases(sr_in, sr_out, T)]
        assert counts[4:7] == [T - 1, T, T + 1] and counts[-1] > 2 * T and len(counts) == 8


@pytest.mark.parametrize("sr_in,sr_out", ALL)
def test_kernel_against_the_float64_restatement_within_the_bound(sr_in, sr_out):
    """|y - y_ref| <= (K + 2) 2^-24 sum_j |k[p][j]| |x_j| at every output of every length; the restatement with its phases rotated
    by one is outside that bound on the same input, so the bound tells the right phase from the wrong one."""
    orig, new, K = rr.RATIOS[(sr_in, sr_out)]
    worst = 0.0
    for c, got in zip(rr.cases(sr_in, sr_out, tile()), batch_on_device(sr_in, sr_out, False)):
        assert got.shape == c["ref"].shape
        err = np.abs(got.astype(np.float64) - c["ref"])
        worst = max(worst, float((err[c["bound"] > 0] / c["bound"][c["bound"] > 0]).max(initial=0.0)))
        bad = np.flatnonzero(err > c["bound"])
        assert bad.size == 0, (c["n"], bad[:5], err[bad[:5]], c["bound"][bad[:5]])
        wrong = np.abs(c["rotated"] - c["ref"]) > c["bound"]
        assert wrong.any(), f"n = {c['n']}: the bound admits the rotated phases"
        if c["count"] >= 64:
            assert wrong.mean() > 0.9, (c["n"], wrong.mean())
    print(f"{sr_in} -> {sr_out} (orig {orig}, new {new}, K {K}): worst error / bound {worst:.4f}")


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("sr_in,sr_out", ALL)
def test_ragged_batch_equals_each_utterance_alone(sr_in, sr_out, pcm16):
    res = resampler()
    together = batch_on_device(sr_in, sr_out, pcm16)
    for c, got in zip(rr.cases(sr_in, sr_out, tile()), together):
        alone, _ = res.launch(torch.tensor(c["x"]).to(DEV), [(0, c["n"], 0, 0, c["count"])], sr_in, sr_out, pcm16)
        assert np.array_equal(alone.cpu().numpy(), got), (c["n"], pcm16)
    # the public call on whole utterances: the same outputs, as many as the length formula says
    whole = [(c, got) for c, got in zip(rr.cases(sr_in, sr_out, tile()), together) if c["count"] == resample.out_length(c["n"], sr_in, sr_out)]
    begins = np.concatenate([[0], np.cumsum([c["n"] for c, _ in whole])[:-1]])
    y, out_spans = res.resample(torch.from_numpy(np.concatenate([c["x"] for c, _ in whole])).to(DEV),
                                [(int(b), c["n"]) for b, (c, _) in zip(begins, whole)], sr_in, sr_out, pcm16)
    y = y.cpu().numpy()
    assert len(whole) >= 5 and [n for _, n in out_spans] == [c["count"] for c, _ in whole]
    for (c, got), (b, n) in zip(whole, out_spans):
        assert np.array_equal(y[b:b + n], got), c["n"]


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("sr_in,sr_out", ALL)
def test_streamer_equals_the_whole(sr_in, sr_out, pcm16):
    """Pieces of 1 000, 196 608 and one sample - none a multiple of 80, the middle one the default chunk of stream()."""
    res = resampler()
    x = torch.from_numpy(rr.noise(1000 + 196608 + 1, seed=9)).to(DEV)
    whole, spans = res.resample(x, [(0, x.numel())], sr_in, sr_out, pcm16)
    assert spans == [(0, resample.out_length(x.numel(), sr_in, sr_out))]
    st = res.streamer(sr_in, sr_out, pcm16)
    pieces = [st.push(x[:1000]), st.push(x[1000:197608]), st.push(x[197608:]), st.finish()]
    assert all(p.dtype == whole.dtype for p in pieces) and pieces[1].numel() > 0 and pieces[3].numel() > 0
    assert torch.equal(torch.cat(pieces), whole)


@pytest.mark.parametrize("sr_in,sr_out", ALL + [(24000, 24000)])
def test_pcm16_is_float2pcm_of_the_float32_result(sr_in, sr_out):
    res = resampler()
    loud = np.clip(rr.noise(5000, seed=3) * 4.0, -1.5, 1.5).astype(np.float32)  # saturates on both sides
    for x in (rr.noise(5000, seed=2), loud, rr.pcm_probe(), np.repeat(rr.pcm_probe(), 40)):
        xd = torch.from_numpy(x).to(DEV)
        f, _ = res.resample(xd, [(0, len(x))], sr_in, sr_out, False)
        q, _ = res.resample(xd, [(0, len(x))], sr_in, sr_out, True)
        f, q = f.cpu().numpy(), q.cpu().numpy()
        assert q.dtype == np.int16 and np.array_equal(q, interface.float2pcm(f))
        if sr_in == sr_out:  # the identity table: the samples themselves, so the probe's values reach the conversion exactly
            assert np.array_equal(f, x) and np.array_equal(q, rr.float2pcm_int16(x))
    assert (np.abs(interface.float2pcm(f).astype(np.int32)) >= 32767).any()


def test_the_entry_refuses_a_ratio_past_the_limit():
    res = resampler()
    with pytest.raises(ValueError, match="1024"):
        res.resample(torch.zeros(10, device=DEV), [(0, 10)], 24000, 44101)
    x, y = torch.zeros(10, device=DEV), torch.zeros(32, device=DEV)
    spans = torch.zeros(6, dtype=torch.int64, device=DEV)
    rc = res.lib.tts_resample(x.data_ptr(), x.data_ptr(), spans.data_ptr(), 1, 0, 24000, 44101, 7, 0, y.data_ptr(), None)
    assert rc == -1 and "TTS_RESAMPLE_MAX_FACTOR" in res.lib.tts_last_error().decode()


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    models = tmp_path_factory.mktemp("resample_models") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    old, interface.MODELS_DIR = interface.MODELS_DIR, str(models)
    try:
        yield interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)
    finally:
        interface.MODELS_DIR = old


PHONES = ["~həlˈoʊ~#", "~wˈɜːld tˈu~#", "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#"]


def gold(tts, phones, frames=6, seed=3):
    L = int(tts.text2phone.string_to_tensor(phones, input_phonemes=True).shape[0])
    z = torch.randn(80, frames * L, generator=torch.Generator().manual_seed(seed)) * 0.8
    return torch.full((L,), frames, dtype=torch.long), z


def test_interface_batch_at_16_khz_is_the_resampler_on_its_24_khz_result(tts):
    dz = [gold(tts, p, seed=s) for s, p in enumerate(PHONES)]
    kw = dict(durations=[d for d, _ in dz], z_noise=[z for _, z in dz])
    plain = tts.synthesize_batch(PHONES, **kw)
    at16 = tts.synthesize_batch(PHONES, sample_rate=16000, **kw)
    pcm = tts.synthesize_batch(PHONES, sample_rate=16000, pcm16=True, **kw)
    packed = torch.cat(plain)
    spans, at = [], 0
    for w in plain:
        spans.append((at, w.numel()))
        at += w.numel()
    want, out_spans = resample.Resampler(DEV).resample(packed, spans, 24000, 16000)
    assert len(at16) == len(pcm) == 3
    for w24, got, q, (b, n) in zip(plain, at16, pcm, out_spans):
        assert got.dtype == torch.float32 and got.is_cuda and got.numel() == n == -(-2 * w24.numel() // 3)
        assert torch.equal(got, want[b:b + n])
        assert q.dtype == torch.int16 and np.array_equal(q.cpu().numpy(), interface.float2pcm(got.cpu().numpy()))
    assert all(torch.equal(a, b) for a, b in zip(tts.synthesize_batch(PHONES, sample_rate=24000, **kw), plain))


def test_interface_forward_without_a_rate_is_forward(tts):
    d, z = gold(tts, PHONES[2])
    kw = dict(input_is_phones=True, durations=d, z_noise=z)
    plain = tts(PHONES[2], **kw)
    assert torch.equal(tts(PHONES[2], sample_rate=None, **kw), plain) and torch.equal(tts(PHONES[2], sample_rate=24000, **kw), plain)
    calls = []
    for rate in ("absent", None, 24000):  # the same ABI calls: no launch is added
        before = capi.CALLS
        tts(PHONES[2], **kw) if rate == "absent" else tts(PHONES[2], sample_rate=rate, **kw)
        calls.append(capi.CALLS - before)
    assert calls[0] == calls[1] == calls[2] and plain.dtype == torch.float32
    before = capi.CALLS
    up = tts(PHONES[2], sample_rate=48000, **kw)
    assert up.numel() == 2 * plain.numel() and up.dtype == torch.float32 and capi.CALLS - before == calls[0] + 1
    d0, z0 = gold(tts, PHONES[0])
    voices = dict(utterance_embeddings=[tts.default_utterance_embedding] * 2, durations=d0, z_noise=[z0] * 2)
    mean24 = tts.synthesize_ensemble(PHONES[0], **voices)
    ens = tts.synthesize_ensemble(PHONES[0], sample_rate=8000, pcm16=True, **voices)
    want, _ = resample.Resampler(DEV).resample(mean24, [(0, mean24.numel())], 24000, 8000, pcm16=True)
    assert ens.dtype == torch.int16 and ens.numel() == -(-mean24.numel() // 3) and torch.equal(ens, want)  # averaged at 24 kHz, then converted


def test_interface_stream_at_44100_equals_forward_at_44100(tts):
    phones = "~" + "wˈʌns əpˈɑːn ɐ mˈɪdnaɪt dɹˈɪɹi " * 6 + "~#"
    d, z = gold(tts, phones, frames=6)
    n24 = tts(phones, input_is_phones=True, durations=d, z_noise=z).numel()
    for pcm16 in (False, True):
        pieces = list(tts.stream(phones, input_is_phones=True, chunk_frames=128, durations=d, z_noise=z, sample_rate=44100, pcm16=pcm16))
        one = tts(phones, input_is_phones=True, durations=d, z_noise=z, sample_rate=44100, pcm16=pcm16)
        assert len(pieces) > 3 and one.numel() == resample.out_length(n24, 24000, 44100)
        assert torch.equal(torch.cat(pieces), one)


def test_interface_read_to_file_at_16_khz_pcm16(tts, tmp_path):
    out = tmp_path / "r16.wav"
    texts = [PHONES[0], "", PHONES[1]]
    d = [gold(tts, PHONES[0])[0], None, gold(tts, PHONES[1])[0]]
    tts.read_to_file(texts, str(out), silent=True, input_is_phones=True, dur_list=d, sample_rate=16000, pcm16=True)
    gap = -(-10600 * 2 // 3)
    n24 = [w.numel() for w in tts.synthesize_batch([PHONES[0], PHONES[1]], durations=[d[0], d[2]])]  # (word boundaries get no frames)
    want = gap + sum(-(-2 * n // 3) + gap for n in n24)
    with wave.open(str(out)) as f:
        assert f.getframerate() == 16000 and f.getsampwidth() == 2 and f.getnchannels() == 1 and f.getnframes() == want
        data = np.frombuffer(f.readframes(want), dtype="<i2")
    assert not data[:gap].any() and not data[-gap:].any() and data[gap:gap + 2000].any()
    with pytest.raises(ValueError):
        tts.read_to_file(texts, str(out), silent=True, input_is_phones=True, increased_compatibility_mode=True, sample_rate=16000)
