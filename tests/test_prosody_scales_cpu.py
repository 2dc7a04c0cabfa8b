"""Per-utterance prosody scales without a GPU: the float64 restatement (tests/prosody_ref.py) against the oracle, its statistics on
hand-made vectors, header / binding / library agreement, the interface's validation, and synthesize_grid's order and chunking on a
stub pipeline."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, interface, prosody
from oracle import toucan_oracle as orc
from tests import abi_emulator, prosody_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PHONES_A = "~həlˈoʊ wˈɜːld~#"
PHONES_B = "~tˈɛst~#"
EPS32 = 2.0 ** -23


def _random_batch(lengths, seed, unvoiced=()):
    rng = np.random.default_rng(seed)
    R = sum(lengths)
    text = np.zeros((R, 62), dtype=np.float32)
    text[:, ref.F_VOICED] = rng.random(R) < 0.6
    text[:, ref.F_PHONEME] = rng.random(R) < 0.8
    text[:, ref.F_WORD_BOUNDARY] = rng.random(R) < 0.15
    text[:, ref.F_SILENCE] = rng.random(R) < 0.2
    b0 = 0
    for u, n in enumerate(lengths):
        if u in unvoiced:
            text[b0:b0 + n, ref.F_VOICED] = 0
        b0 += n
    pitch = (0.3 + 0.5 * rng.standard_normal(R)).astype(np.float32)  # (spread over the mean: the clamp at 0 bites)
    energy = (0.5 + 0.4 * rng.standard_normal(R)).astype(np.float32)
    dur = rng.integers(0, 13, R).astype(np.int64)
    return text, pitch, energy, dur


def test_restatement_equals_the_oracle_per_utterance():
    """prosody_ref.control with per-utterance scales == oracle.toucan_oracle.control run on every utterance alone with its scalars:
    the durations are equal; pitch and energy agree to the fp32 rounding of the oracle's own arithmetic.  Bound: the oracle's mean of
    n fp32 values is off by at most n eps max|v|, which (v - avg) s + avg passes on times |1 - s| <= 1 + |s|; its three fp32 roundings
    add eps (|v| + |avg|) (1 + |s|) each at most: (n + 6) eps (1 + |s|) max|v| in all, eps = 2^-23."""
    lengths = [1, 7, 33, 12, 64]
    scales = np.array([(1.0, 1.3, 1.0, 0.7), (0.9, 1.0, 0.8, 1.0), (1.2, 1.5, 1.0, 1.3), (1.0, 1.0, 1.0, 1.0), (1.5, 0.6, 2.0, 0.5)], dtype=np.float32)
    text, pitch, energy, dur = _random_batch(lengths, 11, unvoiced=(2,))
    gp, ge, gd = ref.control(text, pitch, energy, dur, lengths, scales)
    b0 = 0
    for u, n in enumerate(lengths):
        sl = slice(b0, b0 + n)
        op, oe, od = orc.control(torch.from_numpy(text[sl]), torch.from_numpy(pitch[sl]), torch.from_numpy(energy[sl]), torch.from_numpy(dur[sl]),
                                 *[float(s) for s in scales[u]])
        assert np.array_equal(gd[sl], od.numpy()), u
        for got, want, raw, s in ((gp[sl], op.numpy(), pitch[sl], scales[u, 1]), (ge[sl], oe.numpy(), energy[sl], scales[u, 2])):
            assert np.array_equal(np.isnan(got), np.isnan(want)), u
            tol = (n + 6) * EPS32 * (1 + abs(float(s))) * float(np.abs(raw).max())
            ok = ~np.isnan(want)
            assert np.all(np.abs(got[ok] - want[ok]) <= tol), (u, float(np.abs(got[ok] - want[ok]).max()), tol)
        b0 += n
    assert np.isnan(gp[8:41]).all()  # utterance 2 has no voiced phoneme and a pitch scale of 1.5: the mean of nothing
    # scales None: the overrides alone, the same as every scale 1
    ones = np.ones((len(lengths), 4), dtype=np.float32)
    for a, b in zip(ref.control(text, pitch, energy, dur, lengths, None), ref.control(text, pitch, energy, dur, lengths, ones)):
        assert np.array_equal(a, b)


def test_statistics_on_hand_made_vectors():
    z = np.zeros(5)
    assert np.array_equal(ref.stats_one(z, z, np.zeros(5, dtype=np.int64)), [0, 0, 0, 0, 0, 0, 0, 5])  # nothing non-zero: means and variances 0
    row = ref.stats_one(np.array([0, 0, 2.5, 0]), np.array([0, -1.5, 0, 0]), np.array([3, 0, 4, 1]))
    assert np.array_equal(row, [1, 2.5, 0, 1, -1.5, 0, 8, 4])  # one entry: its own mean, variance 0
    row = ref.stats_one(np.array([1.0, 0, 3.0, 5.0]), np.array([2.0, 2.0, 0, 4.0]), np.array([1, 2, 3, 4]))
    assert np.allclose(row, [3, 3.0, 8.0 / 3.0, 3, 8.0 / 3.0, 8.0 / 9.0, 10, 4], rtol=1e-15)
    # no entry clamps and the zero stays zero (it lands below 0 and is clamped back): the realised variance ratio is scale^2
    before = np.array([0.0, 0.9, 1.0, 1.1])
    after = ref.scale_variance(before, 1.5)
    assert after[0] == 0.0 and (after[1:] > 0).all()
    assert ref.stats_one(after, z[:4], z[:4])[2] / ref.stats_one(before, z[:4], z[:4])[2] == pytest.approx(1.5 ** 2, rel=1e-12)
    # the clamp bites: 0.1 goes to 0 and leaves the statistics, the realised ratio stays below scale^2
    before = np.array([0.1, 0.9, 1.0, 1.1, 2.0])
    after = ref.scale_variance(before, 3.0)
    assert after[0] == 0.0 and ref.stats_one(after, z, z)[0] == 4
    assert ref.stats_one(after, z, z)[2] / ref.stats_one(before, z, z)[2] < 3.0 ** 2
    # a scale below 1 shifts the zeros up: they become entries
    assert ref.stats_one(ref.scale_variance(np.array([0.0, 1.0, 3.0]), 0.5), z[:3], z[:3])[0] == 3
    assert np.array_equal(ref.stats(np.array([1.0, 0, 2.0]), np.zeros(3), np.array([1, 1, 1]), [1, 2])[:, [0, 1, 6, 7]], [[1, 1, 1, 1], [1, 2, 2, 2]])


def test_prosody_header_binding_and_library_agree():
    """include/toucan_prosody.h, capi.PROSODY_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set; none of them
    is declared in toucan_tts.h (whose kernel entries all have an emulator method) and the ABI version stays."""
    root = os.path.dirname(HERE)
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", name), encoding="utf-8").read(), flags=re.S)
    text = strip("toucan_prosody.h")
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.PROSODY_PROTOTYPES) == ["tts_control_and_regulate_v", "tts_copy_prosody_stats", "tts_prosody_control_v", "tts_prosody_stats"]
    assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", strip("toucan_tts.h")))
    assert not set(declared) & set(capi.PROTOTYPES)
    macros = dict(re.findall(r"#define\s+(TTS_PROSODY_[A-Z_]+)\s+(\d+)", text))
    assert {k: int(v) for k, v in macros.items()} == {"TTS_PROSODY_SCALES": capi.PROSODY_SCALES, "TTS_PROSODY_STATS": capi.PROSODY_STATS}
    assert len(prosody.KNOBS) == capi.PROSODY_SCALES and len(prosody.STATS) == capi.PROSODY_STATS
    for arg_list, name in zip(re.findall(r"\bint\s+tts_[a-z0-9_]+\s*\((.*?)\)\s*;", text, flags=re.S), re.findall(r"\bint\s+(tts_[a-z0-9_]+)\s*\(", text)):
        assert len(arg_list.split(",")) == len(capi.PROSODY_PROTOTYPES[name][1]), name
    assert "prosody.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        assert hasattr(handle, n) and getattr(handle, n).argtypes == capi.PROSODY_PROTOTYPES[n][1], n
    assert handle.tts_abi_version() == 15


def test_stage_entry_checks_its_arguments_without_a_gpu():
    """tts_control_and_regulate_v / tts_copy_prosody_stats on a handle with no batch in flight: error codes and messages."""
    lib = capi.lib()
    assert isinstance(lib, ctypes.CDLL)
    h = ctypes.c_void_p()
    cfg = capi.TtsConfig(1, 1, 0, 0, 0, 0.0)
    assert lib.tts_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    scales = (ctypes.c_float * 4)(1, 1, 1, 1)
    assert lib.tts_control_and_regulate_v(h, scales, None, None) != 0 and b"tts_encoder" in lib.tts_last_error()
    out = (ctypes.c_float * 8)()
    assert lib.tts_copy_prosody_stats(h, out, out, None) != 0 and b"tts_control_and_regulate_v" in lib.tts_last_error()
    assert lib.tts_prosody_stats(None, None, None, None, None, 0, None, None) == 0  # (an empty batch launches nothing)
    assert lib.tts_prosody_control_v(None, 62, None, None, None, None, None, 2, None, None) != 0 and b"null" in lib.tts_last_error()
    assert lib.tts_destroy(h) == 0


def test_resolve_scales_and_grid():
    assert prosody.resolve_scales(3, 1.0, 1.2, 0.8, 1.0) is None  # all scalars: the scalar entries serve the call
    t = prosody.resolve_scales(3, [0.9, 1.0, 1.1], 1.5, (1.0, 0.8, 1.0), np.float32(1.25))
    assert t.dtype == np.float32 and t.tolist() == np.array([[0.9, 1.5, 1.0, 1.25], [1.0, 1.5, 0.8, 1.25], [1.1, 1.5, 1.0, 1.25]], dtype=np.float32).tolist()
    assert prosody.resolve_scales(2, torch.tensor([1.0, 2.0]))[:, 0].tolist() == [1.0, 2.0]
    with pytest.raises(ValueError, match="pitch_variance_scale"):
        prosody.resolve_scales(3, 1.0, [1.0, 2.0])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="utterance 1"):
            prosody.resolve_scales(2, [1.0, bad])
    g = prosody.grid((0.9, 1.0, 1.1), (1.0, 1.5), (0.8, 1.0))
    assert g == [(d, p, e, 1.0) for d in (0.9, 1.0, 1.1) for p in (1.0, 1.5) for e in (0.8, 1.0)] and len(g) == 12
    with pytest.raises(ValueError):
        prosody.grid(())


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


def test_interface_validates_per_utterance_scales(tts):
    with pytest.raises(ValueError, match="energy_variance_scale"):
        tts.synthesize_batch([PHONES_A, PHONES_B], energy_variance_scale=[1.0, 1.1, 1.2])
    with pytest.raises(ValueError, match="utterance 1"):
        tts.synthesize_batch([PHONES_A, PHONES_B], duration_scaling_factor=[1.0, 0.0])
    with pytest.raises(ValueError, match="utterance 0"):
        tts.synthesize_batch([PHONES_A, PHONES_B], duration_scaling_factor=[-0.5, 1.0], pitch_variance_scale=1.2)
    with pytest.raises(ValueError, match="distributed"):
        tts.synthesize_batch([PHONES_A, PHONES_B], pitch_variance_scale=[1.0, 1.2], distributed=True)
    with pytest.raises(ValueError, match="utterance 2"):
        tts.synthesize_grid(PHONES_B, duration_scaling_factors=(1.0, 0.5, -1.0))
    with pytest.raises(ValueError, match="z_noise"):
        tts.synthesize_grid(PHONES_B, pitch_variance_scales=(1.0, 1.2), z_noise=[torch.zeros(80, 10)])
    assert tts.last_prosody_stats is None


class StubPipe:
    """Stands in for native.NativePipeline.forward: two frames per variant, the wave of the k-th variant it ever saw filled with k,
    the variant's four scales in the first columns of its statistics rows."""

    def __init__(self):
        self.calls, self.seen = [], 0

    def forward(self, phones, emb, lang_ids, z_noise=None, durations=None, pitch=None, energy=None, **kw):
        n = len(phones)
        table = prosody.resolve_scales(n, **kw)
        assert table is not None, "a grid goes through the per-utterance path"
        assert all(torch.equal(p, phones[0]) for p in phones) and tuple(emb.shape) == (n, 64)
        self.calls.append(dict(n=n, z=z_noise, durations=durations, table=table))
        wav = torch.cat([torch.full((768,), float(self.seen + i)) for i in range(n)])
        self.seen += n
        before = np.concatenate([table, np.zeros((n, 4), dtype=np.float32)], axis=1)
        per = [torch.zeros(1)] * n
        return dict(wav=wav, wav_spans=[(768 * i, 768) for i in range(n)], durations=per, pitch=per, energy=per, mel=per,
                    prosody_stats=(before, before + 100))


def test_grid_order_and_chunking_on_a_stub_pipeline(tts):
    tts.pipe = stub = StubPipe()
    D, P, E = (0.9, 1.0, 1.1), (1.0, 1.5), (0.8, 1.0)
    res = tts.synthesize_grid(PHONES_B, D, P, E)
    want = [(d, p, e, 1.0) for d in D for p in P for e in E]  # row-major: the first tuple varies slowest
    assert len(res) == 12 and [r["scales"] for r in res] == want and [c["n"] for c in stub.calls] == [12]
    for k, r in enumerate(res):
        assert r["frames"] == 2 and r["wave"].shape == (768,) and float(r["wave"][0]) == k
        assert np.array_equal(r["stats_before"][:4], np.float32(want[k])) and np.array_equal(r["stats_after"][:4], np.float32(want[k]) + 100)
    # larger than MAX_FILE_BATCH: split, the results in order; z_noise and gold durations follow their variants
    tts.pipe = stub = StubPipe()
    axes = ((0.9, 1.0, 1.1), (1.0, 1.2, 1.5), (0.8, 1.0, 1.2, 1.4), (1.0, 1.3))
    z = [torch.full((80, 4), float(k)) for k in range(72)]
    gold = torch.full((int(tts.text2phone.string_to_tensor(PHONES_B, input_phonemes=True).shape[0]),), 2, dtype=torch.long)
    res = tts.synthesize_grid(PHONES_B, *axes, z_noise=z, durations=gold)
    assert tts.MAX_FILE_BATCH == 32 and [c["n"] for c in stub.calls] == [32, 32, 8]
    want = prosody.grid(*axes)
    assert want[1] == (0.9, 1.0, 0.8, 1.3) and want[8] == (0.9, 1.2, 0.8, 1.0)  # the pause factor varies fastest
    assert [r["scales"] for r in res] == want and [float(r["wave"][0]) for r in res] == list(range(72))
    assert [float(zz[0, 0]) for c in stub.calls for zz in c["z"]] == list(range(72))
    assert all(len(c["durations"]) == c["n"] and torch.equal(c["durations"][0], gold) for c in stub.calls)
    assert np.array_equal(np.concatenate([c["table"] for c in stub.calls]), np.float32(want))
    # sample_rate / pcm16 are refused before anything runs when the rate cannot be served
    with pytest.raises(ValueError):
        tts.synthesize_grid(PHONES_B, sample_rate=-1)
