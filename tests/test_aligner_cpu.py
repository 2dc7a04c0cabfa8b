"""The prosody cloner's extraction path on the CPU: the MAS + post-processing restatement and pack_aligner's folded weights against
the reference goldens (tests/golden/aligner/aligner.npz, made by make_aligner_golden.py from the reference's own code), the aligner token
ids against the reference's text_vectors_to_id_sequence, the fixture checkpoint, and align.py's host sequencing end to end on the
numpy ABI emulator."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, build, capi, fixture_weights as fw, phonemes
from tests import aligner_emulator
from tests import aligner_ref as ar

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "aligner", "aligner.npz"))
N_MAS = len(G["mas_cases"])
N_CLONE = len(G["clone_phones"])


STORED = [c for c in range(N_MAS) if f"mas{c}_logits" in G.files]  # the long case keeps its durations only


def mas_mel(c):
    return fw.aligner_spectrogram(int(G[f"mas{c}_seed"]), int(G["mas_cases"][c][0]))


def clone_wave(u):
    """The recording of clone case u and its normalised 16 kHz form (what extract_prosody aligns)."""
    from ims_toucan_prosody_variance_amd import style
    wave = fw.reference_wave(int(G[f"clone{u}_seed"]), int(G[f"clone{u}_samples"]))
    return wave, style.normalize_reference_audio(wave, 16000)


@pytest.fixture(scope="module")
def packed():
    return align.pack_aligner(fw.aligner_state_dict())


@pytest.mark.parametrize("c", STORED)
def test_mas_restatement_reproduces_the_reference(c):
    ids, logits = G[f"mas{c}_ids"], G[f"mas{c}_logits"]
    for log64 in (False, True):  # numpy's float32 log (the reference's) and the correctly rounded one the kernel uses
        assert np.array_equal(ar.mas(logits[:, ids], log64=log64)[0], G[f"mas{c}_dur"])
    assert G[f"mas{c}_dur"].sum() == logits.shape[0]


def test_long_case_durations_from_the_restated_aligner(packed):
    """T ~ 4000: the golden keeps the reference's durations only; the folded-weight restatement's logits give them exactly."""
    c = N_MAS - 1
    assert c not in STORED and G["mas_cases"][c][0] > 3000
    logits = ar.aligner_logits(packed, mas_mel(c))
    assert np.array_equal(ar.mas(logits[:, G[f"mas{c}_ids"]], log64=True)[0], G[f"mas{c}_dur"])


def test_mas_restatement_on_exact_ties():
    k = 0
    while f"tie{k}_p" in G.files:
        assert np.array_equal(ar.mas(G[f"tie{k}_p"])[0], G[f"tie{k}_dur"]), k
        k += 1
    assert k >= 5


@pytest.mark.parametrize("u", range(N_CLONE))
def test_duration_postprocessing_reproduces_extract_prosody(packed, u):
    feats = phonemes.phones_to_features(str(G["clone_phones"][u]), handle_missing=False)
    ids, flags = align.token_ids(feats)
    assert np.array_equal(flags, ar.flags_of(feats))
    assert (flags & 1).any() and ((flags & 2).any() or u == 0)  # cases 1 and 2 also repeat phonemes (2 and 3 in a row)
    nb = ar.mas(ar.aligner_logits(packed, G[f"clone{u}_mel"])[:, ids])[0]
    dur = ar.postprocess(nb, flags)
    assert np.array_equal(dur, G[f"clone{u}_dur"])
    assert dur[(flags & 1) != 0].sum() == 0


@pytest.mark.parametrize("c", STORED)
def test_folded_aligner_weights_reproduce_the_reference_logits(packed, c):
    """pack_aligner (BatchNorm 1-4 as scale / shift after the ReLU, BatchNorm 5 and both LSTM biases folded into the input
    projection) run through torch.nn == the reference Aligner's logits."""
    ref = G[f"mas{c}_logits"]
    out = ar.aligner_logits(packed, mas_mel(c))
    assert float(np.abs(out - ref).max()) <= 1e-5 * float(np.abs(ref).max())


def test_pack_aligner_layout(packed):
    sd = fw.aligner_state_dict()
    H = 512
    assert packed["hidden"] == H and packed["w_ih"].shape == (2, 4 * H, 512) and packed["w_hh_t"].shape == (2, H, 4 * H)
    assert len(packed["conv_w"]) == 5 and len(packed["bn_scale"]) == 4
    assert np.array_equal(packed["w_hh_t"][1], sd["rnn.weight_hh_l0_reverse"].T)
    for i in range(5):
        assert (sd[f"convs.{2 * i}.bnorm.running_var"] > 0).all()


def test_token_ids_match_the_reference_lookup():
    cases = json.load(open(os.path.join(HERE, "golden", "aligner", "aligner_ids.json"), encoding="utf-8"))["cases"]
    assert len(cases) >= 10
    for c in cases:
        ids, flags = align.token_ids(phonemes.phones_to_features(c["phones"], handle_missing=True))
        assert ids.tolist() == c["ids"], c["phones"]
    # nasal vowels take their plain vowel's id; word boundaries are dropped; modifiers do not matter
    a = align.token_ids(phonemes.phones_to_features("a ã ˈaː", handle_missing=False))[0]
    assert a.tolist() == [a[0]] * 3


def test_token_averages_follow_the_reference_rules():
    x = np.float32([1, 2, 0, 4, 0, 0, 6, 8])
    d = [2, 3, 0, 3]
    e = ar.token_average(x, d, [True, True, True, False], 0)
    np.testing.assert_allclose(e * np.mean([1.5, 4 / 3]), [1.5, 4 / 3, 0, 0], rtol=1e-6)
    p = ar.token_average(x, d, [True, True, True, True], 1)
    np.testing.assert_allclose(p * np.mean([1.5, 4.0, 7.0]), [1.5, 4.0, 0, 7.0], rtol=1e-6)
    np.testing.assert_array_equal(ar.adjust_centered(np.ones(3), 6), [0, 0, 1, 1, 1, 0])


def test_aligner_checkpoint_writer_and_weights_only_load(tmp_path):
    from ims_toucan_prosody_variance_amd import interface
    path = interface.write_fixture_aligner_checkpoint(str(tmp_path / "Models"))
    assert path.endswith(os.path.join("Aligner", "aligner.pt"))
    ck = torch.load(path, map_location="cpu", weights_only=True)
    sd = fw.aligner_state_dict()
    assert sorted(ck["asr_model"]) == sorted(sd)
    for k, v in sd.items():
        assert np.array_equal(ck["asr_model"][k].numpy(), np.asarray(v)), k


def test_host_path_on_the_emulator_reproduces_the_golden(monkeypatch):
    """align.py's sequencing (conv stack, folded projection, per-step recurrence with ping-pong state, MAS, frame energy, token
    averages) on the numpy ABI emulator, for two clone cases in one ragged batch, fed the golden mel and normalised wave."""
    aligner_emulator.install(monkeypatch)
    ex = align.ProsodyExtractor(fw.aligner_state_dict(), "cpu")
    us = [0, 2]
    feats = [phonemes.phones_to_features(str(G["clone_phones"][u]), handle_missing=False) for u in us]
    res = ex.extract(feats, [clone_wave(u)[1] for u in us], f0=[G[f"clone{u}_f0"] for u in us], mels=[G[f"clone{u}_mel"] for u in us])
    for (d, p, e), u in zip(res, us):
        assert np.array_equal(d.numpy(), G[f"clone{u}_dur"]), u
        assert float(np.abs(e.numpy() - G[f"clone{u}_energy"]).max()) <= 1e-5
        assert float(np.abs(p.numpy() - G[f"clone{u}_pitch"]).max()) <= 1e-5


def test_align_header_binding_library_and_emulator_agree():
    """include/toucan_align.h, capi.ALIGN_PROTOTYPES, the symbols libtoucan_hip.so exports and the CPU emulator's entry points are
    the same set; the cloner's entries do not appear in toucan_tts.h's binding."""
    root = os.path.dirname(HERE)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "toucan_align.h"), encoding="utf-8").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert len(declared) == 5 and sorted(capi.ALIGN_PROTOTYPES) == declared
    assert not set(declared) & set(capi.PROTOTYPES)
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    emu = aligner_emulator.AlignerEmulator()
    for n in declared:
        assert hasattr(handle, n) and getattr(handle, n).argtypes == capi.ALIGN_PROTOTYPES[n][1], n
        assert hasattr(emu, n), n
