"""The aligner's on-line fine-tuning on the CPU: the autograd yardstick (tests/finetune_ref.py) against the reference goldens
(tests/golden/aligner/finetune.npz, made by make_finetune_golden.py from the reference's own loop), the dropout-mask recipe, finetune.py's
sequencing end to end on the numpy ABI emulator, the cloner's keywords, and the binding of include/toucan_train.h."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, build, capi, cloner as cloner_mod, finetune, fixture_weights as fw, interface
from tests import aligner_ref as ar
from tests import finetune_emulator
from tests import finetune_ref as fr

from tests.finetune_cases import G, N, case, check_against_golden, tol, yardstick

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("c", range(N))
def test_yardstick_reproduces_the_reference_loop(c):
    r = yardstick(c)
    stat = lambda k: np.stack([r["state"][f"convs.{2 * i}.bnorm.{k}"] for i in range(5)])
    check_against_golden(c, r["logits"], r["loss"], r["norm"], stat("running_mean"), stat("running_var"))
    assert G[f"ft{c}_sens"] <= 1e-4 and (G[f"ft{c}_norm"] > 1.0).all()  # the maker's selection; clipping active in every step


def test_fine_tuning_is_observable_on_the_goldens():
    """The feature changes the result: the eval-mode logits move by more than 1 (2.6 - 2.8, printed by the golden maker; the comparison tolerance
    is five orders of magnitude below), mostly through the running statistics."""
    packed = align.pack_aligner(fw.aligner_state_dict())
    for c in range(N):
        before = ar.aligner_logits(packed, case(c)[0])
        assert float(np.abs(G[f"ft{c}_logits"] - before).max()) > 1.0
    assert float(np.abs(G["ft0_running_mean"][0] - fw.aligner_state_dict()["convs.0.bnorm.running_mean"]).max()) > 1.0
    flags = G[f"ft{N - 1}_flags"]
    assert (flags & 1).any() and (flags & 2).any()  # the last case: word boundaries and a repeated phoneme


@pytest.mark.parametrize("c", range(N))
def test_mask_recipe_reproduces_the_stored_masks(c):
    T = int(G[f"ft{c}_frames"])
    drawn = np.stack([np.stack(s) for s in finetune.dropout_masks(int(G[f"ft{c}_seed"]), T)])
    assert drawn.shape == (5, 5, T, 512) and np.array_equal(drawn, case(c)[2])
    assert 0.45 < drawn.mean() < 0.55
    # the recipe's point: a contiguous [1, T, 512] draw from the same generator state is another mask
    gen = torch.Generator().manual_seed(int(G[f"ft{c}_seed"]))
    assert not np.array_equal(torch.empty(1, T, 512).bernoulli_(0.5, generator=gen)[0].numpy() != 0, drawn[0, 0])


def test_parameter_arena_round_trip():
    sd = fw.aligner_state_dict()
    theta, stats = finetune.pack_parameters(sd)
    assert theta.shape == (finetune.N_PARAMS,) and stats.shape == (2, 5, 512)
    back = finetune.unpack_parameters(theta, stats)
    for k in fr.PARAM_KEYS + fr.STAT_KEYS:
        assert np.array_equal(back[k], np.asarray(sd[k])), k
    assert sorted(k for k in sd if "num_batches_tracked" not in k) == sorted(back)


def test_emulator_path_equals_the_yardstick():
    """finetune.py's sequencing on the hand-written closed forms of the emulator == autograd on the whole model (float32 buffers
    between the emulator's entries: the golden's tolerance), and the golden itself."""
    c = 0
    mel, ids, masks = case(c)
    ft = finetune.AlignerFineTuner(fw.aligner_state_dict(), "cpu", lib=finetune_emulator.FineTuneEmulator())
    logits = ft.fine_tune(mel, ids, masks).numpy()
    r = yardstick(c)
    top = float(np.abs(r["logits"]).max())
    assert float(np.abs(logits - r["logits"]).max()) / top <= tol(c)
    assert float(np.abs(ft.last_loss.numpy() - r["loss"]).max() / r["loss"].max()) <= tol(c)
    assert float(np.abs(ft.last_norm.numpy() - r["norm"]).max() / r["norm"].max()) <= tol(c)
    got = finetune.unpack_parameters(ft.theta.numpy(), ft.stats.numpy())
    sd = fw.aligner_state_dict()
    for k in fr.PARAM_KEYS + fr.STAT_KEYS:  # every parameter and statistic, relative to how far the five steps moved it
        moved = float(np.abs(r["state"][k] - np.asarray(sd[k])).max())
        assert moved > 0 and float(np.abs(got[k] - r["state"][k]).max()) <= 1e-3 * moved + 1e-7, k
    check_against_golden(c, logits, ft.last_loss.numpy(), ft.last_norm.numpy(), ft.stats[0].numpy(), ft.stats[1].numpy())
    # the checkpoint's copy is never written
    theta0, stats0 = finetune.pack_parameters(sd)
    assert np.array_equal(ft.theta0.numpy(), theta0) and np.array_equal(ft.stats0.numpy(), stats0)


def test_unclipped_branch_and_kernel_math_of_the_yardstick():
    """clip_update below and above norm 1, and lstm_loop == torch.nn.LSTM (it supplies the gate gradients the module hides)."""
    rng = np.random.default_rng(5)
    p, g = rng.standard_normal(1000), rng.standard_normal(1000)
    small = g * (0.5 / np.linalg.norm(g))
    n, q = fr.clip_update(p, small)
    assert abs(n - 0.5) < 1e-12 and np.allclose(q, p - 0.1 * small, rtol=0, atol=1e-15)
    n, q = fr.clip_update(p, g)
    assert n > 1 and np.allclose(q, p - 0.1 * g / (n + 1e-6), rtol=0, atol=1e-15)
    H, C, T = 8, 6, 7
    w = [rng.standard_normal(s) * 0.4 for s in ((2, 4 * H, C), (2, 4 * H, H), (2, 4 * H), (2, 4 * H))]
    r = fr.lstm_bptt(rng.standard_normal((T, C)), *w, rng.standard_normal((T, 2 * H)))
    assert float(np.abs(r["y"] - r["y_loop"]).max()) < 1e-12
    assert float(np.abs(r["dgates"].sum(0).reshape(2, 4 * H) - r["db_ih"]).max()) < 1e-12 and float(np.abs(r["db_ih"] - r["db_hh"]).max()) < 1e-12


# ---- the cloner's keywords, on the emulator ---------------------------------------------------------------------------------------
PHONES = ["~həlˈoʊ~#", "~nnˈaʊ tˈɛn~#"]
SAMPLES = [256 * 20 + 77, 256 * 16 + 3]


@pytest.fixture()
def cloners(tmp_path, monkeypatch):
    """(plain, fine-tuning) UtteranceCloner instances on the CPU emulator, without the synthesis engines."""
    build.build()  # the emulator asks the library itself for the convs' tile sizes
    finetune_emulator.install(monkeypatch)
    models = tmp_path / "Models"
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    monkeypatch.setattr(cloner_mod, "ToucanTTSInterface", lambda **kw: None)
    monkeypatch.setattr(cloner_mod.UtteranceCloner, "_warned_fine_tune", False)
    return (cloner_mod.UtteranceCloner("unused", "cpu"), cloner_mod.UtteranceCloner("unused", "cpu", fine_tune_aligner=True, fine_tune_seed=11))


def test_cloner_keywords(cloners):
    plain, tuned = cloners
    sig = inspect.signature(cloner_mod.UtteranceCloner.__init__).parameters
    assert list(sig)[1:] == ["model_id", "device", "language", "speed_over_quality", "track_pitch", "fine_tune_aligner", "fine_tune_seed"]
    assert sig["fine_tune_aligner"].default is False and sig["fine_tune_seed"].default == 0
    waves = [fw.reference_wave(40 + u, n) for u, n in enumerate(SAMPLES)]
    before = {k: v.clone() for k, v in tuned.aligner_weights.items()}
    with pytest.warns(UserWarning):  # the default: warned about, not performed
        base = plain.extract_prosody_batch(PHONES, waves, 16000)
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        both = tuned.extract_prosody_batch(PHONES, waves, 16000)
        ft_logits, rag = tuned.extractor.last_logits.clone(), tuned.extractor.last_rag
        fts = list(tuned.extractor.last_fine_tune)
        off = tuned.extract_prosody_batch(PHONES, waves, 16000, on_line_fine_tune=False)
    eval_logits = tuned.extractor.last_logits.clone()
    assert len(fts) == 2 and all(np.isfinite(l.numpy()).all() and (n.numpy() > 1).all() for l, n in fts)  # five losses, five clipped norms
    # on_line_fine_tune=False: today's eval-mode result; =True moves the logits by four orders of magnitude more than the 1e-5 by
    # which two correct float32 results differ (by 2.5 - 2.8 on the goldens' mels; about 1 on these short recordings)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) for a, b in zip(off, base))
    for u in range(2):  # (the utterances' own rows: the rows between them hold nothing)
        rows = slice(rag.begins[u], rag.begins[u] + rag.lengths[u])
        assert float((ft_logits[rows] - eval_logits[rows]).abs().max()) > 0.1, u
    # a batch equals its utterances one by one, a repeated call repeats its result, another seed gives another result
    for u in range(2):
        one = tuned.extract_prosody_batch([PHONES[u]], [waves[u]], 16000)[0]
        assert torch.equal(one[0], both[u][0]) and torch.equal(one[2], both[u][2]), u
        b0, n = rag.begins[u], rag.lengths[u]
        assert torch.equal(tuned.extractor.last_logits[:n], ft_logits[b0:b0 + n]), u
    # explicit masks: the recipe's for the instance's seed give the instance's result
    n0 = 1 + SAMPLES[0] // 256
    given = tuned.extract_prosody_batch([PHONES[0]], [waves[0]], 16000, dropout_masks=[finetune.dropout_masks(11, n0)])[0]
    assert torch.equal(given[0], both[0][0])
    first = tuned.extractor.last_logits.clone()
    tuned.fine_tune_seed = 12
    tuned.extract_prosody_batch([PHONES[0]], [waves[0]], 16000)
    assert not torch.equal(tuned.extractor.last_logits[:n0], first[:n0])
    # the loaded weights are never modified
    assert all(torch.equal(v, tuned.aligner_weights[k]) for k, v in before.items())
    theta0, _ = finetune.pack_parameters(before)
    assert np.array_equal(tuned.extractor._tuner.theta0.numpy(), theta0)
    with pytest.raises(ValueError, match="fewer than 2 mel frames"):
        tuned.extract_prosody_batch([PHONES[0]], [waves[0]], 16000, speech_bounds=[(0, 200)])
    with pytest.raises(ValueError, match="dropout_masks"):
        plain.extract_prosody_batch([PHONES[0]], [waves[0]], 16000, dropout_masks=[finetune.dropout_masks(11, n0)])


def test_train_header_binding_library_and_emulator_agree():
    """include/toucan_train.h, capi.TRAIN_PROTOTYPES, the symbols libtoucan_hip.so exports and the emulator's entry points are the
    same set, apart from every other binding table; toucan_tts.h does not declare them."""
    root = os.path.dirname(HERE)
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", p), encoding="utf-8").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", strip("toucan_train.h"))))
    assert len(declared) == 10 and sorted(capi.TRAIN_PROTOTYPES) == declared
    for other in (capi.PROTOTYPES, capi.ALIGN_PROTOTYPES, capi.SCORE_PROTOTYPES, capi.GAN_PROTOTYPES, capi.PITCH_PROTOTYPES):
        assert not set(declared) & set(other)
    assert not set(declared) & set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", strip("toucan_tts.h")))
    text = strip("toucan_train.h")
    for name, value in (("TTS_GEMM_NN", capi.GEMM_NN), ("TTS_GEMM_NT", capi.GEMM_NT), ("TTS_GEMM_TN", capi.GEMM_TN),
                        ("TTS_CTC_GRAD_MAX_TARGETS", capi.CTC_GRAD_MAX_TARGETS), ("TTS_SUMSQ_PARTIALS", capi.SUMSQ_PARTIALS)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value, name
    assert "train.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    emu = finetune_emulator.FineTuneEmulator()
    for n in declared:
        fn = getattr(handle, n)
        assert fn.argtypes == capi.TRAIN_PROTOTYPES[n][1] and fn.restype == capi.TRAIN_PROTOTYPES[n][0], n
        assert len(inspect.signature(getattr(emu, n)).parameters) == len(capi.TRAIN_PROTOTYPES[n][1]), n
    assert handle.tts_abi_version() == 15
