"""The scorer's glow loss without a GPU: the float64 restatement (tests/glow_ref.py) against the golden of the reference's own modules
(tests/golden/make_glow_golden.py), the forward InvConvNear weights and the log-determinant constant that a scoring pipeline uploads,
the bookkeeping of TTSScorer with five losses, and the C entry's argument checks on a handle created without a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import build, capi, fixture_weights as fw, packing, scorer
from tests import glow_ref as gr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["meta", "monolingual", "single"]
NEW_ENTRIES = ["tts_glow_forward_rows", "tts_glow_nll_reduce", "tts_postflow_nll"]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(REPO, "tests", "golden", "scorer", "glow.npz"))


@pytest.fixture(scope="module")
def sd():
    return fw.acoustic_state_dict()


@pytest.fixture(scope="module")
def corpus_items(tmp_path_factory):
    s = np.load(os.path.join(REPO, "tests", "golden", "scorer", "scorer.npz"))
    d = str(tmp_path_factory.mktemp("glow_corpus"))
    fw.write_fixture_corpus(d, **json.loads(str(s["tts_corpus"])))
    return scorer.read_tts_cache(d)[1]


def test_golden_holds_what_the_tests_need(g, corpus_items):
    frames = [it["spec"].shape[0] for it in corpus_items]
    assert list(g["glow_frames"]) == frames == [93, 154, 116, 72, 114]
    for v in VARIANTS:
        ref, f64 = g[f"glow_{v}_ref"], g[f"glow_{v}_f64"]
        assert ref.shape == f64.shape == (5,) and ref.dtype == np.float32 and f64.dtype == np.float64
        assert np.all(np.abs(ref - f64) <= 1e-6 * np.abs(f64))  # the reference's own fp32 run against its float64 run
    assert g["glow_meta_z0"].shape == (92, 80) and g["glow_meta_rows0"].shape == (46, 2) and g["glow_meta_cat0"].shape == (93, 272)
    assert 0 < float(g["glow_roundtrip_fp32"]) < 1e-3
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "scorer", "glow.npz")) < 200 * 1024


def test_loss_from_the_golden_row_parts(g):
    """The loss recombines from the stored row parts with the reference's two divisors: 160 * 46 rows and 80 * 93 frames."""
    rows, want = g["glow_meta_rows0"], float(g["glow_meta_f64"][0])
    assert abs(gr.loss_from_parts(rows, 93) - want) <= 1e-12 * want
    assert abs(gr.loss_from_parts(rows, 92) - want) > 2e-4 * want  # (the truncated length is not the divisor: twice the GPU test's bound away)
    assert abs(rows[:, 1].sum() - g["glow_meta_logdets0"].sum()) <= 1e-12 * abs(rows[:, 1].sum())
    z = g["glow_meta_z0"].reshape(46, 160)
    assert np.abs((0.5 * z * z + gr.HALF_LOG_2PI).sum(axis=1) - rows[:, 0]).max() <= 1e-12 * rows[:, 0].max()
    assert np.isnan(gr.loss_from_parts(np.zeros((0, 2)), 1))


def test_restatement_reproduces_the_golden(g, sd, corpus_items):
    """flow_forward on utterance 0 (T = 93) from the stored conditioning input.  That input is the float64 model's, rounded to fp32 for
    the file's size: 2^-24 relative on the input of g_proj, which the generator bounds by 1e-5 on z and 1e-7 on the loss (it asserts
    1e-10 from the unrounded input)."""
    folded = gr.fold_weight_norm(sd)
    gold = corpus_items[0]["spec"]
    z, ld = gr.flow_forward(folded, gold, g["glow_meta_cat0"])
    assert z.shape == (46, 160) and np.abs(z.reshape(92, 80) - g["glow_meta_z0"]).max() <= 1e-5
    an, inv = gr.logdet_constant(folded)
    want = g["glow_meta_logdets0"]
    assert abs(46 * an - want[0]) <= 1e-10 * abs(want[0]) and abs(46 * inv - want[1]) <= 1e-10 * abs(want[1])
    assert abs(ld.sum() - want[2]) <= 1e-6 * abs(want[2])
    parts = gr.row_parts(z, ld, an + inv)
    assert np.all(np.abs(parts - g["glow_meta_rows0"]) <= 1e-6 * np.abs(g["glow_meta_rows0"]))
    loss = gr.loss_from_parts(parts, 93)
    assert abs(loss - float(g["glow_meta_f64"][0])) <= 1e-7 * loss
    assert abs(gr.glow_loss(folded, gold, g["glow_meta_cat0"]) - loss) == 0.0


def test_forward_weight_times_stored_inverse_is_the_identity(sd):
    folded = packing.fold_weight_norm(sd)
    for b in range(18):
        p = f"post_flow.flows.{3 * b + 1}."
        w, winv = packing.invconv_forward(folded, p), packing.invconv_inverse(folded, p)
        assert w.dtype == np.float32 and w.shape == (4, 4)
        assert np.abs(w.astype(np.float64) @ winv.astype(np.float64) - np.eye(4)).max() <= 1e-6, b
        assert np.abs(w - gr.invconv_weight(folded, p)[0]).max() <= 2.0 ** -24 * np.abs(w).max(), b  # float64, rounded once


def test_logdet_constant_equals_slogdet(sd):
    """40 log|det W| per block from numpy's LU, not from log_s: also where sign_s is negative (log_s is the log of |diag U|)."""
    folded = packing.fold_weight_norm(sd)
    total, negative = 0.0, 0
    for b in range(18):
        p = f"post_flow.flows.{3 * b + 1}."
        w, log_s = gr.invconv_weight(folded, p)
        sign, logabs = np.linalg.slogdet(w)
        assert abs(logabs - log_s) <= 1e-9 * max(1.0, abs(log_s)), b
        negative += int((np.asarray(folded[p + "sign_s"]) < 0).any())
        total += 40.0 * logabs + float(np.asarray(folded[f"post_flow.flows.{3 * b}.logs"], dtype=np.float64).sum())
    assert negative > 0, "the fixture has no block with a negative sign_s"
    const = packing.glow_logdet_constant(folded)
    assert isinstance(const, float) and abs(const - total) <= 1e-9 * abs(total)
    assert abs(const - sum(gr.logdet_constant(folded))) <= 1e-12 * abs(const)


def _scorer_without_device():
    tts = scorer.TTSScorer.__new__(scorer.TTSScorer)
    tts.nans_removed = False
    return tts


def test_record_scores_with_four_and_five_columns(tmp_path):
    d = str(tmp_path)
    paths = fw.write_fixture_corpus(d, 4, seed=4)
    datapoints, items = scorer.read_tts_cache(d)
    rng = np.random.default_rng(5)
    parts = rng.uniform(0.1, 9.0, size=(4, 5)).astype(np.float32)
    parts[2, 4] = np.nan  # an utterance of one frame has no glow loss
    five = _scorer_without_device()
    five.record_scores(scorer.ScoredCorpus(d, datapoints, 12), items, parts, include_glow=True)
    four = _scorer_without_device()
    four.record_scores(scorer.ScoredCorpus(d, datapoints, 12), items, parts[:, :4])
    for k, p in enumerate(paths):
        today = np.float32(parts[k, 0]) + np.float32(parts[k, 1]) + np.float32(parts[k, 2]) + np.float32(parts[k, 3])
        assert four.path_to_score[p] == float(today)  # four columns: bit for bit what the scorer recorded before the fifth existed
        assert four.path_to_parts[p] == tuple(float(v) for v in parts[k, :4])
        if k == 2:
            assert np.isnan(five.path_to_score[p])
            continue
        assert five.path_to_score[p] == float(today + np.float32(parts[k, 4]))
        assert five.path_to_parts[p] == tuple(float(v) for v in parts[k])
    assert four.nans == [] and five.nans == [paths[2]] and five.nan_indexes == [2]
    assert four.path_to_id == five.path_to_id == {p: i for i, p in enumerate(paths)}
    with pytest.raises(ValueError, match="include_glow"):
        four.record_scores(scorer.ScoredCorpus(d, datapoints, 12), items, parts)  # five columns, not asked for
    with pytest.raises(ValueError, match="include_glow"):
        five.record_scores(scorer.ScoredCorpus(d, datapoints, 12), items, parts[:, :4], include_glow=True)
    with pytest.raises(ValueError, match="keep_row_scores"):
        five.score(d, "en", keep_row_scores=True)  # (refused before anything touches a device)


def test_header_bindings_and_library_agree():
    with open(os.path.join(REPO, "include", "toucan_score.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.SCORE_PROTOTYPES) and set(NEW_ENTRIES) <= set(declared)
    for other in (capi.PROTOTYPES, capi.ALIGN_PROTOTYPES, capi.GAN_PROTOTYPES, capi.PITCH_PROTOTYPES, capi.TRAIN_PROTOTYPES, capi.RESAMPLE_PROTOTYPES):
        assert not set(declared) & set(other)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_GLOW_FORWARD_[A-Z_]+)\s+(\d+)", text)}
    assert macros == {"TTS_GLOW_FORWARD_BLOCK_ROWS": capi.GLOW_FORWARD_BLOCK_ROWS, "TTS_GLOW_FORWARD_GRID_ROWS": capi.GLOW_FORWARD_GRID_ROWS}
    assert capi.GLOW_FORWARD_GRID_ROWS % capi.GLOW_FORWARD_BLOCK_ROWS == 0
    assert "glow_forward.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, C.CDLL)
    for n in declared:  # every symbol the header declares is exported and bound as declared
        fn = getattr(handle, n)
        assert fn.argtypes == capi.SCORE_PROTOTYPES[n][1] and fn.restype == capi.SCORE_PROTOTYPES[n][0], n
    assert handle.tts_abi_version() == 15  # additive: no struct and no existing prototype changed


def test_kernel_entries_check_their_arguments_before_any_launch():
    lib = capi.lib()
    err = lambda: lib.tts_last_error().decode()
    assert lib.tts_glow_forward_rows(None, 160, 4, None, 0, None, None, None, None, None) == -1 and "null x" in err()
    x = C.c_void_p(4096)  # never dereferenced: every call below is refused
    assert lib.tts_glow_forward_rows(x, 159, 4, None, 0, None, x, x, x, None) == -1 and "159" in err()
    assert lib.tts_glow_forward_rows(x, 160, 4, None, 0, None, None, None, None, None) == -1 and "neither half" in err()
    assert lib.tts_glow_forward_rows(x, 160, 4, x, 160, None, None, None, None, None) == -1 and "row_logdet" in err()
    assert lib.tts_glow_forward_rows(x, 160, 4, x, 100, x, None, None, None, None) == -1 and "100" in err()
    assert lib.tts_glow_forward_rows(x, 160, 4, None, 0, None, x, None, x, None) == -1 and "an_bias" in err()
    assert lib.tts_glow_forward_rows(x, 160, 0, None, 0, None, x, x, x, None) == 0  # no rows: nothing to launch
    assert lib.tts_glow_nll_reduce(x, 160, x, x, x, None, 1, 0.0, x, None, None) == -1 and "null pointer" in err()
    assert lib.tts_glow_nll_reduce(x, 100, x, x, x, x, 1, 0.0, x, None, None) == -1 and "100" in err()
    assert lib.tts_glow_nll_reduce(x, 160, x, x, x, x, 0, 0.0, x, None, None) == 0


def _create(precision):
    lib = capi.lib()
    cfg = capi.TtsConfig(1, 1, 0, precision, 0, 0.0)
    h = C.c_void_p()
    assert lib.tts_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def test_postflow_nll_refuses_with_a_code_and_a_message():
    """A handle created without a device: no forward weights, nothing run.  Every refusal is a negative code and a message."""
    lib, h = _create(capi.COMPUTE_F32)
    x = C.c_void_p(4096)
    assert lib.tts_postflow_nll(None, x, 80, x, None, None, None) < 0 and "null handle" in lib.tts_last_error().decode()
    rc = lib.tts_postflow_nll(h, x, 80, x, None, None, None)
    msg = lib.tts_last_error().decode()
    assert rc < 0 and "flow.<b>.wfwd" in msg and "flow.logdet" in msg and "flow.<b>.end_ml" in msg and "scoring=True" in msg
    # the constant alone (host metadata: loads without a device) is not the forward weights
    const = np.array([1.5], dtype=np.float64).view(np.int32).copy()
    shape = (C.c_int64 * 1)(2)
    assert lib.tts_load_weights(h, b"flow.logdet", const.ctypes.data_as(C.c_void_p), shape, 1, 3) == 0
    assert lib.tts_postflow_nll(h, x, 80, x, None, None, None) < 0 and "flow.<b>.wfwd" in lib.tts_last_error().decode()
    assert lib.tts_destroy(h) == 0
    lib, h16 = _create(capi.COMPUTE_BF16)
    assert lib.tts_postflow_nll(h16, x, 80, x, None, None, None) < 0 and "fp32 handles only" in lib.tts_last_error().decode()
    assert lib.tts_destroy(h16) == 0
