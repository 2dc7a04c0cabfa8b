"""The corpus scorer on the MI355X (csrc/score.hip, tts_teacher_forced, ims-toucan-prosody-variance_amd/scorer.py): the CTC kernel
against the float64 CTC of the golden (tests/golden/make_scorer_golden.py) and batch against one by one, the teacher-forced losses
against the reference's training ToucanTTS for the three checkpoint variants, the gold prosody left untouched by teacher forcing, and
both scorers end to end on a fixture corpus."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, capi, engine, fixture_weights as fw, scorer
from ims_toucan_prosody_variance_amd.phonemes import IDX
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import scorer_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "scorer", "scorer.npz"))
CASES = json.loads(str(G["ctc_cases"]))
VARIANTS = ["meta", "monolingual", "single"]


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


@pytest.fixture(scope="module")
def ops():
    return engine.Ops(DEV)


@pytest.fixture(scope="module")
def aligner():
    return align.AlignerEngine(fw.aligner_state_dict(), DEV)


def _ctc(ops, logits_list, ids_list):
    """Several utterances' logits packed back to back -> the kernel's losses (numpy)."""
    rag = Ragged([lg.shape[0] for lg in logits_list], ops.device)
    x = torch.from_numpy(np.concatenate(logits_list).astype(np.float32)).to(ops.device)
    return scorer.ctc_loss_batch(ops, x, rag, ids_list).cpu().numpy()


def test_ctc_on_the_reference_logits_matches_float64(ops):
    for name in CASES:
        if f"ctc_{name}_logits" not in G:
            continue
        got = _ctc(ops, [G[f"ctc_{name}_logits"]], [G[f"ctc_{name}_ids"]])[0]
        f64 = float(G[f"ctc_{name}_f64"])
        if name == "infeasible":
            assert got == 0.0, got  # zero_infinity: exactly 0
        else:
            assert _rel(got, f64) <= 1e-5, (name, got, f64)


def test_ctc_through_the_gpu_aligner_matches_float64(ops, aligner):
    """Every golden case, T ~ 4000 included: seeded mel -> AlignerEngine.logits -> tts_ctc_loss."""
    worst = 0.0
    for name in CASES:
        T, u = int(G[f"ctc_{name}_T"]), int(G[f"ctc_{name}_u"])
        mel = torch.from_numpy(fw.aligner_spectrogram(u, T)).to(aligner.device)
        rag = Ragged([T], aligner.device)
        with torch.inference_mode():
            lg = aligner.logits(mel, rag)
            got = float(scorer.ctc_loss_batch(aligner.ops, lg, rag, [G[f"ctc_{name}_ids"]]).cpu()[0])
        f64 = float(G[f"ctc_{name}_f64"])
        if name == "infeasible":
            assert got == 0.0, got
        else:
            worst = max(worst, _rel(got, f64))
            assert _rel(got, f64) <= 1e-5, (name, got, f64)
    print(f"largest CTC relative error against float64: {worst:.2e}")


def test_ctc_batch_equals_one_by_one_bit_for_bit(ops):
    rng = np.random.default_rng(11)
    logits, ids = [], []
    for b in range(32):
        T = int(rng.integers(1, 700))
        n = int(rng.integers(0, min(T, 180) + 1)) if b % 7 else int(T + 3)  # every 7th: more ids than frames (infeasible)
        lg = rng.normal(0.0, 3.0, size=(T, 145)).astype(np.float32)
        tg = rng.integers(0, 144, size=n).astype(np.int32)
        if n > 4:
            tg[2] = tg[1]  # a repeat
        logits.append(lg)
        ids.append(tg)
    batch = _ctc(ops, logits, ids)
    alone = np.array([_ctc(ops, [lg], [tg])[0] for lg, tg in zip(logits, ids)])
    assert np.array_equal(batch.view(np.uint32), alone.view(np.uint32))
    for b in (0, 1, 7, 13, 31):  # spot checks against the float64 restatement
        lp = sr.log_softmax32(logits[b])
        want = sr.ctc_loss(lp, ids[b])
        assert abs(batch[b] - want) <= 1e-5 * max(1.0, abs(want)), (b, batch[b], want)
    assert (batch[::7] == 0).all()


@pytest.mark.parametrize("T, n", [(33, 4), (140, 130)])
def test_ctc_loss_and_ctc_grad_return_the_same_loss(ops, T, n):
    """tts_ctc_loss at batch 1 and tts_ctc_grad walk one lattice (csrc/ctc_lattice.h) and reach the same fp64 log-likelihood by the
    same operations; then one divides nll / n and the other multiplies nll * (1 / n), at most one fp64 ulp apart, which is at most
    one float32 step after the rounding.  T = 33 crosses the loss kernel's chunk of 32 frames; T = 140 with n = 130 has S = 261
    states, past one stride of 256, and ends in a chunk of 12."""
    rng = np.random.default_rng(1000 * T + n)
    lg = rng.normal(0.0, 3.0, size=(T, 145)).astype(np.float32)
    ids = ((np.arange(n) * 7 + int(rng.integers(0, 144))) % 144).astype(np.int32)  # 7 is no divisor of 144: neighbours differ
    assert (np.diff(ids) != 0).all() and ids.min() >= 0 and ids.max() < 144
    x = torch.from_numpy(lg).to(ops.device)
    a = float(scorer.ctc_loss_batch(ops, x, Ragged([T], ops.device), [ids]).cpu()[0])
    alpha = torch.empty(T * (2 * n + 1), dtype=torch.float64, device=ops.device)
    lp, loss, grad = (torch.zeros(s, dtype=torch.float32, device=ops.device) for s in ((T, 145), (1,), (T, 145)))
    targets = torch.from_numpy(ids).to(ops.device)
    capi.check(ops.lib.tts_ctc_grad(x.data_ptr(), 145, 145, T, targets.data_ptr(), n, 144, alpha.data_ptr(), lp.data_ptr(), loss.data_ptr(),
                                    grad.data_ptr(), 145, ops.stream()), "tts_ctc_grad")
    b = float(loss.cpu()[0])
    print(f"T {T}, n {n}: tts_ctc_loss {a!r}, tts_ctc_grad {b!r}, one float32 step {float(np.spacing(np.float32(a)))!r}")
    assert a == a and b == b and a != 0.0 and b != 0.0
    assert abs(a - b) <= float(np.spacing(np.float32(max(abs(a), abs(b)))))


def test_ctc_argument_checks(ops):
    lg = np.zeros((4, 145), dtype=np.float32)
    with pytest.raises(ValueError):
        _ctc(ops, [lg], [np.zeros(capi.CTC_MAX_TARGETS + 1, dtype=np.int32)])
    assert np.isnan(_ctc(ops, [lg], [np.array([144], dtype=np.int32)])[0])  # the blank is not a target


def _write_checkpoints(d, variant_kw):
    model = os.path.join(d, "model.pt")
    emb = os.path.join(d, "embedding_function.pt")
    t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    torch.save({"model": t(fw.acoustic_state_dict(**variant_kw))}, model)
    torch.save({"style_emb_func": t(fw.style_state_dict())}, emb)
    return model, emb


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("golden_corpus"))
    fw.write_fixture_corpus(d, **json.loads(str(G["tts_corpus"])))
    return d


@pytest.mark.parametrize("variant", VARIANTS)
def test_tts_losses_match_reference(variant, corpus, tmp_path):
    model, emb = _write_checkpoints(str(tmp_path), json.loads(str(G[f"tts_{variant}_fixture"])))
    tts = scorer.TTSScorer(model, DEV, path_to_embedding_checkpoint=emb)
    _, items = scorer.read_tts_cache(corpus)
    got = tts.score_items(items, int(G["tts_lang_id"]), batch_size=1).astype(np.float64)
    ref = G[f"tts_{variant}_losses"]
    err = np.abs(got - ref)
    rel = err / np.abs(ref)
    print(f"{variant}: largest relative error l1 {rel[:, 0].max():.2e}, dur {rel[:, 1].max():.2e}, pitch {rel[:, 2].max():.2e}, "
          f"energy {rel[:, 3].max():.2e}")
    assert (rel[:, 0] <= 1e-4).all(), (got, ref)
    bound = np.maximum(1e-4 * np.abs(ref[:, 1:]), 1e-6)
    assert (err[:, 1:] <= bound).all(), (got, ref)
    if variant == "meta":  # before_outs / after_outs of utterance 0
        out = tts.forward_batch([items[0]], int(G["tts_lang_id"]))
        T = items[0]["spec"].shape[0]
        before = out["before"][:T].cpu().numpy()
        after = torch.empty(out["before"].shape, dtype=torch.float32, device=tts.pipe.device)
        capi.check(tts.pipe.lib.tts_copy_mel(tts.pipe.h, C.c_void_p(after.data_ptr()), 80, tts.pipe._stream()), "tts_copy_mel")
        after = after[:T].cpu().numpy()
        assert np.abs(before - G["tts_meta_before0"]).mean() < 1e-5 and np.abs(before - G["tts_meta_before0"]).max() < 2e-4
        assert np.abs(after - G["tts_meta_after0"]).mean() < 1e-5 and np.abs(after - G["tts_meta_after0"]).max() < 2e-4
        pred = out["pred"].cpu().numpy()
        assert np.abs(pred - G["tts_meta_pred0"]).max() < 1e-4


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ckpt"))
    model, emb = _write_checkpoints(d, {})
    return scorer.TTSScorer(model, DEV, path_to_embedding_checkpoint=emb), model, emb


def test_teacher_forcing_keeps_the_gold_prosody(meta, corpus):
    tts = meta[0]
    _, items = scorer.read_tts_cache(corpus)
    for it in items:  # the fixture: nonzero gold pitch on word boundaries and unvoiced phonemes
        wb = it["text"][:, IDX["word_boundary"]] != 0
        unv = (it["text"][:, IDX["phoneme"]] != 0) & (it["text"][:, IDX["voiced"]] == 0)
        assert wb.any() and unv.any() and (it["pitch"][wb] != 0).all() and (it["pitch"][unv] != 0).all()
    out = tts.forward_batch(items, int(G["tts_lang_id"]))
    R = out["rag_phone"].total_rows
    d = torch.empty(R, dtype=torch.int32, device=tts.pipe.device)
    p = torch.empty(R, dtype=torch.float32, device=tts.pipe.device)
    e = torch.empty(R, dtype=torch.float32, device=tts.pipe.device)
    capi.check(tts.pipe.lib.tts_copy_prosody(tts.pipe.h, C.c_void_p(d.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(e.data_ptr()),
                                             tts.pipe._stream()), "tts_copy_prosody")
    assert np.array_equal(d.cpu().numpy(), np.concatenate([it["durations"] for it in items]).astype(np.int32))
    assert np.array_equal(p.cpu().numpy(), np.concatenate([it["pitch"] for it in items]))
    assert np.array_equal(e.cpu().numpy(), np.concatenate([it["energy"] for it in items]))


def test_tts_batch_matches_batch_one(meta, tmp_path):
    tts = meta[0]
    fw.write_fixture_corpus(str(tmp_path), 12, seed=21, words=(2, 12))
    _, items = scorer.read_tts_cache(str(tmp_path))
    lid = int(G["tts_lang_id"])
    one = tts.score_items(items, lid, batch_size=1)
    many = tts.score_items(items, lid, batch_size=32)
    assert np.all(np.abs(many - one) <= 1e-5 * np.abs(one)), (many, one)


def test_scorers_end_to_end(meta, tmp_path, capsys):
    tts, model, emb = meta
    d = str(tmp_path / "corpus")
    paths = fw.write_fixture_corpus(d, 40, seed=31, words=(2, 10))
    lid = int(G["tts_lang_id"])
    # AlignmentScorer.score: per file path, bit for bit the kernel run on that utterance alone
    ckpt = os.path.join(str(tmp_path), "aligner.pt")
    torch.save({"asr_model": {k: torch.from_numpy(np.array(v)) for k, v in fw.aligner_state_dict().items()}}, ckpt)
    al = scorer.AlignmentScorer(ckpt, DEV)
    al.score(os.path.join(d, "aligner_train_cache.pt"))
    assert list(al.path_to_score) == paths and al.nans == []
    items, _ = scorer.read_aligner_cache(d)
    for k in (0, 17, 39):
        text, mel = items[k]
        alone = al.score_items([(text, mel)], batch_size=1)[0]
        assert np.float32(al.path_to_score[paths[k]]).view(np.uint32) == np.float32(alone).view(np.uint32), k
        with torch.inference_mode():
            rag = Ragged([mel.shape[0]], al.aligner.device)
            lp = torch.log_softmax(al.aligner.logits(torch.from_numpy(mel).to(al.aligner.device), rag), 1).cpu().numpy()
        want = sr.ctc_loss(lp, align.token_ids(text)[0])
        assert abs(alone - want) <= 1e-5 * want, (k, alone, want)
    al.show_samples_with_highest_loss(3)
    # TTSScorer.score: per file path, the kernel-level losses of that utterance (batch of one)
    tts.score(d, lang_id="en")
    assert list(tts.path_to_score) == paths and tts.path_to_id == {p: i for i, p in enumerate(paths)} and tts.nans == []
    _, its = scorer.read_tts_cache(d)
    for k in (0, 5, 39):
        parts = tts.forward_batch([its[k]], lid)["losses"].cpu().numpy()[0]
        want = np.float32(parts[0]) + np.float32(parts[1]) + np.float32(parts[2]) + np.float32(parts[3])
        assert abs(tts.path_to_score[paths[k]] - want) <= 1e-5 * abs(want), (k, tts.path_to_score[paths[k]], want)
    tts.show_samples_with_highest_loss(5)
    worst = sorted(tts.path_to_score, key=tts.path_to_score.get, reverse=True)[:5]
    tts.remove_samples_with_highest_loss(5)
    left = [dp[8] for dp in torch.load(os.path.join(d, "fast_train_cache.pt"), weights_only=True)]
    assert left == [p for p in paths if p not in worst]
    assert "Loss:" in capsys.readouterr().out
