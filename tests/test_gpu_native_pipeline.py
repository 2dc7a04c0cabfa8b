"""The stage API (include/toucan_tts.h: tts_create ... tts_synthesize_batch; csrc/pipeline.hip sequences the kernels in C++)
on a real MI355X, through ctypes:
 (1) against the committed reference goldens (tests/golden/*.npz) with the fp32 tolerances of test_gpu_e2e.py, and
 (2) against the Python-sequenced engines (engine.py), which launch the same kernels in the same order: bit-identical."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, fixture_weights as fw, native, synthetic as syn
from ims_toucan_prosody_variance_amd.ragged import Ragged

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


def _gold(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _inputs(gs):
    texts = [torch.from_numpy(g["text"]) for g in gs]
    embs = torch.stack([torch.from_numpy(g["utt_emb"]) for g in gs])
    langs = [int(g["lang_id"]) for g in gs]
    zs = [torch.from_numpy(g["z"]) for g in gs]
    return texts, embs, langs, zs


@pytest.fixture(scope="module")
def pipes():
    assert torch.cuda.is_available()
    ac = fw.acoustic_state_dict()
    return {k: native.NativePipeline(ac, sd, k, DEV) for k, sd in (("hifigan", fw.hifigan_state_dict()), ("bigvgan", fw.bigvgan_state_dict()))}


@pytest.mark.parametrize("name", ["L7_pred", "L20_pred", "L20_ctrl", "L20_gold_odd", "L20_gold_prosody", "L128_gold5"])
def test_stage_api_matches_reference_golden(pipes, name):
    g = _gold(name)
    texts, embs, langs, zs = _inputs([g])
    kw = json.loads(str(g["ctrl"]))
    if "gold_durations" in g.files:
        kw["durations"] = [torch.from_numpy(g["gold_durations"])]
    if "gold_pitch" in g.files:  # gold prosody overrides (InferenceToucanTTS.py:209-210; UtteranceCloner.py:163): zeroed and scaled like predictions
        kw["pitch"], kw["energy"] = [torch.from_numpy(g["gold_pitch"])], [torch.from_numpy(g["gold_energy"])]
    out = pipes["hifigan"].forward(texts, embs, langs, z_noise=zs, **kw)
    assert np.array_equal(out["durations"][0].cpu().numpy(), g["durations"]), "durations must be bit exact"
    np.testing.assert_allclose(out["pitch"][0].cpu().numpy(), g["pitch"], atol=5e-5)
    np.testing.assert_allclose(out["energy"][0].cpu().numpy(), g["energy"], atol=5e-5)
    mel = out["mel"][0].cpu().numpy()
    assert mel.shape == g["mel"].shape
    err = np.abs(mel - g["mel"])
    assert err.max() < 5e-4 and err.mean() < 1e-4, (float(err.max()), float(err.mean()))
    if "wav_hifigan" in g.files:
        b, n = out["wav_spans"][0]
        assert np.abs(out["wav"][b:b + n].cpu().numpy() - g["wav_hifigan"]).max() < 5e-4


@pytest.mark.parametrize("kind", ["hifigan", "bigvgan"])
def test_stage_api_vocoders_match_reference_golden(pipes, kind):
    for name in ("L7_pred", "L20_pred"):
        g = _gold(name)
        mel = torch.from_numpy(g["mel"]).to(DEV).contiguous()
        wav, rag = pipes[kind].vocode(mel, Ragged([mel.shape[0]], DEV))
        assert np.abs(wav.cpu().numpy()[: rag.lengths[0]] - g["wav_" + kind]).max() < 5e-4, (kind, name)


@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
def test_stage_api_is_bit_identical_to_the_python_sequencer(precision):
    """Ragged 4-batch (goldens R128/R97/R64/R20, gold durations) + BigVGAN: C++ sequencing == Python sequencing, bit for bit,
    in every precision (same kernels, same order, same tile-form decisions)."""
    gs = [_gold(n) for n in ("R128", "R97", "R64", "R20")]
    texts, embs, langs, zs = _inputs(gs)
    durs = [torch.from_numpy(g["gold_durations"]) for g in gs]
    ac_sd, voc_sd = fw.acoustic_state_dict(), fw.bigvgan_state_dict()
    pipe = native.NativePipeline(ac_sd, voc_sd, "bigvgan", DEV, precision=precision)
    ac = engine.AcousticEngine(ac_sd, DEV, precision=precision)
    voc = engine.VocoderEngine(voc_sd, "bigvgan", DEV, precision=precision)
    kw = dict(pitch_variance_scale=1.3, energy_variance_scale=0.7)
    ref = ac.forward(texts, embs, langs, durations=durs, z_noise=zs, **kw)
    wref, rw = voc.forward(ref["mel_packed"], ref["rag_mel"])
    out = pipe.forward(texts, embs, langs, durations=durs, z_noise=zs, **kw)
    for u in range(4):
        assert torch.equal(out["pitch"][u], ref["pitch"][u])
        assert torch.equal(out["mel"][u], ref["mel"][u]), f"utterance {u}: max diff {float((out['mel'][u] - ref['mel'][u]).abs().max()):.3e}"
        b, n = out["wav_spans"][u]
        assert (b, n) == (rw.begins[u], rw.lengths[u])
        assert torch.equal(out["wav"][b:b + n], wref[b:b + n]), f"utterance {u}: waveform differs"


def test_predicted_durations_and_variants_through_the_stage_api():
    """Predicted durations (duration predictor + control + host round trip inside tts_control_and_regulate) on a seeded batch, and
    the single-speaker checkpoint variant (plain LayerNorm predictors, no utterance embedding) - both equal to the Python sequencer."""
    us, Ls = [300, 301, 302], [48, 21, 33]
    feats = [torch.from_numpy(syn.utterance_features(u, L)) for u, L in zip(us, Ls)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in us]))
    kw = dict(duration_scaling_factor=0.9, pitch_variance_scale=1.2, energy_variance_scale=0.8, pause_duration_scaling_factor=1.3)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    for sd, langs in ((fw.acoustic_state_dict(), [syn.LANG_EN] * 3),):
        pipe = native.NativePipeline(sd, None, None, DEV)
        ac = engine.AcousticEngine(sd, DEV)
        ref = ac.forward(feats, embs, langs, generator=gen(), **kw)
        out = pipe.forward(feats, embs, langs, generator=gen(), **kw)
        assert torch.equal(out["durations_packed"], ref["durations_packed"])
        for u in range(3):
            assert torch.equal(out["mel"][u], ref["mel"][u])
    # checkpoint variants (ToucanTTSInterface.py:55-63) against their reference goldens, through the stage API
    for name in ("V20_monolingual", "V20_single"):
        g = _gold(name)
        sd = fw.acoustic_state_dict(**json.loads(str(g["fixture"])))
        pipe = native.NativePipeline(sd, None, None, DEV)
        assert pipe.multilingual is False and pipe.multispeaker is (name == "V20_monolingual")
        out = pipe.forward([torch.from_numpy(g["text"])], torch.from_numpy(g["utt_emb"])[None], [int(g["lang_id"])], z_noise=[torch.from_numpy(g["z"])])
        assert np.array_equal(out["durations"][0].cpu().numpy(), g["durations"])
        err = np.abs(out["mel"][0].cpu().numpy() - g["mel"])
        assert err.max() < 5e-4 and err.mean() < 1e-4, name


def test_synthesize_batch_one_call_and_error_paths(pipes):
    """tts_synthesize_batch through ctypes: the whole pass in ONE call; too small a waveform buffer and a missing weight come back
    as error codes with a message."""
    pipe = pipes["hifigan"]
    lib, h = pipe.lib, pipe.h
    gs = [_gold("L20_pred"), _gold("L7_pred")]
    texts, embs, langs, zs = _inputs(gs)
    ref = pipe.forward(texts, embs, langs, z_noise=zs)
    B = 2
    text = torch.cat(texts).to(DEV).contiguous()
    emb = embs.to(DEV).contiguous()
    lang = torch.tensor(langs, dtype=torch.int32, device=DEV)
    lens = (C.c_int32 * B)(*[int(t.shape[0]) for t in texts])
    rag_s = ref["rag_frame"].halved()
    z_sq = torch.zeros(ref["rag_frame"].total_rows // 2, 160, device=DEV)
    for zu, b0, n in zip(zs, rag_s.begins, rag_s.lengths):
        z_sq[b0:b0 + n].copy_(zu.t()[: 2 * n].reshape(n, 160))
    fb, fc = (C.c_int32 * B)(), (C.c_int32 * B)()
    need = C.c_int64()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: C.c_void_p(t.data_ptr())
    tiny = torch.empty(16, device=DEV)
    rc = lib.tts_synthesize_batch(h, p(text), p(emb), p(lang), lens, B, None, None, None, 1.0, 1.0, 1.0, 1.0, p(z_sq), fb, fc, p(tiny), 16,
                                  C.byref(need), st)
    assert rc != 0 and b"samples" in lib.tts_last_error() and need.value == ref["wav"].numel()
    wav = torch.empty(need.value, device=DEV)
    rc = lib.tts_synthesize_batch(h, p(text), p(emb), p(lang), lens, B, None, None, None, 1.0, 1.0, 1.0, 1.0, p(z_sq), fb, fc, p(wav),
                                  need.value, C.byref(need), st)
    assert rc == 0, lib.tts_last_error()
    torch.cuda.synchronize()
    for u in range(B):
        b, n = ref["wav_spans"][u]
        assert (384 * fb[u], 384 * fc[u]) == (b, n)
        assert torch.equal(wav[b:b + n], ref["wav"][b:b + n])
    # a handle without weights reports what is missing
    h2 = C.c_void_p()
    cfg = capi.TtsConfig(1, 1, 0, 0, 0, 0.0)
    assert lib.tts_create(C.byref(cfg), C.byref(h2)) == 0
    assert lib.tts_encoder(h2, p(text), p(emb), p(lang), lens, B, st) != 0 and b"was not loaded" in lib.tts_last_error()
    assert lib.tts_destroy(h2) == 0
    assert pipe.workspace_bytes(32, 128, 640) > pipe.workspace_bytes(1, 128, 640) > 0


@pytest.mark.parametrize("precision,kind", [("f32", "bigvgan"), ("bf16", "bigvgan"), ("f32", "hifigan")])
def test_workspace_bound_covers_what_a_batch_claims(precision, kind):
    """tts_workspace_bytes(B, Lmax, Tmax) is an upper bound of what the arenas really hold after a batch of that shape
    (tts_workspace_claimed) - and not a wild one (within 2x for a ragged batch described by its maxima): a caller budgets HBM from it."""
    voc_sd = fw.bigvgan_state_dict() if kind == "bigvgan" else fw.hifigan_state_dict()
    pipe = native.NativePipeline(fw.acoustic_state_dict(), voc_sd, kind, DEV, precision=precision)
    for names in (("R20",), ("R128", "R97", "R64", "R20")):
        gs = [_gold(n) for n in names]
        texts, embs, langs, zs = _inputs(gs)
        durs = [torch.from_numpy(g["gold_durations"]) for g in gs]
        pipe.forward(texts, embs, langs, durations=durs, z_noise=zs)
        torch.cuda.synchronize()
        B, Lmax, Tmax = len(gs), max(t.shape[0] for t in texts), max(int(d.sum()) for d in durs)
        bound, claimed = pipe.workspace_bytes(B, Lmax, Tmax), pipe.workspace_claimed()
        assert claimed > 0 and bound >= claimed, (names, bound, claimed)
        assert bound < 2 * claimed + (256 << 20), (names, bound, claimed)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_pipelined_batches_equal_one_batch_at_a_time(precision):
    """forward_pipelined (acoustic model of batch k+1 on one HIP stream beside the vocoder of batch k on another): six batches
    of different shapes, twice over, give bit for bit what forward() gives batch by batch."""
    names = [("R128", "R20"), ("R97",), ("R64", "R128", "R97"), ("R20",), ("R128", "R97", "R64", "R20"), ("R64", "R20")]
    pipe = native.NativePipeline(fw.acoustic_state_dict(), fw.bigvgan_state_dict(), "bigvgan", DEV, precision=precision)
    batches = []
    for group in names * 2:
        gs = [_gold(n) for n in group]
        texts, embs, langs, zs = _inputs(gs)
        batches.append(dict(texts=[t.to(DEV) for t in texts], utt_embs=embs.to(DEV), lang_ids=langs, z_noise=[z.to(DEV) for z in zs],
                            durations=[torch.from_numpy(g["gold_durations"]).to(DEV) for g in gs]))
    want = []
    for kw in batches:
        out = pipe.forward(**kw)
        want.append(([m.clone() for m in out["mel"]], out["wav"].clone(), list(out["wav_spans"])))
    torch.cuda.synchronize()
    got = list(pipe.forward_pipelined(batches))
    assert len(got) == len(want)
    for k, (out, (mel, wav, spans)) in enumerate(zip(got, want)):
        assert out["wav_spans"] == spans
        for m_got, m_want in zip(out["mel"], mel):  # (alignment rows between utterances are never written: compare utterance by utterance)
            assert torch.equal(m_got, m_want), k
        for b0, n in spans:
            assert torch.equal(out["wav"][b0:b0 + n], wav[b0:b0 + n]), (k, b0, n, float((out["wav"][b0:b0 + n] - wav[b0:b0 + n]).abs().max()))


def test_mixed_precision_pipeline_is_the_fp32_acoustic_model_plus_the_fp16_vocoder():
    """NativePipeline(precision="f32", vocoder_precision="f16") (two handles): the mel is bit for bit the fp32 pipeline's - so it
    carries the fp32 configuration's parity with the reference goldens - and the waveform is bit for bit what the fp16 pipeline's
    vocoder makes of that mel."""
    gs = [_gold(n) for n in ("R128", "R97", "R64", "R20")]
    texts, embs, langs, zs = _inputs(gs)
    durs = [torch.from_numpy(g["gold_durations"]) for g in gs]
    ac_sd, voc_sd = fw.acoustic_state_dict(), fw.bigvgan_state_dict()
    mixed = native.NativePipeline(ac_sd, voc_sd, "bigvgan", DEV, precision="f32", vocoder_precision="f16")
    exact = native.NativePipeline(ac_sd, voc_sd, "bigvgan", DEV, precision="f32")
    half = native.NativePipeline(ac_sd, voc_sd, "bigvgan", DEV, precision="f16")
    out = mixed.forward(texts, embs, langs, durations=durs, z_noise=zs)
    ref = exact.forward(texts, embs, langs, durations=durs, z_noise=zs, vocode=False)
    for m_got, m_want, g in zip(out["mel"], ref["mel"], gs):
        assert torch.equal(m_got, m_want)
        assert np.abs(m_got.cpu().numpy() - g["mel"]).mean() < 1e-4  # the north-star bound, against the reference's own output
    wav, rag = half.vocode(ref["mel_packed"], ref["rag_mel"])
    for (b0, n), (b1, n1) in zip(out["wav_spans"], zip(rag.begins, rag.lengths)):
        assert n == n1 and torch.equal(out["wav"][b0:b0 + n], wav[b1:b1 + n1])
    assert mixed.workspace_bytes(4, 128, 640) > 0


def _fresh_layouts_then_replay(kind):
    ac_sd, voc_sd = fw.acoustic_state_dict(), (fw.hifigan_state_dict() if kind == "hifigan" else fw.bigvgan_state_dict())
    pipe = native.NativePipeline(ac_sd, voc_sd, kind, DEV)
    ac, voc = engine.AcousticEngine(ac_sd, DEV), engine.VocoderEngine(voc_sd, kind, DEV)
    batches = []
    for k in range(12):
        Ls = [9 + 5 * k + 3 * u for u in range(1 + k % 3)]
        feats = [torch.from_numpy(syn.utterance_features(800 + 10 * k + u, L)) for u, L in enumerate(Ls)]
        embs = torch.from_numpy(np.stack([syn.utterance_embedding(800 + 10 * k + u) for u in range(len(Ls))]))
        durs = [torch.from_numpy(syn.ragged_durations(800 + 10 * k + u, f.numpy())) for u, f in enumerate(feats)]
        zs = [torch.from_numpy(syn.postflow_noise(800 + 10 * k + u, int(d.sum()))) for u, d in enumerate(durs)]
        batches.append(dict(texts=feats, utt_embs=embs, lang_ids=[syn.LANG_EN] * len(Ls), durations=durs, z_noise=zs))
    want = []
    for kw in batches:
        ref = ac.forward(kw["texts"], kw["utt_embs"], kw["lang_ids"], durations=kw["durations"], z_noise=kw["z_noise"])
        w, rw = voc.forward(ref["mel_packed"], ref["rag_mel"])
        want.append(([m.clone() for m in ref["mel"]], [w[b0:b0 + n].clone() for b0, n in zip(rw.begins, rw.lengths)]))
    torch.cuda.synchronize()
    a0, c0 = pipe.table_stats()
    got = list(pipe.forward_pipelined(batches))
    torch.cuda.synchronize()
    a1, c1 = pipe.table_stats()
    assert a1 - a0 >= 12 * 6 and c1 > 4, (kind, a0, c0, a1, c1)
    for out, (mels, wavs) in zip(got, want):
        for m_got, m_want in zip(out["mel"], mels):
            assert torch.equal(m_got, m_want)
        for (b0, n), w_want in zip(out["wav_spans"], wavs):
            assert torch.equal(out["wav"][b0:b0 + n], w_want)
    again = list(pipe.forward_pipelined(batches[:3]))  # (replayed, batch k takes the generation that kept its tables)
    torch.cuda.synchronize()
    a2, c2 = pipe.table_stats()
    assert a2 == a1, (kind, a1, c1, a2, c2)
    for out, (mels, wavs) in zip(again, want[:3]):
        for m_got, m_want in zip(out["mel"], mels):
            assert torch.equal(m_got, m_want)
        for (b0, n), w_want in zip(out["wav_spans"], wavs):
            assert torch.equal(out["wav"][b0:b0 + n], w_want)


def test_fresh_layouts_build_tables_and_replayed_batches_build_none():
    """Real traffic: every batch has utterance lengths never seen before.  Twelve such batches through the two-stream pipeline, with
    HiFiGAN and with BigVGAN (fp32: BigVGAN takes the non-fused path, whose snake table is held across conv launches that add
    tables): each builds its tile tables, the table store chains chunks while they run (one handle starts with 2 stage groups x 2
    generations = 4), and every result equals the Python sequencer's (own tables, own path) bit for bit.  Three of the batches
    replayed find all their tables in the generation that kept them: nothing is built or uploaded, and the bits are the same."""
    for kind in ("hifigan", "bigvgan"):
        _fresh_layouts_then_replay(kind)


def _without(*names):
    """NativePipeline whose upload leaves the tensors `names` out."""
    class Dropping(native.NativePipeline):
        def _load(self, name, t):
            if name not in names:
                super()._load(name, t)
    return Dropping


def test_a_missing_late_stage_tensor_is_reported_up_front():
    """The model is resolved at the first stage entry of a pass: a handle that lacks a tensor of the LAST acoustic stage (PostFlow)
    fails in tts_encoder, one that lacks a tensor of the vocoder's last residual block at the top of tts_vocoder_hifigan - both by
    name, and before anything was reserved or launched (the handle's arenas are still empty)."""
    texts, embs, langs, _ = _inputs([_gold("L7_pred")])
    pipe = _without("flow.17.winv", "voc.blk.3.2.2.c2.w")(fw.acoustic_state_dict(), fw.hifigan_state_dict(), "hifigan", DEV)
    lib, st = pipe.lib, torch.cuda.current_stream().cuda_stream
    packed = pipe.pack_inputs(texts, embs, langs)
    lens = (C.c_int32 * 1)(*packed["Ls"])
    assert packed["Ls"] == [7]
    assert lib.tts_encoder(pipe.h, native.ptr(packed["text"]), native.ptr(packed["emb"]), native.ptr(packed["lang"]), lens, 1, st) != 0
    err = lib.tts_last_error()
    assert b"flow.17.winv" in err and b"was not loaded" in err, err
    assert int(lib.tts_workspace_claimed(pipe.h)) == 0
    mel = torch.zeros(7, 80, device=DEV)
    wav = torch.empty(7 * 384, device=DEV)
    fb, fc = (C.c_int32 * 1)(0), (C.c_int32 * 1)(7)
    assert lib.tts_vocoder_hifigan(pipe.h_voc, native.ptr(mel), 80, fb, fc, 1, native.ptr(wav), st) != 0
    err = lib.tts_last_error()
    assert b"voc.blk.3.2.2.c2.w" in err and b"was not loaded" in err, err
    assert int(lib.tts_workspace_claimed(pipe.h_voc)) == 0


def test_a_re_uploaded_tensor_is_resolved_again():
    """tts_load_weights on a name the handle holds frees the old allocation: the next pass must resolve the model again.  A pass,
    out_norm.b + 0.5 uploaded over the old one, a pass: the mel of a fresh pipeline built with that bias, bit for bit; the original
    uploaded again: the first mel, bit for bit."""
    texts, embs, langs, _ = _inputs([_gold("L7_pred")])
    sd = fw.acoustic_state_dict()
    key = "encoder.output_norm.bias"
    shifted = sd[key] + np.float32(0.5)
    # (seeded noise, not the golden's: the shifted bias may change the predicted frame count)
    run = lambda p: p.forward(texts, embs, langs, generator=torch.Generator(device=DEV).manual_seed(5))["mel"][0].clone()
    pipe = native.NativePipeline(sd, None, None, DEV)
    first = run(pipe)
    pipe._load("out_norm.b", torch.from_numpy(shifted))
    second = run(pipe)
    assert not torch.equal(second, first)
    assert torch.equal(second, run(native.NativePipeline(dict(sd, **{key: shifted}), None, None, DEV)))
    pipe._load("out_norm.b", torch.from_numpy(sd[key]))
    assert torch.equal(run(pipe), first)


def test_predict_frame_counts_is_stage_a_of_forward():
    """predict_frame_counts (the multi-GPU deal's balancing key) and forward() share stage A: same frame counts, with the default
    controls and with all four scales."""
    us, Ls = [300, 301, 302], [48, 21, 33]
    feats = [torch.from_numpy(syn.utterance_features(u, L)) for u, L in zip(us, Ls)]
    embs = torch.from_numpy(np.stack([syn.utterance_embedding(u) for u in us]))
    langs = [syn.LANG_EN] * 3
    pipe = native.NativePipeline(fw.acoustic_state_dict(), None, None, DEV)
    for kw in ({}, dict(duration_scaling_factor=0.9, pitch_variance_scale=1.2, energy_variance_scale=0.8, pause_duration_scaling_factor=1.3)):
        want = [int(n) for n in pipe.forward(feats, embs, langs, vocode=False, **kw)["rag_frame"].lengths]
        assert pipe.predict_frame_counts(feats, embs, langs, **kw) == want and len(want) == 3 and min(want) > 0, kw
