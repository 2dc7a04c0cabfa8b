"""The prosody cloner's kernels (csrc/align.hip) on the MI355X: each against the restatement in tests/aligner_ref.py, then the
extraction path end to end against the reference goldens (tests/golden/aligner/aligner.npz), batch against one by one, and the
UtteranceCloner interface against the plain synthesis call with the same prosody."""
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, capi, fixture_weights as fw, phonemes
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import aligner_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
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
def eng():
    return align.AlignerEngine(fw.aligner_state_dict(), DEV)


@pytest.fixture(scope="module")
def extractor():
    return align.ProsodyExtractor(fw.aligner_state_dict(), DEV)


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def test_lstm_recurrence_on_ragged_lengths(eng):
    """Lengths 1, 2, 37, 640 and 2000 in one batch against a float64 recurrence; the state buffers are poisoned with NaN, so a step
    that read state it never received would show.  Each utterance alone gives the batch's rows bit for bit (both directions)."""
    H = eng.H
    lens = [1, 2, 37, 640, 2000]
    rag = Ragged(lens, DEV)
    xproj = fw.normal("lstm.x", (rag.total_rows, 8 * H), 5, 0.5)
    y = eng.lstm(_t(xproj), rag, poison_state=True).cpu().numpy()
    assert np.isfinite(y).all()
    ref = ar.lstm_reference(xproj, eng.w_hh_t, lens, H)
    err = np.abs(y - ref).max()
    print(f"lstm max abs error vs float64: {err:.2e}")
    assert err < 2e-4
    for b, (b0, n) in enumerate(zip(rag.begins, lens)):
        one = eng.lstm(_t(xproj[b0:b0 + n]), Ragged([n], DEV), poison_state=True).cpu().numpy()
        assert np.array_equal(one, y[b0:b0 + n]), b
        # the reverse direction starts at the utterance's own last frame: its first step sees no state
        assert np.array_equal(one[n - 1, H:], eng.lstm(_t(xproj[b0 + n - 1:b0 + n]), Ragged([1], DEV)).cpu().numpy()[0, H:])


def _mas_gpu(eng, cases, flags=None, force_scratch=False):
    """MAS through the kernel for a list of [T, L] matrices (L <= 145: put in the first L columns of the logits) or of (logits
    [T, 145], token ids) pairs."""
    cases = [c if isinstance(c, tuple) else (c, np.arange(c.shape[1], dtype=np.int32)) for c in cases]
    rag = Ragged([m.shape[0] for m, _ in cases], DEV)
    lg = np.zeros((rag.total_rows, align.N_SYMBOLS), np.float32)
    for (m, _), b0 in zip(cases, rag.begins):
        lg[b0:b0 + m.shape[0], :m.shape[1]] = m
    ids = [np.asarray(i, dtype=np.int32) for _, i in cases]
    flags = flags or [np.zeros(len(i), np.int32) for i in ids]
    d, begins = eng.durations(_t(lg), rag, ids, flags, force_scratch)
    d = d.cpu().numpy()
    return [d[b:b + len(f)] for b, f in zip(begins, flags)]


@pytest.mark.parametrize("force_scratch", [False, True])
def test_mas_kernel_on_the_golden_cases(eng, force_scratch):
    mats = [(G[f"mas{c}_logits"], G[f"mas{c}_ids"]) for c in STORED]
    k = 0
    while f"tie{k}_p" in G.files:
        mats.append(G[f"tie{k}_p"])
        k += 1
    want = [G[f"mas{c}_dur"] for c in STORED] + [G[f"tie{j}_dur"] for j in range(k)]
    for got, w in zip(_mas_gpu(eng, mats, force_scratch=force_scratch), want):
        assert np.array_equal(got, w)


@pytest.mark.parametrize("force_scratch", [False, True])
def test_mas_kernel_on_random_matrices(eng, force_scratch):
    """200 seeded random matrices (T < L included): identical to the float32 restatement with the kernel's correctly rounded log;
    against numpy's float32 log (the reference's) any difference must be a near tie in float64 rescoring."""
    rng = np.random.default_rng(7)
    mats = []
    for _ in range(200):
        T, L = int(rng.integers(1, 300)), int(rng.integers(1, 90))
        mats.append((rng.standard_normal((T, L)) * rng.choice([0.1, 1.0, 5.0])).astype(np.float32))
    got = _mas_gpu(eng, mats, force_scratch=force_scratch)
    flips = 0
    for m, g in zip(mats, got):
        assert np.array_equal(g, ar.mas(m, log64=True)[0])
        ref = ar.mas(m)[0]
        if not np.array_equal(g, ref):
            flips += 1
            s0, s1 = ar.mas_float64_score(m, g), ar.mas_float64_score(m, ref)
            assert abs(s0 - s1) <= 1e-5 * max(1.0, abs(s1)), (s0, s1)
    print(f"MAS ({'scratch' if force_scratch else 'LDS'}): {flips} of 200 random matrices differ from numpy's float32 log, all near ties")


def test_mas_postprocessing_in_the_kernel(eng):
    """Word-boundary zeros and the 3/5 - 2/5 repair, chains of three included, against the restatement."""
    rng = np.random.default_rng(3)
    mats, flags = [], []
    for L_full in (5, 9, 14, 30):
        f = np.zeros(L_full, np.int32)
        f[rng.choice(L_full, L_full // 4, replace=False)] |= 1
        f[1:][rng.random(L_full - 1) < 0.4] |= 2
        f[0] &= ~1  # the first token is never a boundary: at least one token is aligned
        n = int(((f & 1) == 0).sum())
        mats.append(rng.standard_normal((3 * L_full, n)).astype(np.float32))
        flags.append(f)
    got = _mas_gpu(eng, mats, flags=flags)
    for m, f, g in zip(mats, flags, got):
        assert np.array_equal(g, ar.postprocess(ar.mas(m, log64=True)[0], f)), f


def test_frame_energy_and_token_averages(extractor):
    ops = extractor.ops
    rng = np.random.default_rng(11)
    rows, bins = 300, 513
    spec = rng.standard_normal((rows, 2 * bins)).astype(np.float32)
    spec[5] = 0.0
    y = torch.empty(rows, dtype=torch.float32, device=DEV)
    sd = _t(spec)
    capi.check(ops.lib.tts_frame_energy(sd.data_ptr(), 2 * bins, bins, y.data_ptr(), rows, ops.stream()))
    ref = ar.frame_energy(spec, bins)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=2e-6)
    assert abs(y[5].item() - 1e-5) <= 1e-11  # sqrt of the 1e-10 floor
    lens = [40, 1, 259]
    rag = Ragged(lens, DEV)
    x = np.abs(rng.standard_normal(rag.total_rows)).astype(np.float32)
    x[rng.random(rag.total_rows) < 0.3] = 0.0
    durs, keeps = [], []
    for n in lens:
        L = max(1, n // 7)
        cuts = np.sort(rng.integers(0, n + 1, L - 1))
        durs.append(np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int32))
        k = rng.random(L) > 0.2
        k[0] = True
        keeps.append(k)
    n_full = [len(d) for d in durs]
    full_begin = list(np.concatenate([[0], np.cumsum(n_full)[:-1]]))
    dd = _t(np.concatenate(durs), torch.int32)
    for mode in (0, 1):
        out = extractor.token_average(_t(x), rag, dd, np.concatenate(keeps), full_begin, n_full, mode).cpu().numpy()
        for b, (b0, n) in enumerate(zip(rag.begins, lens)):
            want = ar.token_average(x[b0:b0 + n], durs[b], keeps[b], mode)
            got = out[full_begin[b]:full_begin[b] + n_full[b]]
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7, equal_nan=True)


def test_aligner_end_to_end_against_the_reference(eng):
    """Logits within 1e-5 of the reference's largest |logit| (fp32 MFMA), durations exact, on every golden mel - in one batch - and
    the batch equals each utterance alone bit for bit."""
    mels = [mas_mel(c) for c in range(N_MAS)]
    ids = [G[f"mas{c}_ids"] for c in range(N_MAS)]
    durs = eng.align(mels, ids, poison_state=True)
    lg = eng.last_logits.cpu().numpy()
    rag = eng.last_rag
    worst = 0.0
    for c in range(N_MAS):
        assert np.array_equal(durs[c].numpy(), G[f"mas{c}_dur"]), c
    for c in STORED:  # (the long case's reference logits are not stored; its durations are checked above)
        ref = G[f"mas{c}_logits"]
        got = lg[rag.begins[c]:rag.begins[c] + rag.lengths[c]]
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f"aligner logits: largest error {worst:.2e} of the largest |logit|")
    assert worst <= 1e-5
    for c in range(N_MAS):
        one = eng.align([mels[c]], [ids[c]])
        assert torch.equal(one[0], durs[c])
        got = eng.last_logits.cpu().numpy()[:rag.lengths[c]]
        assert np.array_equal(got, lg[rag.begins[c]:rag.begins[c] + rag.lengths[c]]), c
    # the scratch form of MAS on the same logits
    assert all(torch.equal(a, b) for a, b in zip(eng.align(mels, ids, force_scratch=True), durs))


def test_extraction_end_to_end_against_extract_prosody(extractor):
    """The whole extraction (golden mel and normalised wave, seeded f0) == the reference's extract_prosody: durations exact, energy
    and pitch within 1e-5; the batch equals each utterance alone bit for bit."""
    feats = [phonemes.phones_to_features(str(G["clone_phones"][u]), handle_missing=False) for u in range(N_CLONE)]
    waves = [clone_wave(u)[1] for u in range(N_CLONE)]
    f0 = [G[f"clone{u}_f0"] for u in range(N_CLONE)]
    mels = [G[f"clone{u}_mel"] for u in range(N_CLONE)]
    res = extractor.extract(feats, waves, f0=f0, mels=mels)
    for u, (d, p, e) in enumerate(res):
        assert np.array_equal(d.numpy(), G[f"clone{u}_dur"]), u
        e_err = float(np.abs(e.numpy() - G[f"clone{u}_energy"]).max())
        p_err = float(np.abs(p.numpy() - G[f"clone{u}_pitch"]).max())
        print(f"clone case {u}: energy err {e_err:.1e}, pitch err {p_err:.1e}")
        assert e_err <= 1e-5 and p_err <= 1e-5
        one = extractor.extract([feats[u]], [waves[u]], f0=[f0[u]], mels=[mels[u]])[0]
        assert all(torch.equal(a, b) for a, b in zip(one, (d, p, e))), u
    # the front end's own log-mel (style.LogMel's arithmetic) instead of the stored one: a batch still equals its utterances
    both = extractor.extract(feats[:2], waves[:2])
    for u in range(2):
        one = extractor.extract([feats[u]], [waves[u]])[0]
        assert torch.equal(one[0], both[u][0]) and torch.equal(one[2], both[u][2]) and one[1] is None


def test_utterance_cloner_interface(tmp_path, monkeypatch):
    """The reference's script form: phoneme transcript, fixture checkpoints; the cloned wave equals the plain call with the extracted
    prosody, and the extracted prosody is what extract_prosody_batch gives for the same recording."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    from InferenceInterfaces.UtteranceCloner import UtteranceCloner
    u = 1
    phones = str(G["clone_phones"][u])
    ref_wav = str(tmp_path / "ref.wav")
    interface.write_wav(ref_wav, clone_wave(u)[0], 16000)
    cl = UtteranceCloner(model_id=str(models / "ToucanTTS_Meta" / "best.pt"), device=DEV, language="en")
    with pytest.warns(UserWarning):
        d, p, e, s0, s1 = cl.extract_prosody(phones, ref_wav, lang="en", f0=G[f"clone{u}_f0"])
    assert s0 == 0 and s1 == 0 and d.shape == p.shape == e.shape and int(d.sum()) > 0
    batch = cl.extract_prosody_batch([phones, str(G["clone_phones"][0])], [interface_wave(ref_wav), clone_wave(0)[0]], 16000,
                                     f0=[G[f"clone{u}_f0"], G["clone0_f0"]])
    assert torch.equal(batch[0][0], d) and torch.equal(batch[0][1], p) and torch.equal(batch[0][2], e)
    out = tmp_path / "cloned.wav"
    d2, p2, e2, s0, s1 = cl.extract_prosody(phones, ref_wav, lang="en", f0=G[f"clone{u}_f0"], speech_bounds=(256, 256 * 250))
    assert s0 == 256 and s1 == len(interface_wave(ref_wav)) - 256 * 250
    z2 = torch.from_numpy(fw.normal("clone.z", (80, int(d2.sum())), 1, 0.8))
    cloned = cl.clone_utterance(ref_wav, ref_wav, phones, filename_of_result=str(out), lang="en", f0=G[f"clone{u}_f0"], z_noise=z2,
                                speech_bounds=(256, 256 * 250))
    plain = cl.tts(phones, durations=d2, pitch=p2, energy=e2, input_is_phones=True, z_noise=z2).cpu().numpy()
    assert np.array_equal(cloned[3 * s0:len(cloned) - 3 * s1], plain)
    assert not cloned[:3 * s0].any() and not cloned[len(cloned) - 3 * s1:].any()
    assert np.array_equal(cl.tts.last_durations[0].cpu().numpy(), d2.numpy())
    assert out.stat().st_size > 2 * len(cloned)
    z = torch.from_numpy(fw.normal("clone.z", (80, int(d.sum())), 1, 0.8))
    angel = cl.biblical_accurate_angel_mode(ref_wav, phones, [ref_wav, ref_wav], lang="en", f0=G[f"clone{u}_f0"], z_noise=[z, z])
    assert np.isfinite(angel).all() and len(angel) > 0


def interface_wave(path):
    from ims_toucan_prosody_variance_amd import style
    return style.read_audio(path)[0]
