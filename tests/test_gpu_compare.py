"""The comparison kernels (csrc/compare.hip) on the MI355X against the float64 restatement in tests/compare_ref.py: the warping of
the seeded cases in one ragged batch (both forms of the back-pointer store, and each case alone), the cepstra, the sums along the
restatement's paths, ``SpeechComparator.compare`` end to end, and the two entry points of the interface."""
import math
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, compare, fixture_weights as fw, resample, style
from tests import compare_ref as cr, pitch_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = len(cr.CASE_SIZES)
COUNTS = [cr.SUM_COLUMNS.index(c) for c in ("diag", "vv", "gross", "vuv")]
DB = 10.0 / math.log(10.0)


@pytest.fixture(scope="module")
def cmp():
    return compare.SpeechComparator(DEV)


def packed(which):
    """The cases `which` as one ragged batch: (cepstra a, frames a, cepstra b, frames b), the cepstra on the device."""
    t = lambda arrays: torch.from_numpy(np.concatenate(arrays)).to(DEV)
    a, b = [cr.cases()[n][0] for n in which], [cr.cases()[n][1] for n in which]
    return t(a), [len(x) for x in a], t(b), [len(x) for x in b]


def same(x, y):
    """Two result dicts hold the same bits (NaN equal to NaN)."""
    return x.keys() == y.keys() and all(np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=np.asarray(x[k]).dtype.kind == "f") for k in x)


# ---- tts_dtw ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_runs(cmp):
    """All the cases in one ragged batch, once per form of the back-pointer store: {force_scratch: (costs, paths)}."""
    return {force: cmp.dtw(*packed(range(N)), force_scratch=force) for force in (False, True)}


@pytest.mark.parametrize("force_scratch", [False, True])
def test_dtw_batch_against_the_restatement(batch_runs, force_scratch):
    """The path is exactly the restatement's and the cost within 1e-12 relative (at most 8191 fp64 additions of correctly rounded
    terms, with room for the contraction of the squares in d).  Without force_scratch the cases lie on both sides of the LDS form's
    limit."""
    sizes = [compare.bp_bytes(ta, tb) for ta, tb in cr.CASE_SIZES]
    assert any(s <= capi.DTW_LDS_BP_BYTES for s in sizes) and any(s > capi.DTW_LDS_BP_BYTES for s in sizes)
    costs, paths = batch_runs[force_scratch]
    assert costs.dtype == np.float64 and len(costs) == len(paths) == N
    for n in range(N):
        ref = cr.solved(n)
        assert paths[n].dtype == np.int32 and np.array_equal(paths[n], ref["path"]), cr.CASE_SIZES[n]
        rel = abs(costs[n] - ref["cost"]) / ref["cost"]
        print(f"case {cr.CASE_SIZES[n]}: cost {costs[n]:.12g}, relative error {rel:.2e}")
        assert rel <= 1e-12, cr.CASE_SIZES[n]
    assert np.array_equal(batch_runs[False][0], batch_runs[True][0])


def test_dtw_each_case_alone_returns_the_bits_of_the_batch(cmp, batch_runs):
    costs, paths = batch_runs[False]
    for n in range(N):
        cost, path = cmp.dtw(*packed([n]))
        assert cost[0] == costs[n] and np.array_equal(path[0], paths[n]), cr.CASE_SIZES[n]


def test_dtw_refuses_what_it_cannot_lay_out(cmp):
    """The library names the pair: too many frames, and back-pointers that fit neither store."""
    a, fa, b, fb = packed([2, 3])
    lib = cmp.ops.lib
    table, dev, total, lds, entries, _ = cmp._pair_table(fa, fb, False)
    out = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=DEV)
    path, path_len, cost = out(entries, 2), out(2), out(2, dtype=torch.float64)
    call = lambda lds_bytes: lib.tts_dtw(a.data_ptr(), sum(fa), b.data_ptr(), sum(fb), 13, table, dev.data_ptr(), 2, None, 0, lds_bytes,
                                         path.data_ptr(), entries, path_len.data_ptr(), cost.data_ptr(), cmp.ops.stream())
    assert call(lds - 16) == -1 and b"pair 1" in lib.tts_last_error()
    table[0].frames_a = capi.DTW_MAX_FRAMES + 1
    assert call(lds) == -1 and b"pair 0" in lib.tts_last_error()
    table[0].frames_a = 0
    assert call(lds) == -1 and b"pair 0" in lib.tts_last_error()
    with pytest.raises(ValueError, match="pair 0, side b"):
        cmp.dtw(a, fa, b, [0, fb[0] + fb[1]])


# ---- tts_mel_cepstra ------------------------------------------------------------------------------------------------------------
def test_cepstra_against_the_correctly_rounded_restatement(cmp):
    """Log-mels of the pitch tracker's short test signals (silence, a DC offset and the shortest wave among them): every coefficient
    within one float32 ulp of the correctly rounded value."""
    from ims_toucan_prosody_variance_amd import align
    waves = [pr.signals()[n][0] for n in pr.SHORT]
    spec, rag = align.batched_spectra(cmp.ops, cmp.logmel, waves)
    mel = align.batched_log_mel(cmp.ops, cmp.logmel, spec, rag)
    rows = np.concatenate([np.arange(b, b + n) for b, n in zip(rag.begins, rag.lengths)])  # (the rows between the waves hold no frames)
    got = cmp.mel_cepstra(mel).cpu().numpy()[rows]
    want = cr.cepstra(mel.cpu().numpy()[rows])
    assert got.shape == want.shape == (sum(rag.lengths), 13) and got.dtype == np.float32
    differ = got != want
    print(f"cepstra of {got.shape[0]} rows: {differ.mean():.3%} of the values differ from the correctly rounded ones")
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()
    # the packed form: the frames of every wave, one after the other
    cep, frames = cmp.cepstra(waves)
    assert frames == [1 + len(w) // 256 for w in waves]
    assert np.array_equal(cep.cpu().numpy(), got)
    # more coefficients, and a source row that does not exist
    wide = compare.SpeechComparator(DEV, n_cep=32)
    few = mel[:37].contiguous()  # frames of the first wave
    got32 = wide.mel_cepstra(few).cpu().numpy()
    want32 = cr.cepstra(few.cpu().numpy(), 32)
    assert (np.abs(got32.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)).all()
    assert np.array_equal(got32[:, :13], got[:37])
    picked = cmp.mel_cepstra(few, torch.tensor([3, 37, 0, -1], dtype=torch.int32, device=DEV)).cpu().numpy()
    assert np.array_equal(picked[[0, 2]], got[[3, 0]]) and np.isnan(picked[[1, 3]]).all()


# ---- tts_dtw_path_sums ----------------------------------------------------------------------------------------------------------
def test_path_sums_against_the_restatement(cmp):
    """Along the restatement's paths, with seeded f0 tracks that are voiceless in stretches on both sides: every sum within 1e-12
    relative, the four counts exact; without f0 the F0 columns stay zero."""
    a, fa, b, fb = packed(range(N))
    paths = [cr.solved(n)["path"] for n in range(N)]
    f0_a = np.concatenate([cr.f0_tracks(n)[0] for n in range(N)])
    f0_b = np.concatenate([cr.f0_tracks(n)[1] for n in range(N)])
    got = cmp.path_sums(a, fa, b, fb, paths, f0_a, f0_b)
    plain = cmp.path_sums(a, fa, b, fb, paths)
    assert got.shape == plain.shape == (N, compare.N_SUMS) and got.dtype == np.float64
    worst = 0.0
    for n in range(N):
        want = cr.path_sums(*cr.cases()[n], paths[n], *cr.f0_tracks(n))
        rel = np.abs(got[n] - want) / np.where(want != 0, np.abs(want), 1.0)
        worst = max(worst, float(rel.max()))
        assert (rel <= 1e-12).all(), (cr.CASE_SIZES[n], dict(zip(cr.SUM_COLUMNS, rel)))
        assert np.array_equal(got[n][COUNTS], want[COUNTS]), cr.CASE_SIZES[n]
        assert np.array_equal(plain[n][:2], got[n][:2]) and not plain[n][2:].any()
    big = cr.CASE_SIZES.index((300, 420))
    counts = dict(zip(cr.SUM_COLUMNS, got[big]))
    assert counts["vv"] > 100 and counts["vuv"] > 20 and 0 < counts["gross"] < counts["vv"]  # the tracks exercise every column
    print(f"path sums of {N} cases: worst relative error {worst:.2e}")
    # a path that leaves its pair: a row of NaN, the neighbour untouched
    bad = [p.copy() for p in paths]
    bad[2][-1, 0] = 9
    marked = cmp.path_sums(a, fa, b, fb, bad)
    assert np.isnan(marked[2]).all() and np.array_equal(np.delete(marked, 2, axis=0), np.delete(plain, 2, axis=0))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def voiced(seed, seconds=2.0, **kw):
    w = pr.glide(seed, seconds=seconds, gap=0.0, **kw)[0]
    return w / np.abs(w).max()  # (already divided by its peak: compare() leaves its bits alone)


def test_a_wave_against_itself(cmp):
    w = voiced(5)
    r = cmp.compare([w], [w], 16000, keep_paths=True)[0]
    T = 1 + len(w) // 256
    assert r["mcd_db"] == 0.0 and r["dtw_cost"] == 0.0 and r["frames_a"] == r["frames_b"] == r["path_length"] == T and r["diag_share"] == 1.0
    assert r["path"].dtype == np.int32 and np.array_equal(r["path"], np.stack([np.arange(T)] * 2, axis=1))
    assert r["vde"] == 0.0 and r["ffe"] == 0.0 and r["gpe"] == 0.0 and r["f0_rmse_hz"] == 0.0 and r["f0_rmse_cents"] == 0.0
    assert abs(r["f0_corr"] - 1.0) <= 1e-12
    assert set(r) == {"mcd_db", "dtw_cost", "path_length", "diag_share", "frames_a", "frames_b", "path"} | set(compare.F0_MEASURES)
    plain = cmp.compare([w], [w], 16000, f0=None)[0]
    assert set(plain) == {"mcd_db", "dtw_cost", "path_length", "diag_share", "frames_a", "frames_b"} and plain["mcd_db"] == 0.0


def test_a_repeated_stretch_lengthens_the_path(cmp):
    """0.2 s (12.5 frames) of the wave repeated in its middle: the path exceeds the shorter side by the inserted frames +- 2."""
    w = voiced(5)
    m = len(w) // 2
    longer = np.concatenate([w[:m], w[m - 3200:m], w[m:]])
    r = cmp.compare([longer], [w], 16000)[0]
    excess = r["path_length"] - min(r["frames_a"], r["frames_b"])
    print(f"{r['frames_a']} x {r['frames_b']} frames, path of {r['path_length']}: {excess} past the shorter side; mcd {r['mcd_db']:.3f} dB")
    assert abs(excess - 3200 / 256) <= 2
    assert r["mcd_db"] > 0 and r["diag_share"] < 1


def test_mcd_against_the_restatement_on_the_devices_cepstra(cmp):
    wa, wb = voiced(6), voiced(7, seconds=1.7)
    cep, frames = cmp.cepstra([wa, wb])
    cep = cep.cpu().numpy()
    a, b = cep[:frames[0]], cep[frames[0]:]
    ref = cr.dtw(a, b)
    want = DB * cr.path_sums(a, b, ref["path"])[0] / len(ref["path"])
    r = cmp.compare([wa], [wb], 16000, f0=None, keep_paths=True)[0]
    print(f"mcd {r['mcd_db']:.6f} dB, restatement {want:.6f} dB, smallest gap {ref['gap']:.2e}")
    assert ref["gap"] >= cr.MIN_GAP and np.array_equal(r["path"], ref["path"])
    assert abs(r["mcd_db"] - want) <= 1e-12 * want and abs(r["dtw_cost"] - ref["cost"]) <= 1e-12 * ref["cost"]


def test_a_batch_equals_its_pairs_alone_however_it_is_split(cmp):
    """Three pairs, two of them past the LDS form: the batch in one launch, split by a scratch bound of one byte (a launch then
    takes one pair that needs the scratch buffer), and every pair alone return the same bits."""
    long_a, long_b = voiced(8, seconds=6.6, lo=80.0, hi=160.0), voiced(9, seconds=6.5, lo=80.0, hi=160.0)
    A, Bs = [voiced(6), long_a, long_b], [voiced(7, seconds=1.7), long_b, long_a]
    assert compare.bp_bytes(1 + len(long_a) // 256, 1 + len(long_b) // 256) > capi.DTW_LDS_BP_BYTES
    whole = cmp.compare(A, Bs, 16000, keep_paths=True)
    assert cmp.last_launches == 1 and len(whole) == 3
    cmp.max_scratch_bytes = 1
    try:
        split = cmp.compare(A, Bs, 16000, keep_paths=True)
        assert cmp.last_launches == 2
    finally:
        cmp.max_scratch_bytes = compare.MAX_SCRATCH_BYTES
    for p in range(3):
        assert same(whole[p], split[p]), p
        assert same(whole[p], cmp.compare([A[p]], [Bs[p]], 16000, keep_paths=True)[0]), p
    assert whole[1]["frames_a"] == whole[2]["frames_b"] and math.isfinite(whole[1]["f0_corr"])


def test_a_24_khz_input_equals_its_resampled_form_fed_directly(cmp):
    """The waves are taken as 24 kHz material; the device resampler's 16 kHz output, fed as 16 kHz, gives the same bits."""
    wa, wb = voiced(10, seconds=1.5, lo=70.0, hi=200.0), voiced(11, seconds=1.8, lo=70.0, hi=200.0)
    rs = resample.Resampler(DEV)
    pre = []
    for w in (wa, wb):
        y, spans = rs.resample(torch.from_numpy(w).to(DEV), [(0, len(w))], 24000, 16000)
        assert spans == [(0, resample.out_length(len(w), 24000, 16000))]
        pre.append(y.cpu().numpy())
    r24 = cmp.compare([wa], [wb], 24000)[0]
    assert same(r24, cmp.compare([pre[0]], [pre[1]], 16000)[0])
    assert same(r24, cmp.compare([wa], [pre[1]], 24000, 16000)[0])
    assert r24["frames_a"] == 1 + len(pre[0]) // 256


def test_compare_refuses_before_it_launches(cmp):
    w = voiced(5, seconds=0.5)
    for args, kw, words in ((([w, w], [w]), {}, "pairs"),
                            (([w, np.append(w[:-1], np.float32("nan"))], [w, w]), {}, "pair 1, side a"),
                            (([w], [w[:512]]), {}, "pair 0, side b.*STFT"),
                            (([w[:1199]], [w]), {}, "pair 0, side a.*tracker"),
                            (([w], [np.zeros(4096 * 256, dtype=np.float32)]), {"f0": None}, "pair 0, side b.*cap"),
                            (([w], [w]), {"f0": "yin"}, "f0 takes")):
        with pytest.raises(ValueError, match=words):
            cmp.compare(*args, 16000, **kw)
    assert cmp.compare([w[:1199]], [w], 16000, f0=None)[0]["frames_a"] == 5
    assert cmp.compare([], [], 16000) == []


# ---- the interface --------------------------------------------------------------------------------------------------------------
PHONES_20 = "~wˈʌns əpˈɑːn mˈɪdnaɪt~#"
PHONES_13 = "~həlˈoʊ wˈɜːld~#"


def test_evaluate_against_recordings(tmp_path, monkeypatch):
    """With fixture checkpoints: the result equals ``SpeechComparator.compare`` on the waves it returns, bit for bit; a recording may
    be a file; prosody keywords reach the synthesis; the sharded path is refused."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    monkeypatch.delenv("TOUCAN_PY_SEQUENCER", raising=False)
    tts = interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)
    tts.set_language("en")
    texts = [PHONES_20, PHONES_13]
    rec_path = str(tmp_path / "rec.wav")
    interface.write_wav(rec_path, 0.5 * voiced(12, seconds=1.1), 16000)
    stereo = np.stack([voiced(13, seconds=0.9), voiced(14, seconds=0.9)], axis=1)
    res = tts.evaluate_against_recordings(texts, [rec_path, (stereo, 22050)], keep_waves=True)
    assert len(res) == 2 and res[0]["recording_sr"] == 16000 and res[1]["recording_sr"] == 22050
    assert np.array_equal(res[0]["recording"], style.read_audio(rec_path)[0]) and np.array_equal(res[1]["recording"], stereo.mean(axis=1))
    again = compare.SpeechComparator(DEV).compare([r["synth"] for r in res], [r["recording"] for r in res], 24000, [16000, 22050])
    for r, a in zip(res, again):
        assert r["synth"].dtype == np.float32 and r["frames_a"] == 1 + resample.out_length(len(r["synth"]), 24000, 16000) // 256
        assert same({k: v for k, v in r.items() if k not in ("synth", "recording", "recording_sr")}, a)
        assert math.isfinite(r["mcd_db"]) and r["mcd_db"] > 0 and 0 <= r["vde"] <= 1
    slow = tts.evaluate_against_recordings(texts, [rec_path, (stereo, 22050)], duration_scaling_factor=[1.5, 1.0], f0=None)
    assert slow[0]["frames_a"] > res[0]["frames_a"] and slow[1]["frames_a"] == res[1]["frames_a"]
    assert set(slow[0]) == {"mcd_db", "dtw_cost", "path_length", "diag_share", "frames_a", "frames_b"}
    for kw in (dict(distributed=True), dict(sample_rate=16000), dict(pcm16=True)):
        with pytest.raises(ValueError):
            tts.evaluate_against_recordings(texts, [rec_path, (stereo, 22050)], **kw)
    with pytest.raises(ValueError):
        tts.evaluate_against_recordings(texts, [rec_path])


def test_clone_utterance_evaluates_on_request(tmp_path, monkeypatch):
    """evaluate=False returns what it returned before; evaluate=True the same waveform and the comparison of the clone with the
    intonation reference."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    from InferenceInterfaces.UtteranceCloner import UtteranceCloner
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aligner", "aligner.npz"))
    phones = str(G["clone_phones"][1])
    ref_wav = str(tmp_path / "ref.wav")
    interface.write_wav(ref_wav, pr.glide(32, seconds=int(G["clone1_samples"]) / 16000.0)[0], 16000)
    cl = UtteranceCloner(model_id=str(models / "ToucanTTS_Meta" / "best.pt"), device=DEV, language="en")
    frames = int(cl.extract_prosody(phones, ref_wav, lang="en", f0="track")[0].sum())
    z = torch.from_numpy(fw.normal("clone.z", (80, frames), 1, 0.8))
    before = cl.clone_utterance(ref_wav, ref_wav, phones, lang="en", f0="track", z_noise=z)
    assert isinstance(before, np.ndarray)
    assert np.array_equal(cl.clone_utterance(ref_wav, ref_wav, phones, lang="en", f0="track", z_noise=z, evaluate=False), before)
    utt, report = cl.clone_utterance(ref_wav, ref_wav, phones, lang="en", f0="track", z_noise=z, evaluate=True)
    assert np.array_equal(utt, before)
    assert set(report) == {"mcd_db", "dtw_cost", "path_length", "diag_share", "frames_a", "frames_b"} | set(compare.F0_MEASURES)
    ref16 = style.normalize_reference_audio(*style.read_audio(ref_wav))
    assert report["frames_b"] == 1 + len(ref16) // 256 and report["frames_a"] == 1 + resample.out_length(len(before), 24000, 16000) // 256
    assert same(report, compare.SpeechComparator(DEV).compare([before], [ref16], 24000, 16000)[0])
