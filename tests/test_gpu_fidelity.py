"""The spectral distances (csrc/fidelity.hip, fidelity.py) on the MI355X: the framing kernel against numpy's reflection padding
byte for byte and, at hop 256, against the host-padded front end; the distance and reduce kernels on given spectra against the
float64 restatement (tests/fidelity_ref.py); the whole measure against the reference's stored losses; a batch against its pairs
alone bit for bit; and the copy-synthesis scorer on the fixture vocoders.

Tolerances are derived, not chosen: four times the largest error of the float32 numpy stand-in of tests/fidelity_ref.py against
the float64 restatement over the very cases of a test.  The figures measured on the MI355X are recorded in DESIGN.md section 21."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, capi, fidelity, fixture_weights as fw, resample, style
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import fidelity_ref as fr
from tests.wave_order import butterfly_order_sum, sequential_order_sum, tree_order_sum

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 0.97  # what lies between the spans of a packed wave: a read across an utterance's edge picks it up
LENGTHS = (769, 384 * 3, 384 * 3 + 1, 5000)  # 769: the smallest the 1536-point STFT admits (3 frames)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fidelity", "mel_loss.npz")


@functools.lru_cache(maxsize=None)
def measure():
    return fidelity.SpectralDistance(DEV)


def pack(waves, gap=0):
    """The waves one after the other with ``gap`` samples of junk in front of each and behind the last -> (packed on the device, spans)."""
    parts, spans, at = [], [], 0
    for i, x in enumerate(waves):
        parts.append(np.full(gap, JUNK if i % 2 else -JUNK, dtype=np.float32))
        at += gap
        spans.append((at, len(x)))
        parts.append(np.asarray(x, dtype=np.float32))
        at += len(x)
    parts.append(np.full(gap, JUNK, dtype=np.float32))
    return torch.from_numpy(np.concatenate(parts)).to(DEV), spans


def waves_of(lengths, seed=40):
    return [fr.golden_wave(n, seed + i) for i, n in enumerate(lengths)]


# ---- tts_frame_reflect -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [192, 384])
def test_frame_reflect_equals_numpy_reflection(hop):
    """Every length alone and all as one ragged batch with junk between the spans: the rows equal numpy.pad(mode="reflect") in whole
    rows of hop samples with a zero tail, byte for byte; the row layout is the cumulative one."""
    m, waves = measure(), waves_of(LENGTHS)
    want = [fr.row_buffer(x, hop) for x in waves]
    for x, w in zip(waves, want):
        packed, spans = pack([x], gap=3)
        rows, rag = m.frame(packed, spans, hop)
        assert rows.shape == w.shape and rag.lengths == [w.shape[0]] and rag.begins == [0]
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), w.view(np.uint32))
    packed, spans = pack(waves, gap=5)
    rows, rag = m.frame(packed, spans, hop)
    assert rag.lengths == [w.shape[0] for w in want] and rag.begins == list(np.cumsum([0] + [w.shape[0] for w in want[:-1]]))
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), np.concatenate(want).view(np.uint32))
    with pytest.raises(ValueError, match=f"needs more than {2 * hop}"):
        m.frame(packed, [(0, 2 * hop)], hop)


def test_frame_reflect_at_hop_256_is_the_front_ends_buffer_and_spectrum():
    """At the 16 kHz front end's resolution the rows are byte-equal to the buffer align.batched_spectra pads on the host, and with
    the existing conv behind them the spectrum is torch.equal to batched_spectra's."""
    m, waves = measure(), waves_of((513, 1024, 1025, 5000), seed=60)
    logmel = style.LogMel(DEV)
    packed, spans = pack(waves, gap=7)
    rows, rag = m.frame(packed, spans, style.HOP)
    host = np.concatenate([fr.row_buffer(x, style.HOP) for x in waves])  # np.pad(x, 512, "reflect") in whole rows: batched_spectra's xd
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), host.view(np.uint32))
    spec = m.ops.conv(logmel.dft, rows, m.ops.empty(rag.total_rows, 2 * logmel.bins), rag, compute=capi.COMPUTE_F32, split_k=False)
    want, frames = align.batched_spectra(m.ops, logmel, waves)
    assert frames.begins == rag.begins and frames.lengths == [1 + len(x) // style.HOP for x in waves]
    assert torch.equal(spec, want)


# ---- tts_spectral_distance, tts_spectral_reduce on given spectra --------------------------------------------------------------------
def tail_cases(bins):
    """[(re_a, im_a, re_b, im_b) float32 [F, bins]]: 1 frame, one frame more than a workgroup takes, a NaN pair, more than one sweep
    of the reduce, an all-zero pair (both sides at the clamp)."""
    rng = np.random.default_rng(1000 + bins)
    per_group, sweep = measure().frames_per_group, measure().reduce_sweep
    assert (per_group, sweep) == (4, 256)
    cases = []
    for F in (1, per_group + 1, per_group + 1, sweep + 45, per_group + 1):
        scale = np.exp(rng.normal(size=(1, bins))).astype(np.float32)  # a spectrum with a shape: three orders of magnitude
        cases.append(tuple((scale * rng.normal(size=(F, bins))).astype(np.float32) for _ in range(4)))
    cases[2][1][2, bins // 2] = np.nan
    cases[4] = tuple(np.zeros_like(c) for c in cases[4])
    return cases


def run_tail(cases, bins, which, with_mel, pad=2):
    """The pairs ``which`` of ``cases`` in ONE launch each of the two kernels, in a spectrum buffer full of NaN apart from their rows
    -> (frame sums [F, 4] per pair, totals [4] per pair) as numpy float64."""
    m = measure()
    ld, at, pairs = 2 * bins + pad, 1, []
    total = 1 + sum(2 * cases[i][0].shape[0] + 1 for i in which)
    spec = np.full((total, ld), np.nan, dtype=np.float32)
    for i in which:
        ra, ia, rb, ib = cases[i]
        F = ra.shape[0]
        spec[at: at + F, :bins], spec[at: at + F, bins: 2 * bins] = ra, ia
        spec[at + F: at + 2 * F, :bins], spec[at + F: at + 2 * F, bins: 2 * bins] = rb, ib
        pairs.append((at, at + F, F))
        at += 2 * F + 1
    frame_sums, totals = m.sums(torch.from_numpy(spec).to(DEV), bins, pairs, with_mel)
    fs, tt = frame_sums.cpu().numpy(), totals.cpu().numpy()
    return [fs[k, :p[2]].copy() for k, p in enumerate(pairs)], [tt[k].copy() for k in range(len(pairs))]


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), initial=0.0))


@pytest.mark.parametrize("bins", [385, 769, 1537])
def test_spectral_distance_and_reduce_against_float64(bins):
    """Per-frame sums and per-pair totals of given fp32 spectra against the float64 restatement of the tail, relative; the tolerance
    is 4 x the largest such error of the float32 numpy restatement of the same tail on the same cases.  A batch equals its pairs
    alone bit for bit, and the NaN pair in its middle is NaN itself and leaves its neighbours' bits alone."""
    cases, with_mel = tail_cases(bins), bins == 769
    mel = fr.mel_matrix() if with_mel else None
    finite = [0, 1, 3, 4]
    ref = [fr.frame_sums(c[:2], c[2:], mel) for c in cases]
    f32 = [fr.frame_sums(c[:2], c[2:], mel, np.float32) for c in cases]
    cols = slice(0 if with_mel else 1, 4)
    standin = max(max(rel_err(f32[i][:, cols], ref[i][:, cols]), rel_err(f32[i][:, cols].sum(axis=0, dtype=np.float32), ref[i][:, cols].sum(axis=0)))
                  for i in finite)
    tol = 4.0 * standin
    batch_frames, batch_totals = run_tail(cases, bins, range(len(cases)), with_mel)
    worst = 0.0
    for i in finite:
        worst = max(worst, rel_err(batch_frames[i][:, cols], ref[i][:, cols]), rel_err(batch_totals[i][cols], ref[i][:, cols].sum(axis=0)))
        if not with_mel:
            assert not batch_frames[i][:, 0].any() and batch_totals[i][0] == 0.0
    print(f"bins {bins}: float32 stand-in {standin:.3e}, tolerance {tol:.3e}, MI355X {worst:.3e}")
    assert 0.0 < standin < 1e-5
    assert worst <= tol
    # the all-zero pair: no difference, and the denominator is the clamp's, not zero
    assert not batch_totals[4][[0, 1, 3]].any() and batch_totals[4][2] > 0.0
    # the NaN pair: its frame 2 and its totals, nothing else
    # (the NaN is on the generated side: the recording's energy, column 2, stays finite)
    nan_cols = [0, 1, 3] if with_mel else [1, 3]
    assert np.isnan(batch_frames[2][2, nan_cols]).all() and np.isnan(batch_totals[2][nan_cols]).all()
    assert np.isfinite(batch_frames[2][2, 2]) and np.isfinite(batch_totals[2][2]) and np.isfinite(np.delete(batch_frames[2], 2, axis=0)).all()
    for i in range(len(cases)):
        alone_frames, alone_totals = run_tail(cases, bins, [i], with_mel, pad=0)
        assert np.array_equal(alone_frames[0].view(np.uint64), batch_frames[i].view(np.uint64)), i
        assert np.array_equal(alone_totals[0].view(np.uint64), batch_totals[i].view(np.uint64)), i


def test_spectral_reduce_adds_in_the_documented_order():
    """tts_spectral_reduce on given frame sums equals the numpy emulation of its documented order (strided per-thread sums, xor
    butterfly, four wavefronts left to right) bit for bit.  The values spread over 40 binary orders of magnitude, so another order
    shows: on the host, before the GPU is touched, every case of more than one wavefront differs from the plain sequential sum and
    from the 256-entry tree in at least one column (up to 64 frames the tree and the butterfly add the same pairs)."""
    frames = (1, 64, 65, 255, 256, 257, 1000)
    rng = np.random.default_rng(20261021)
    cases = [rng.normal(size=(F, 4)) * 2.0 ** rng.integers(-20, 21, size=(F, 4)) for F in frames]
    want = np.stack([butterfly_order_sum(c) for c in cases])
    for F, c, w in zip(frames, cases, want):
        if F >= 65:
            assert (sequential_order_sum(c).view(np.int64) != w.view(np.int64)).any(), F
            assert (tree_order_sum(c).view(np.int64) != w.view(np.int64)).any(), F
    m = measure()
    max_frames = max(frames)
    frame_sums = np.full((len(frames), max_frames, capi.FIDELITY_SUMS), np.nan)  # what lies past a pair's frames is not read
    for k, c in enumerate(cases):
        frame_sums[k, : len(c)] = c
    pairs = np.array([(0, 0, F) for F in frames], dtype=np.int64)  # the reduce reads the frame counts alone
    fs_d, pr_d = torch.from_numpy(frame_sums).to(DEV), torch.from_numpy(pairs).to(DEV)
    totals = torch.empty((len(frames), capi.FIDELITY_SUMS), dtype=torch.float64, device=DEV)
    capi.check(m.lib.tts_spectral_reduce(fs_d.data_ptr(), pr_d.data_ptr(), len(frames), max_frames, totals.data_ptr(), m.ops.stream()),
               "tts_spectral_reduce")
    torch.cuda.synchronize()
    got = totals.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


# ---- the whole measure -------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_reference_golden():
    """The seeded pairs of the golden through SpectralDistance.distance against the reference's stored losses.  The bound is 4 x the
    largest error, over these cases, of the CPU stand-in (numpy float32 DFT by matrix product + float32 tail) against the float64
    restatement: the matrix cores add the 1536 products of a bin in another order than numpy does."""
    g = np.load(GOLDEN)
    cases = fr.golden_cases()
    res = (fidelity.REFERENCE_RESOLUTION,)
    pairs = [fr.golden_pair(n, kind, seed) for n, kind, seed in cases]
    f64 = [fr.distance(a, b, res) for a, b in pairs]
    f32 = [fr.distance(a, b, res, f32=True) for a, b in pairs]
    standin = max(abs(s["mel_l1"] - d["mel_l1"]) for s, d in zip(f32, f64))
    bound = 4.0 * standin
    others = {k: 4.0 * max(abs(s[res[0]][k] - d[res[0]][k]) for s, d in zip(f32, f64)) for k in ("spectral_convergence", "log_magnitude_l1")}
    got = measure().distance([a for a, _ in pairs], [b for _, b in pairs], resolutions=res, keep_frames=True)
    err_ref = max(abs(r["mel_l1"] - float(v)) for r, v in zip(got, g["mel_loss"]))
    err_f64 = max(abs(r["mel_l1"] - d["mel_l1"]) for r, d in zip(got, f64))
    err_frames = max(float(np.abs(r["frame_mel_l1"].cpu().numpy() - d["frame_mel_l1"]).max()) for r, d in zip(got, f64))
    print(f"golden: stand-in {standin:.3e}, bound {bound:.3e}, MI355X against the reference {err_ref:.3e}, against float64 {err_f64:.3e}, "
          f"per frame against float64 {err_frames:.3e}; bounds of the other measures {others}")
    assert 0.0 < standin < 1e-6
    assert err_ref <= bound
    for r, (n, _, _), d in zip(got, cases, f64):
        assert r["frames"] == 1 + n // 384 and r["lengths"] == (n, n) and r["samples"] == n
        assert r["worst_frame"] == int(np.argmax(r["frame_mel_l1"].cpu().numpy())) and r["worst_frame_seconds"] == r["worst_frame"] * 384 / 24000
        for k, b in others.items():  # the other two measures against the float64 restatement, bounds derived the same way
            assert abs(r["resolutions"][res[0]][k] - d[res[0]][k]) <= b, (k, b)
    # the same pairs alone: the same bits
    for k in (0, 5):
        alone = measure().distance([pairs[k][0]], [pairs[k][1]], resolutions=res)[0]
        assert alone["mel_l1"] == got[k]["mel_l1"] and alone["resolutions"] == got[k]["resolutions"]


def test_known_answer_pair_through_the_public_distance():
    """generated = recording / 2 (exact in float32, and the fp32 DFT of the half is the half of the DFT): mel_l1 = log10 2 and
    log_magnitude_l1 = ln 2 at all three resolutions; the spectral convergence is 1/2 with the recording in the denominator and 1
    with the two swapped.  Unequal lengths are cut to the shorter and reported; a pair that is too short raises."""
    b = fr.golden_wave(5000, 77)
    a = (0.5 * b).astype(np.float32)
    m = measure()
    half, swapped = m.distance([torch.from_numpy(a).to(DEV), b], [b, a[:4900]])
    for rec, sc, lengths in ((half, 0.5, (5000, 5000)), (swapped, 1.0, (5000, 4900))):
        print({k: v for k, v in rec.items() if k != "resolutions"}, rec["resolutions"])
        assert rec["lengths"] == lengths and rec["samples"] == min(lengths) and rec["frames"] == 1 + min(lengths) // 384
        assert abs(rec["mel_l1"] - math.log10(2.0)) < 1e-12
        assert set(rec["resolutions"]) == set(fidelity.DEFAULT_RESOLUTIONS)
        for r in fidelity.DEFAULT_RESOLUTIONS:
            assert abs(rec["resolutions"][r]["spectral_convergence"] - sc) < 1e-12
            assert abs(rec["resolutions"][r]["log_magnitude_l1"] - math.log(2.0)) < 1e-12
    same = m.distance([b], [b], keep_frames=True)[0]
    assert same["mel_l1"] == 0.0 and not same["frame_mel_l1"].any() and same["worst_frame"] == 0
    assert all(v == {"spectral_convergence": 0.0, "log_magnitude_l1": 0.0} for v in same["resolutions"].values())
    only = m.distance([a], [b], resolutions=((768, 192),))[0]
    assert only["mel_l1"] is None and "worst_frame" not in only and list(only["resolutions"]) == [(768, 192)]
    # 32 kHz in: converted on the device, 3/4 of the samples
    up = m.distance([fr.golden_wave(8000, 5)], [fr.golden_wave(8000, 5)], sr_a=32000, resolutions=((1536, 384),))[0]
    assert up["lengths"] == (6000, 6000) and up["mel_l1"] == 0.0
    with pytest.raises(ValueError, match="needs more than 1536"):
        m.distance([a[:1536]], [b])
    with pytest.raises(ValueError, match="2 generated signals for 1 recordings"):
        m.distance([a, a], [b])


# ---- copy-synthesis -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocoder_checkpoints(tmp_path_factory):
    root = tmp_path_factory.mktemp("fidelity_models")
    paths = {}
    for kind, sub, sd in (("bigvgan", "BigVGAN", fw.bigvgan_state_dict()), ("hifigan", "Avocodo", fw.hifigan_state_dict())):
        os.makedirs(root / sub)
        paths[kind] = str(root / sub / "best.pt")
        torch.save({"generator": {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}}, paths[kind])
    return paths


def recordings():
    """Three seeded 16 kHz recordings of 7 to 12 vocoder frames (0.11 to 0.2 s)."""
    return [fw.reference_wave(u, n).astype(np.float32) for u, n in ((0, 256 * 7 + 40), (1, 256 * 12 + 3), (2, 256 * 9))]


@pytest.mark.parametrize("kind", ["bigvgan", "hifigan"])
def test_vocoder_scorer_is_the_hand_composed_chain(kind, vocoder_checkpoints, capsys):
    """VocoderScorer on the seeded fixture vocoders at bf16 (the scores say nothing about quality: plumbing and determinism only):
    its mel_l1 equals resample -> log-mel (the host-padded front end) -> vocode -> distance composed by hand, bit for bit; batch
    size 1 and 3 give the same bits; listing works on the result."""
    scorer = fidelity.VocoderScorer(vocoder_checkpoints[kind], DEV, faster_vocoder=kind == "hifigan", precision="bf16")
    waves = recordings()
    scorer.score(waves, sr=16000, batch_size=3)
    keys = [f"wave {i}" for i in range(3)]
    assert list(scorer.path_to_score) == keys and not scorer.nans
    batch3 = dict(scorer.path_to_score)
    records3 = dict(scorer.path_to_record)
    scorer.score(waves, sr=16000, batch_size=1)
    assert scorer.path_to_score == batch3
    for k in keys:
        assert scorer.path_to_record[k]["resolutions"] == records3[k]["resolutions"] and scorer.path_to_record[k]["worst_frame"] == records3[k]["worst_frame"]
    res, logmel, m = resample.Resampler(DEV), style.LogMel(DEV), measure()
    for k, w in zip(keys, waves):
        y24, _ = res.resample(torch.from_numpy(w).to(DEV), [(0, len(w))], 16000, 24000)
        F = y24.numel() // 384
        assert F == records3[k]["frames"] - 1 and records3[k]["samples"] == 384 * F  # (the 24 kHz STFT of 384 F samples has F + 1 frames)
        y16, _ = res.resample(y24, [(0, 384 * F)], 24000, 16000)
        assert y16.numel() == 256 * F
        mel = logmel.forward(y16.cpu().numpy())
        assert mel.shape == (F + 1, 80)
        wav, rag = scorer.vocoder.forward(mel[:F].contiguous(), Ragged([F], scorer.device))
        assert rag.lengths == [384 * F]
        by_hand = m.distance([wav[:384 * F]], [y24[:384 * F]])[0]
        print(kind, k, "mel_l1", by_hand["mel_l1"], by_hand["resolutions"])
        assert math.isfinite(by_hand["mel_l1"]) and by_hand["mel_l1"] > 0.0
        assert by_hand["mel_l1"] == batch3[k] and by_hand["resolutions"] == records3[k]["resolutions"]
    capsys.readouterr()
    scorer.show_samples_with_highest_loss(2)
    assert capsys.readouterr().out.count("Loss:") == 2
    scorer.remove_samples_with_highest_loss(1)
    assert len(scorer.current_dset) == 2 and max(batch3, key=batch3.get) not in scorer.current_dset.datapoints


def test_worst_frame_finds_a_burst():
    """A 20 ms burst added to the generated side: worst_frame is the frame centred on it."""
    rec = fw.reference_wave(5, 24000).astype(np.float32)
    gen = rec.copy()
    centre = 384 * 31 + 50
    gen[centre - 240: centre + 240] += 0.5 * fr.golden_wave(480, 9) / 0.1
    r = measure().distance([gen], [rec], keep_frames=True)[0]
    per_frame = r["frame_mel_l1"].cpu().numpy()
    print("burst at", centre / 24000, "s: worst frame", r["worst_frame"], "at", r["worst_frame_seconds"], "s, mel_l1 there", per_frame[r["worst_frame"]])
    assert abs(r["worst_frame"] * 384 - centre) <= 384 and r["worst_frame_seconds"] == r["worst_frame"] * 384 / 24000
    away = np.abs(np.arange(per_frame.size) * 384 - centre) > 768 + 240
    assert not per_frame[away].any() and per_frame[r["worst_frame"]] > 0.1


def test_interface_vocoder_fidelity_runs_its_own_vocoder_handle(tmp_path_factory):
    """ToucanTTSInterface.vocoder_fidelity at bf16 through the stage API's vocoder: the records are those of the chain composed by
    hand on the interface's own handle, bit for bit; tuples, waveforms with ``sr`` and ``keep_waves`` are taken."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path_factory.mktemp("fidelity_interface") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(interface, "MODELS_DIR", str(models))
        mp.setenv("TOUCAN_PRECISION", "bf16")
        mp.delenv("TOUCAN_PY_SEQUENCER", raising=False)
        tts = interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)
    waves = recordings()
    got = tts.vocoder_fidelity([(w, 16000) for w in waves], keep_waves=True)
    assert len(got) == 3
    again = tts.vocoder_fidelity(waves[1:2], sr=16000)[0]
    assert again["mel_l1"] == got[1]["mel_l1"] and again["resolutions"] == got[1]["resolutions"] and "generated" not in again
    with pytest.raises(ValueError, match="sample rate"):
        tts.vocoder_fidelity(waves[:1])
    chain = tts._fidelity_obj
    for w, rec in zip(waves, got):
        packed24, spans24, frames = chain.recordings_24k([w], 16000)
        mel, rag = chain.log_mel_16k(packed24, spans24, frames)
        wav, rag_w = tts.mel2wav.vocode(mel, rag)
        n = 384 * frames[0]
        by_hand = measure().distance([wav[rag_w.begins[0]: rag_w.begins[0] + n]], [packed24[:n]])[0]
        print("interface", rec["mel_l1"], rec["resolutions"])
        assert math.isfinite(rec["mel_l1"]) and rec["mel_l1"] > 0.0 and rec["samples"] == n and rec["frames"] == frames[0] + 1
        assert by_hand["mel_l1"] == rec["mel_l1"] and by_hand["resolutions"] == rec["resolutions"]
        assert rec["generated"].shape == rec["recording"].shape == (n,) and torch.equal(rec["recording"], packed24[:n])
