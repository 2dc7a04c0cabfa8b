"""STOI and ESTOI (csrc/intelligibility.hip, intelligibility.py) on the MI355X against the restatement of
tests/intelligibility_ref.py: the kept-frame lists exactly, the gathered rows bit for bit, the tail on given band values, the
whole measure, known answers through the public entry, a batch against its pairs alone bit for bit, the resampled entry and the
hook into the copy-synthesis scorer.

Tolerances are derived, not chosen.  The tail computes in fp64 like the restatement and differs from it in the order of its sums:
its bound is 4 x the largest difference, over the very cases, between the float64 and the numpy.longdouble restatement.  The whole
measure goes through an fp32 DFT: its bound is 4 x the largest error, over the very cases, of the float32 stand-in (float32 matrix
product, float32 tail) against float64.  The figures measured on the MI355X are recorded in DESIGN.md section 23."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import fidelity, fixture_weights as fw, intelligibility, resample
from tests import intelligibility_ref as ir

pytestmark = pytest.mark.gpu
DEV = "cuda"
JUNK = 0.97  # what lies between the spans of a packed wave: a read across a signal's edge picks it up
NAN_CASE, ZERO_CASE = 8, 7


@functools.lru_cache(maxsize=None)
def measure():
    return intelligibility.Intelligibility(DEV)


def pack(waves, gap=5):
    """The waves one after the other with ``gap`` samples of junk in front of each and behind the last -> (packed on the device,
    first samples)."""
    parts, begins, at = [], [], 0
    for i, x in enumerate(waves):
        parts.append(np.full(gap, JUNK if i % 2 else -JUNK, dtype=np.float32))
        at += gap
        begins.append(at)
        parts.append(np.asarray(x, dtype=np.float32))
        at += len(x)
    parts.append(np.full(gap, JUNK, dtype=np.float32))
    return torch.from_numpy(np.concatenate(parts)).to(DEV), begins


def pack_pairs(pairs, gap=5):
    """[(recording, generated)] -> (packed wave, int64 [P, 3] pair spans)."""
    packed, begins = pack([w for pr in pairs for w in pr], gap)
    return packed, np.asarray([(begins[2 * p], begins[2 * p + 1], min(len(x), len(y))) for p, (x, y) in enumerate(pairs)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    """[(recording, generated)] at 10 kHz: too short by one sample; 30 frames, one segment; two segments; one frame past a sweep of
    the select kernel; one segment past a workgroup's block of segments; a gap of 12 x 128 exact zeros; unequal lengths; an
    all-zero pair; one NaN sample on the generated side."""
    sweep, block = measure().select_sweep, measure().segments_per_group
    frames_of = lambda F: 256 + 128 * (F - 1)
    lengths = [3967, 3968, 4096, frames_of(sweep + 1), frames_of(block + 1 + 29), frames_of(70), 5000, 4096, 4096]
    out = []
    for i, n in enumerate(lengths):
        x = ir.speech_like(n, 200 + i)
        out.append([x, ir.at_snr(x, 5.0, 300 + i)])
    out[5][0] = ir.with_gap(out[5][0], 20, 12)
    out[6][1] = out[6][1][:4700]
    out[ZERO_CASE] = [np.zeros(4096, dtype=np.float32), np.zeros(4096, dtype=np.float32)]
    out[NAN_CASE][1][2000] = np.nan
    return tuple((x, y) for x, y in out)


@functools.lru_cache(maxsize=None)
def references():
    """The float64 restatement of every case, computed once: dicts of tests/intelligibility_ref.score."""
    with np.errstate(all="ignore"):
        return tuple(ir.score(x, y) for x, y in cases())


@functools.lru_cache(maxsize=None)
def end_to_end_bound():
    """(stand-in, bound): the largest error in STOI or ESTOI of the float32 stand-in against float64 over the cases with a finite
    answer, and 4 x that."""
    worst = 0.0
    for (x, y), ref in zip(cases(), references()):
        if math.isfinite(ref["stoi"]):
            s = ir.score(x, y, np.float32)
            worst = max(worst, abs(s["stoi"] - ref["stoi"]), abs(s["estoi"] - ref["estoi"]))
    return worst, 4.0 * worst


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- tts_stoi_frame_energy, tts_stoi_select ------------------------------------------------------------------------------------------
def test_kept_frames_equal_the_restatements():
    """Condition on the inputs, asserted: in float64 no frame energy of any case lies within 0.1 dB of its threshold (the generators
    give more than 26 dB).  Then the kept lists are the restatement's exactly, in a batch and alone."""
    m = measure()
    packed, pairs = pack_pairs(cases())
    for (x, _), (_, _, n) in zip(cases(), pairs):
        margin = ir.threshold_margin(x[:n])
        assert margin > 0.1, margin
    kept, counts, max_frames, _ = m.select(packed, pairs)
    kept, counts = kept.cpu().numpy(), counts.cpu().numpy()
    assert max_frames == m.select_sweep + 1
    want = [ir.kept_frames(x[:n]) for (x, _), (_, _, n) in zip(cases(), pairs)]
    assert [len(w) for w in want] == [29, 30, 31, m.select_sweep + 1, m.segments_per_group + 30, 59, 35, 31, 31]
    for p, w in enumerate(want):
        assert counts[p] == len(w) and np.array_equal(kept[p, :len(w)], w), p
    for p in (0, 3, 5):
        alone, pr = pack_pairs([cases()[p]], gap=3)
        k1, c1, _, _ = m.select(alone, pr)
        assert int(c1[0]) == len(want[p]) and np.array_equal(k1[0, :len(want[p])].cpu().numpy(), want[p])


# ---- tts_stoi_gather -----------------------------------------------------------------------------------------------------------------
def test_gathered_rows_equal_the_float32_restatement_bit_for_bit():
    """Rows 0 .. K - 1 of both sides are the compacted frames of the restatement in float32 with the header's operand order, the rows
    K .. F - 1 are zeros; junk between the spans is never read."""
    m = measure()
    packed, pairs = pack_pairs(cases())
    kept, counts, max_frames, pairs_d = m.select(packed, pairs)
    rows, row_begin = m.gather(packed, pairs, pairs_d, kept, counts, max_frames)
    rows = rows.cpu().numpy()
    assert rows.shape == (2 * sum(ir.n_frames(n) for n in pairs[:, 2]), 256)
    for p, ((x, y), (_, _, n)) in enumerate(zip(cases(), pairs)):
        F, k = ir.n_frames(n), ir.kept_frames(x[:n])
        for side, sig in enumerate((x, y)):
            with np.errstate(invalid="ignore"):
                want = ir.gathered_rows(sig[:n], k, np.float32)
            got = rows[row_begin[p, side]: row_begin[p, side] + F]
            ok = ~np.isnan(want)
            assert np.array_equal(got[:len(k)].view(np.uint32)[ok], want.view(np.uint32)[ok]), (p, side)
            assert np.isnan(got[:len(k)][~ok]).all() and (ok.all() or (p, side) == (NAN_CASE, 1))
            assert not got[len(k):].view(np.uint32).any(), (p, side)
    assert not rows[row_begin[5, 0] + 59: row_begin[5, 0] + 70].any()  # the gap pair: 11 rows past its 59 frames


# ---- tts_stoi_segments, tts_stoi_reduce on given band values -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_cases():
    """[(X, Y) float64 [M, 15]]: one segment; two; one segment past a workgroup's block; more segments than one sweep of the reduce;
    an all-zero pair; a pair with one NaN band value on the generated side; 29 frames (no segment)."""
    rng = np.random.default_rng(2300)
    block = measure().segments_per_group
    out = []
    for M in (30, 31, block + 30, 256 + 45 + 29, 40, 40, 29):
        shape = np.exp(rng.normal(size=(1, 15)))  # band levels over an order of magnitude
        env = 0.6 + 0.4 * np.sin(np.arange(M)[:, None] / 3.0 + rng.uniform(0, 6.0, size=(1, 15)))
        X = shape * env * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=(M, 15)))
        Y = X * (1.0 + 0.8 * rng.uniform(-1.0, 1.0, size=(M, 15))) + 0.1 * shape * rng.uniform(size=(M, 15))
        out.append((np.ascontiguousarray(X), np.ascontiguousarray(Y)))
    out[4] = (np.zeros((40, 15)), np.zeros((40, 15)))
    out[5][1][17, 6] = np.nan
    return tuple(out)


def run_tail(which):
    """The pairs ``which`` of tail_cases() in ONE launch of each of the two kernels, in a band buffer full of NaN apart from their
    rows (a row of slack behind every pair's rows, which the counts exclude) -> [(segment values [S, 2], totals [2])]."""
    m, tc = measure(), tail_cases()
    total = 1 + sum(2 * (tc[i][0].shape[0] + 1) for i in which)
    buf, at, row_begin, frames, counts = np.full((total, 15), np.nan), 1, [], [], []
    for i in which:
        X, Y = tc[i]
        M = X.shape[0]
        buf[at: at + M], buf[at + M + 1: at + 2 * M + 1] = X, Y
        row_begin.append((at, at + M + 1))
        frames.append(M + 1)
        counts.append(M)
        at += 2 * (M + 1)
    seg, tot = m.tail(torch.from_numpy(buf).to(DEV), row_begin, frames, torch.tensor(counts, dtype=torch.int32, device=DEV))
    seg, tot = seg.cpu().numpy(), tot.cpu().numpy()
    return [(seg[k, :max(0, c - 29)].copy(), tot[k].copy()) for k, c in enumerate(counts)]


def test_tail_on_given_band_values_against_float64():
    """Per-segment and per-pair STOI and ESTOI of given fp64 band values against the float64 restatement; the bound is 4 x the
    largest difference between the float64 and the long double restatement over these cases."""
    tc = tail_cases()
    finite = [0, 1, 2, 3, 4]
    with np.errstate(all="ignore"):
        f64 = [ir.tail(X, Y) for X, Y in tc]
        wide = [ir.tail(X, Y, np.longdouble) for X, Y in tc]
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    dist = lambda a, b: max(float(np.max(np.abs(np.asarray(a[q], dtype=np.longdouble) - b[q]), initial=0.0)) for q in range(4))
    standin = max(dist(f64[i], wide[i]) for i in finite)
    tol = 4.0 * standin
    got = run_tail(range(len(tc)))
    worst = 0.0
    for i in finite:
        seg, tot = got[i]
        assert seg.shape == (tc[i][0].shape[0] - 29, 2)
        worst = max(worst, float(np.abs(seg[:, 0] - f64[i][0]).max()), float(np.abs(seg[:, 1] - f64[i][1]).max()), abs(tot[0] - f64[i][2]),
                    abs(tot[1] - f64[i][3]))
    print(f"tail: float64 against long double {standin:.3e}, tolerance {tol:.3e}, MI355X against float64 {worst:.3e}")
    assert 0.0 < standin < 1e-14
    assert worst <= tol
    assert not got[4][0].any() and not got[4][1].any()  # silence: d = 0 through the eps divisors
    # the NaN band value: the segments that hold frame 17 (all 11 of them) and the totals
    assert np.isnan(got[5][0]).all() and np.isnan(got[5][1]).all() and np.isnan(f64[5][2])
    assert got[6][0].shape == (0, 2) and np.isnan(got[6][1]).all()
    for i in range(len(tc)):
        alone = run_tail([i])[0]
        assert np.array_equal(bits(alone[0]), bits(got[i][0])) and np.array_equal(bits(alone[1]), bits(got[i][1])), i


# ---- the whole measure -------------------------------------------------------------------------------------------------------------
def test_end_to_end_against_the_float64_restatement():
    """Every case through score_packed.  The bound is 4 x the largest error of the float32 stand-in over these cases; the stand-in
    itself is non-zero and below 1e-6 (first measured on the host: 8.0e-08)."""
    standin, bound = end_to_end_bound()
    packed, pairs = pack_pairs(cases())
    got = measure().score_packed(packed, pairs, keep_segments=True)
    worst = worst_seg = 0.0
    for p, (rec, ref) in enumerate(zip(got, references())):
        assert (rec["status"], rec["frames"], rec["kept_frames"], rec["segments"]) == (ref["status"], ref["frames"], ref["kept_frames"], ref["segments"]), p
        assert rec["lengths"] == (int(pairs[p, 2]),) * 2
        if math.isfinite(ref["stoi"]):
            worst = max(worst, abs(rec["stoi"] - ref["stoi"]), abs(rec["estoi"] - ref["estoi"]))
            worst_seg = max(worst_seg, float(np.abs(rec["segment_stoi"].cpu().numpy() - ref["segment_stoi"]).max()),
                            float(np.abs(rec["segment_estoi"].cpu().numpy() - ref["segment_estoi"]).max()))
            assert np.array_equal(rec["kept"].cpu().numpy(), ref["kept"])
    print(f"end to end: float32 stand-in {standin:.3e}, bound {bound:.3e}, MI355X against float64 {worst:.3e}, per segment {worst_seg:.3e}")
    assert 0.0 < standin < 1e-6
    assert worst <= bound
    assert got[0]["status"] == "too_short" and math.isnan(got[0]["stoi"]) and math.isnan(got[0]["estoi"]) and got[0]["worst_segment"] is None
    assert (got[1]["segments"], got[2]["segments"], got[4]["segments"]) == (1, 2, measure().segments_per_group + 1)
    assert (got[ZERO_CASE]["status"], got[ZERO_CASE]["kept_frames"], got[ZERO_CASE]["stoi"], got[ZERO_CASE]["estoi"]) == ("ok", 31, 0.0, 0.0)
    assert got[NAN_CASE]["status"] == "ok" and math.isnan(got[NAN_CASE]["stoi"]) and math.isnan(got[NAN_CASE]["estoi"])
    assert 0.3 < got[3]["estoi"] < got[3]["stoi"] < 0.99  # 5 dB SNR


def test_known_answers_through_the_public_score():
    """A signal against itself and against its half scores 1 within the end-to-end bound; the SNR ladder is strictly decreasing; a
    100 ms burst in one half of the generated signal puts the worst segment's start inside that half."""
    m, (_, bound) = measure(), end_to_end_bound()
    x = ir.speech_like(20000, 1)
    ladder = [ir.at_snr(x, snr, 50) for snr in (20, 10, 0, -10)]
    got = m.score([x] * 6, [torch.from_numpy(x).to(DEV), (0.5 * x).astype(np.float32)] + ladder, 10000)
    print([(r["stoi"], r["estoi"]) for r in got])
    for r in got[:2]:
        assert r["status"] == "ok" and (r["frames"], r["kept_frames"], r["segments"], r["lengths"]) == (155, 155, 126, (20000, 20000))
        assert abs(r["stoi"] - 1.0) <= bound and abs(r["estoi"] - 1.0) <= bound
    for hi, lo in zip(got[1:], got[2:]):
        assert lo["stoi"] < hi["stoi"] and lo["estoi"] < hi["estoi"]
    for half, start in ((0, 5000), (1, 14000)):
        y = x.copy()
        y[start: start + 1000] += ir.white(1000, 60 + half, 0.3)
        r = m.score([x], [y], 10000, keep_segments=True)[0]
        print("burst from", start / 10000, "s: worst segment", r["worst_segment"], "from", r["worst_segment_seconds"], "s")
        assert r["worst_segment"] == int(np.argmin(r["segment_estoi"].cpu().numpy())) and r["segment_stoi"].shape == (126,)
        assert half <= r["worst_segment_seconds"] < half + 1.0
        assert r["worst_segment_seconds"] == int(r["kept"][r["worst_segment"]]) * 128 / 10000
    # the worst segment is told in the signal's own time: 12 dropped frames in front of it move its index, not its start
    g = ir.with_gap(x, 8, 13)
    y = g.copy()
    y[14000: 15000] += ir.white(1000, 61, 0.3)
    r = m.score([g], [y], 10000, keep_segments=True)[0]
    assert r["kept_frames"] == 143 and 1.0 <= r["worst_segment_seconds"] < 2.0
    assert r["worst_segment_seconds"] == (r["worst_segment"] + 12) * 128 / 10000
    with pytest.raises(ValueError, match="2 recordings for 1 generated"):
        m.score([x, x], [x], 10000)
    assert m.score([], [], 10000) == []


def test_a_batch_equals_its_pairs_alone_bit_for_bit():
    """Every pair scored alone returns the bits it has in the batch (uint64 views of the measures and of every segment value); the
    NaN pair is NaN, the pairs that are too short are NaN, and none of them disturbs a neighbour."""
    m = measure()
    packed, pairs = pack_pairs(cases())
    batch = m.score_packed(packed, pairs, keep_segments=True)
    batch_seg = [(r["segment_stoi"].cpu().numpy(), r["segment_estoi"].cpu().numpy()) for r in batch]
    for p, pr in enumerate(cases()):
        alone_packed, alone_pairs = pack_pairs([pr], gap=2)
        alone = m.score_packed(alone_packed, alone_pairs, keep_segments=True)[0]
        assert {k: alone[k] for k in ("status", "frames", "kept_frames", "segments")} == {k: batch[p][k] for k in ("status", "frames", "kept_frames", "segments")}
        if p in (0, NAN_CASE):
            assert math.isnan(alone["stoi"]) and math.isnan(batch[p]["stoi"]) and math.isnan(alone["estoi"]) and math.isnan(batch[p]["estoi"])
        else:
            assert np.array_equal(bits([alone["stoi"], alone["estoi"]]), bits([batch[p]["stoi"], batch[p]["estoi"]])), p
            assert np.array_equal(bits(alone["segment_stoi"].cpu().numpy()), bits(batch_seg[p][0])), p
            assert np.array_equal(bits(alone["segment_estoi"].cpu().numpy()), bits(batch_seg[p][1])), p
    # the same batch without its NaN pair and its short pair: the others keep their bits
    rest = [p for p in range(len(cases())) if p not in (0, NAN_CASE)]
    sub_packed, sub_pairs = pack_pairs([cases()[p] for p in rest], gap=9)
    for p, r in zip(rest, m.score_packed(sub_packed, sub_pairs)):
        assert np.array_equal(bits([r["stoi"], r["estoi"]]), bits([batch[p]["stoi"], batch[p]["estoi"]])), p


def test_the_resampled_entry_is_score_packed_on_the_resamplers_output():
    """A 24 kHz pair and a 16 kHz pair through ``score`` equal score_packed on what Resampler.resample(..., 10000) returns, bit for
    bit; lengths follow resample.out_length."""
    m = measure()
    res = resample.Resampler(DEV)
    for sr, n, m_gen in ((24000, 24000, 23000), (16000, 12001, 12001)):
        x = fw.reference_wave(3, n).astype(np.float32) * 0.5
        y = (x + ir.white(n, 70, 0.02))[:m_gen].astype(np.float32)
        got = m.score([x], [y], sr)[0]
        nx, ny = resample.out_length(n, sr, 10000), resample.out_length(m_gen, sr, 10000)
        assert got["lengths"] == (nx, ny) and got["frames"] == ir.n_frames(min(nx, ny)) and got["status"] == "ok"
        x10, sx = res.resample(torch.from_numpy(x).to(DEV), [(0, n)], sr, 10000)
        y10, sy = res.resample(torch.from_numpy(y).to(DEV), [(0, m_gen)], sr, 10000)
        assert sx == [(0, nx)] and sy == [(0, ny)]
        by_hand = m.score_packed(torch.cat([x10, y10]), [(0, nx, min(nx, ny))])[0]
        print(sr, got["stoi"], got["estoi"])
        assert np.array_equal(bits([got["stoi"], got["estoi"]]), bits([by_hand["stoi"], by_hand["estoi"]])) and math.isfinite(got["estoi"])
    # the two sides at different rates
    x24 = fw.reference_wave(4, 24000).astype(np.float32) * 0.5
    x16, _ = res.resample(torch.from_numpy(x24).to(DEV), [(0, 24000)], 24000, 16000)
    r = m.score([x24], [x16], 24000, sr_b=16000)[0]
    assert r["lengths"] == (10000, 10000) and r["status"] == "ok" and r["estoi"] > 0.9


# ---- the hook into the copy-synthesis scorer --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocoder_checkpoint(tmp_path_factory):
    root = tmp_path_factory.mktemp("intelligibility_models")
    os.makedirs(root / "Avocodo")
    path = str(root / "Avocodo" / "best.pt")
    torch.save({"generator": {k: torch.from_numpy(np.array(v)) for k, v in fw.hifigan_state_dict().items()}}, path)
    return path


def recordings():
    """Two seeded 16 kHz recordings of 50 and 56 vocoder frames (0.8 and 0.9 s: 61 and 68 frames at 10 kHz)."""
    return [fw.reference_wave(u, n).astype(np.float32) for u, n in ((0, 256 * 50 + 40), (1, 256 * 56))]


def test_vocoder_scorer_hook_is_the_hand_composed_chain(vocoder_checkpoint, capsys):
    """VocoderScorer on the seeded fixture vocoder at bf16 (plumbing and determinism only): with the keyword the records gain
    exactly ``stoi``, ``estoi`` and ``intelligibility_status``, equal bit for bit to Intelligibility.score on the two 24 kHz signals
    the distances saw; without it the records keep their keys and their bits."""
    scorer = fidelity.VocoderScorer(vocoder_checkpoint, DEV, faster_vocoder=True, precision="bf16")
    waves = recordings()
    plain = scorer.score_waves(waves, 16000, batch_size=2)
    with_it = scorer.score_waves(waves, 16000, batch_size=2, intelligibility=True)
    one_by_one = scorer.score_waves(waves, 16000, batch_size=1, intelligibility=True)
    new = {"stoi", "estoi", "intelligibility_status"}
    for a, b, c in zip(plain, with_it, one_by_one):
        assert set(a) == {"samples", "lengths", "mel_l1", "resolutions", "frames", "worst_frame", "worst_frame_seconds"}
        assert set(b) == set(a) | new and {k: b[k] for k in a} == a
        assert np.array_equal(bits([b["stoi"], b["estoi"]]), bits([c["stoi"], c["estoi"]]))
    chain, m = scorer.chain, measure()
    for w, rec in zip(waves, with_it):
        packed24, spans24, frames = chain.recordings_24k([w], 16000)
        mel, rag = chain.log_mel_16k(packed24, spans24, frames)
        wav, rag_w = scorer.vocoder.forward(mel, rag)
        n = 384 * frames[0]
        by_hand = m.score([packed24[:n]], [wav[rag_w.begins[0]: rag_w.begins[0] + n]], 24000)[0]
        print("hook", rec["stoi"], rec["estoi"], rec["intelligibility_status"], by_hand["frames"], by_hand["kept_frames"])
        assert rec["intelligibility_status"] == by_hand["status"] == "ok" and math.isfinite(rec["stoi"]) and math.isfinite(rec["estoi"])
        assert np.array_equal(bits([rec["stoi"], rec["estoi"]]), bits([by_hand["stoi"], by_hand["estoi"]]))
    scorer.score(waves, sr=16000, batch_size=2, rank_by="estoi")
    assert [scorer.path_to_score[f"wave {i}"] for i in range(2)] == [1.0 - r["estoi"] for r in with_it]
    with pytest.raises(ValueError, match="rank_by"):
        scorer.score(waves, sr=16000, rank_by="stoi")
    capsys.readouterr()


def test_interface_vocoder_fidelity_takes_the_keyword(tmp_path_factory):
    """ToucanTTSInterface.vocoder_fidelity(..., intelligibility=True) returns the three new fields, those of the chain on the
    interface's own vocoder handle; without the keyword the records do not hold them."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path_factory.mktemp("intelligibility_interface") / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(interface, "MODELS_DIR", str(models))
        mp.setenv("TOUCAN_PRECISION", "bf16")
        mp.delenv("TOUCAN_PY_SEQUENCER", raising=False)
        tts = interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)
    waves = recordings()
    got = tts.vocoder_fidelity([(w, 16000) for w in waves], intelligibility=True, keep_waves=True)
    plain = tts.vocoder_fidelity(waves, sr=16000)
    for rec, old in zip(got, plain):
        assert not {"stoi", "estoi", "intelligibility_status"} & set(old) and old["mel_l1"] == rec["mel_l1"] and old["resolutions"] == rec["resolutions"]
        by_hand = measure().score([rec["recording"]], [rec["generated"]], 24000)[0]
        print("interface", rec["stoi"], rec["estoi"], rec["intelligibility_status"])
        assert rec["intelligibility_status"] == "ok" and math.isfinite(rec["stoi"]) and math.isfinite(rec["estoi"])
        assert np.array_equal(bits([rec["stoi"], rec["estoi"]]), bits([by_hand["stoi"], by_hand["estoi"]]))
