"""The recording-free pronunciation check without a GPU: the float64 restatement (tests/pronunciation_ref.py) on cases worked by
hand and against identities and a brute-force enumeration, that the seeds of the GPU beam test keep their gap, the host half of
pronunciation.py (the reference tokens and their map back, ``id_to_phone``, ``summarise``, every refusal), and that the header, the
binding and the library declare the same entries."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, build, capi, pronunciation as pron
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from tests import pronunciation_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))


def table(probabilities):
    """Rows of probabilities -> fp32 logits whose softmax they are (to fp32 rounding)."""
    return np.log(np.asarray(probabilities, dtype=np.float64)).astype(np.float32)


# ---- cases worked by hand -------------------------------------------------------------------------------------------------------
def test_kitten_sitting():
    """k i t t e n / s i t t i n g: D = 3.  Walking back from (6, 7): the diagonal costs D(5, 6) + 1 = 4, the deletion D(5, 7) + 1 = 5,
    the insertion D(6, 6) + 1 = 3 - the only strict improvement, so g is inserted; from (6, 6) the diagonal is never beaten strictly:
    n = n, e / i, t = t, t = t, i = i, k / s.  4 hits, 2 substitutions, no deletion, 1 insertion."""
    counts, r2h, h2r = pr.levenshtein("kitten", "sitting")
    assert counts == (4, 2, 0, 1)
    assert r2h == [0, 1, 2, 3, 4, 5] and h2r == [0, 1, 2, 3, 4, 5, -1]
    assert pr.distance_two_rows("kitten", "sitting") == 3
    # the tie order: "ab" / "ba" costs 2 by two substitutions (diagonal first), not by a deletion and an insertion
    assert pr.levenshtein("ab", "ba") == ((0, 2, 0, 0), [0, 1], [0, 1])
    assert pr.levenshtein("", "ab") == ((0, 0, 0, 2), [], [-1, -1]) and pr.levenshtein("ab", "") == ((0, 0, 2, 0), [-1, -1], [])
    # a deletion where the diagonal is strictly worse: "abc" / "ac"
    assert pr.levenshtein("abc", "ac") == ((2, 0, 1, 0), [0, -1, 1], [0, 2])


BEST = [(1, 0.6), (1, 0.8), (4, 0.9), (1, 0.7), (2, 0.5), (2, 0.5), (0, 0.6), (4, 0.6)]  # per frame (its best symbol, its probability)


def five_symbol_table():
    rows = []
    for sym, p in BEST:
        row = [(1.0 - p) / 4] * 5
        row[sym] = p
        rows.append(row)
    return table(rows)


def test_greedy_decode_of_a_five_symbol_table():
    """Symbols 0 .. 3 and the blank 4; the frames' best symbols are 1 1 _ 1 2 2 0 _: four runs, the blank separating the two 1s;
    the confidences are the means of ln p of the best symbol."""
    x = five_symbol_table()
    got = pr.best_path(x, blank=4)
    assert got["ids"] == [1, 1, 2, 0] and got["first"] == [0, 3, 4, 6] and got["last"] == [1, 3, 5, 6]
    want = [(math.log(0.6) + math.log(0.8)) / 2, math.log(0.7), math.log(0.5), math.log(0.6)]
    assert all(c.dtype == np.float32 for c in got["conf"])
    assert np.allclose(got["conf"], want, rtol=0, atol=1e-6)  # (the table is exact to fp32 rounding of the logits only)
    # symbol 0 dropped: its frame counts as blank
    drop = np.array([1, 0, 0, 0, 0], dtype=np.uint8)
    assert pr.best_path(x, blank=4, drop=drop)["ids"] == [1, 1, 2]
    # symbol 2 dropped between the 1 of frame 3 and nothing else: still a run of its own before it
    assert pr.best_path(x, blank=4, drop=np.array([0, 0, 1, 0, 0], dtype=np.uint8))["ids"] == [1, 1, 0]
    # an exact tie goes to the lower index
    tie = np.zeros((1, 5), dtype=np.float32)
    assert pr.best_path(tie, blank=4)["ids"] == [0] and pr.best_path(tie, blank=0)["ids"] == []
    bad = x.copy()
    bad[3, 2] = np.nan
    assert pr.best_path(bad, blank=4) is None and pr.beam_search(bad, 4, 2) is None


def test_beam_search_and_greedy_disagree_on_three_frames():
    """Symbols a, b and the blank with p = 0.45, 0.05, 0.5 at each of three frames.  The best path is blank blank blank: the empty
    prefix, 0.5^3 = 0.125.  The prefix "a" collects a--, -a-, --a, aa-, -aa and aaa: 3 * 0.45 * 0.25 + 2 * 0.45^2 * 0.5 + 0.45^3 =
    0.631125 (a-a is "aa")."""
    x = table([[0.45, 0.05, 0.5]] * 3)
    assert pr.best_path(x, blank=2)["ids"] == []
    for beam in (2, 8):
        ids, score = pr.beam_search(x, 2, beam)
        assert ids == [0] and abs(score - math.log(0.631125)) < 1e-6
    ids, score = pr.enumerate_best_prefix(x, 2)
    assert ids == [0] and abs(score - math.log(0.631125)) < 1e-6
    # a beam of one keeps only the empty prefix's stay at frame 0 ... and still finds "a" later, but with less of its mass
    ids1, score1 = pr.beam_search(x, 2, 1)
    assert score1 < score


# ---- identities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_levenshtein_identities(seed):
    rng = np.random.default_rng(seed)
    R, H = int(rng.integers(0, 40)), int(rng.integers(0, 40))
    ref, hyp = [int(v) for v in rng.integers(0, 4, R)], [int(v) for v in rng.integers(0, 4, H)]
    (hits, subs, dels, ins), r2h, h2r = pr.levenshtein(ref, hyp)
    assert hits + subs + dels == R and hits + subs + ins == H
    assert subs + dels + ins == pr.distance_two_rows(ref, hyp)
    assert sum(j < 0 for j in r2h) == dels and sum(i < 0 for i in h2r) == ins
    matched = [(i, j) for i, j in enumerate(r2h) if j >= 0]
    assert all(h2r[j] == i for i, j in matched) and [j for _, j in matched] == sorted(j for _, j in matched)
    assert sum(ref[i] == hyp[j] for i, j in matched) == hits


@pytest.mark.parametrize("seed,T,S", [(s, 3, 3) for s in range(4)] + [(s, 4, 3) for s in range(4)] + [(s, 3, 4) for s in range(3)])
def test_a_beam_that_holds_every_prefix_finds_the_most_probable_one(seed, T, S):
    """With beam >= S^T nothing is ever pruned: the search returns the prefix with the largest probability summed over all its
    alignments, found by enumerating every alignment."""
    x = np.random.default_rng(100 + seed).normal(0.0, 1.0, size=(T, S)).astype(np.float32)
    ids, score = pr.beam_search(x, S - 1, S ** T)
    want_ids, want = pr.enumerate_best_prefix(x, S - 1)
    assert ids == want_ids and abs(score - want) < 1e-12


def test_logaddexp_and_log_softmax():
    assert pr.logaddexp(pr.NINF, -3.0) == -3.0 and pr.logaddexp(-3.0, pr.NINF) == -3.0 and pr.logaddexp(pr.NINF, pr.NINF) == pr.NINF
    assert abs(pr.logaddexp(math.log(0.25), math.log(0.5)) - math.log(0.75)) < 1e-15
    lp = pr.log_softmax(np.array([[1000.0, 1000.0, -1000.0]], dtype=np.float32))
    assert abs(lp[0, 0] - math.log(0.5)) < 1e-15 and lp[0, 2] < -1999


def test_posterior_scores_by_hand():
    """Two frames of (0.7, 0.2, 0.1) and one of (0.1, 0.8, 0.1); the text is symbol 0 on two frames, a word boundary, symbol 2 on one
    frame and symbol 1 on none."""
    x = table([[0.7, 0.2, 0.1], [0.7, 0.2, 0.1], [0.1, 0.8, 0.1]])
    out = pr.phone_posteriors(x, [2, 0, 1, 0], [0, -1, 2, 1])
    assert out.dtype == np.float32 and out.shape == (4, 4) and list(out[:, 3]) == [2, 0, 1, 0]
    assert np.allclose(out[0, :3], [math.log(0.7), 0.0, 1.0], atol=1e-6)
    assert np.isnan(out[1, :3]).all() and np.isnan(out[3, :3]).all()
    assert np.allclose(out[2, :3], [math.log(0.1), math.log(0.1) - math.log(0.8), 0.0], atol=1e-6)
    assert (out[[0, 2], 1] <= 0).all()
    assert np.isnan(pr.phone_posteriors(x, [2, 0, 2, 0], [0, -1, 2, 1])).all()  # does not add up
    assert np.isnan(pr.phone_posteriors(x, [-1, -1, -1, -1], [0, -1, 2, 1])).all()  # MAS could not run


@pytest.mark.parametrize("case", [c for c in pr.BEAM_CASES if c[1] * c[2] * c[3] <= 33 * 145 * 32])
def test_the_beam_seeds_keep_their_gap(case):
    """The GPU test asks for the restatement's prefix exactly: at no frame may the selection decide by less than MIN_GAP.  (The
    largest cases are checked where they are used.)  The merge case meets a live beam at most frames."""
    assert pr.BEAM_SEEDS[case] == 0
    seed, x, (ids, score), gap = pr.beam_case(*case)
    print(f"{case}: seed {seed}, smallest gap {gap:.3e}, {len(ids)} symbols, score {score:.6f}")
    assert gap > pr.MIN_GAP and x.shape == (case[1], case[2] + 3) and x.dtype == np.float32
    if case[0] == "merge" and case[3] >= 2:
        met = []
        pr.beam_search(x[:, :case[2]], case[2] - 1, case[3], merges=met)
        assert sum(m > 0 for m in met) > len(met) // 2


@pytest.mark.parametrize("case", pr.REMADE_CASES)
def test_the_remade_cases_prune_a_prefix_and_make_it_again(case):
    """Each of these tables joins, at some frame, an extend candidate into a live beam whose parent prefix had left the beams and
    come back - what a search that knows prefixes by node numbers alone gets wrong - and keeps MIN_GAP.  The first one by hand of
    the restatement: prefix 1 0 1 0 1 with log-probability -3.30840."""
    x, (ids, score), gap, frames = pr.remade_case(*case)
    print(f"{case}: smallest gap {gap:.3e}, {frames} frames with a remade parent, {ids}, score {score:.6f}")
    assert frames >= 1 and gap > pr.MIN_GAP and x.shape == (case[1], case[2] + 3)
    if case == (1983, 8, 3, 2):
        assert ids == [1, 0, 1, 0, 1] and abs(score + 3.30840) < 1e-5
    if case[2] ** case[1] <= 3 ** 8:  # the whole search never beats the best prefix's full probability
        assert score <= pr.enumerate_best_prefix(x[:, :case[2]], case[2] - 1)[1] + 1e-12


# ---- the host half ------------------------------------------------------------------------------------------------------------------
PHONES = "~həlˈoʊ wˈɜːld~#"


def test_reference_tokens_and_the_map_back():
    feats = phones_to_features(PHONES, handle_missing=False)
    ids, flags, full_ids, ref, ref_tokens = pron.reference_tokens(feats)
    want_ids, want_flags = align.token_ids(feats)
    assert np.array_equal(ids, want_ids) and np.array_equal(flags, want_flags)
    assert len(full_ids) == len(feats) and (full_ids[(flags & 1) == 1] == -1).all() and np.array_equal(full_ids[full_ids >= 0], ids)
    assert np.array_equal(ref, ids) and np.array_equal(full_ids[ref_tokens], ref) and (flags & 1).sum() >= 1
    silence = int(ids[0])  # "~"
    _, _, full2, ref2, tokens2 = pron.reference_tokens(feats, ignore_ids=[silence])
    assert np.array_equal(full2, full_ids) and silence not in ref2 and len(ref2) == len(ids) - (ids == silence).sum()
    assert np.array_equal(full_ids[tokens2], ref2) and set(tokens2) == {k for k, i in enumerate(full_ids) if i >= 0 and i != silence}
    mask = pron.drop_mask([silence])
    assert mask.dtype == np.uint8 and mask.shape == (pron.N_SYMBOLS,) and mask.sum() == 1 and mask[silence] == 1
    assert pron.drop_mask(()) is None


def test_id_to_phone_inverts_phone_ids():
    ids, names = align.phone_ids(), pron.id_to_phone()
    assert set(names) == {int(v) for v in ids.values()}
    for i, sym in names.items():
        assert ids[sym] == i and sym == min(s for s in ids if ids[s] == i)


def test_summarise():
    post = np.array([[-1.0, -0.5, 0.5, 3], [np.nan, np.nan, np.nan, 0], [-3.0, -2.5, 0.0, 2], [-0.2, 0.0, 1.0, 4]], dtype=np.float32)
    r = pron.summarise((9, 1, 2, 3), 12, post)
    assert r["per"] == 6 / 12 and (r["hits"], r["substitutions"], r["deletions"], r["insertions"], r["n_ref"]) == (9, 1, 2, 3, 12)
    assert r["gop_argmin"] == 2 and r["gop_min"] == -2.5 and r["gop_mean"] == pytest.approx(-1.0)
    assert pron.summarise((0, 0, 0, 2), 0, post)["per"] == 2.0
    failed = pron.summarise((-1, -1, -1, -1), 5, post[1:2])
    assert math.isnan(failed["per"]) and math.isnan(failed["gop_mean"]) and math.isnan(failed["gop_min"]) and failed["gop_argmin"] == -1
    assert pron.bp_bytes(128, 640) == 4 * 128 * 40 and pron.bp_bytes(10, 10 ** 6) == 4 * 10 * 256 and pron.bp_bytes(0, 5) == 0


def test_every_refusal():
    """Everything ``check`` refuses, it refuses before the device is touched (the extractor here is a stand-in without one)."""
    chk = pron.PronunciationChecker(extractor=types.SimpleNamespace(aligner=None, ops=None, device="cpu"))
    feats = phones_to_features(PHONES, handle_missing=False)
    w = np.sin(np.arange(4000) * 0.05).astype(np.float32)
    with pytest.raises(ValueError, match="2 texts for 1 waves"):
        chk.check([PHONES, PHONES], [w], 16000)
    for beam in (-1, 33, 2.5, True, None):
        with pytest.raises(ValueError, match="beam is an integer from 0"):
            chk.check([PHONES], [w], 16000, beam=beam)
        with pytest.raises(ValueError, match="beam is an integer from 0"):
            chk.recognise([w], 16000, beam=beam)
    with pytest.raises(ValueError, match="the blank"):
        chk.check([PHONES], [w], 16000, ignore_ids=[pron.BLANK])
    with pytest.raises(ValueError, match="none of the 145 symbols"):
        chk.check([PHONES], [w], 16000, ignore_ids=[145])
    bad = w.copy()
    bad[17] = np.inf
    with pytest.raises(ValueError, match="utterance 1: the wave holds a sample that is not finite"):
        chk.check([PHONES, PHONES], [w, bad], 16000)
    with pytest.raises(ValueError, match="utterance 0: 512 samples at 16 kHz are too short"):
        chk.check([PHONES], [w[:512]], 16000)
    with pytest.raises(ValueError, match=r"utterance 0: \d+ samples at 16 kHz are too short"):
        chk.check([PHONES], [w[:512]], 24000)
    long = np.repeat(feats[1:2], pron.MAX_REF + 1, axis=0)
    with pytest.raises(ValueError, match=f"utterance 1: {pron.MAX_REF + 1} aligner tokens"):
        chk.check([PHONES, long], [w, w], 16000)
    boundary = feats[np.asarray(feats)[:, align.IDX["word_boundary"]] != 0][:1]
    with pytest.raises(ValueError, match="utterance 0: its text holds no phoneme"):
        chk.check([boundary], [w], 16000)
    with pytest.raises(ValueError, match="2 sample rates for 1 waves"):
        chk.check([PHONES], [w], [16000, 16000])
    with pytest.raises(ValueError):
        pron.PronunciationChecker()
    assert chk.check([], [], 16000) == [] and chk.recognise([], 16000) == []


def test_a_cpu_device_is_refused():
    from ims_toucan_prosody_variance_amd import fixture_weights as fw
    build.build()
    with pytest.raises(capi.ToucanHipError):
        pron.PronunciationChecker(fw.aligner_state_dict(), "cpu")


def test_interface_refusals(tmp_path, monkeypatch):
    """``check_pronunciation`` refuses the keywords ``evaluate_against_recordings`` refuses, before anything runs."""
    from ims_toucan_prosody_variance_amd.interface import ToucanTTSInterface
    tts = ToucanTTSInterface.__new__(ToucanTTSInterface)  # the refusals come before any attribute is read
    for kw, words in ((dict(distributed=True), "not available with distributed=True"), (dict(sample_rate=16000), "sample_rate / pcm16 do not apply"),
                      (dict(pcm16=True), "sample_rate / pcm16 do not apply"), (dict(loudness=-23.0), "loudness does not apply"),
                      (dict(speech_level=-26.0), "speech_level does not apply")):
        with pytest.raises(ValueError, match=words):
            ToucanTTSInterface.check_pronunciation(tts, [PHONES], **kw)
    with pytest.raises(ValueError, match="beam is an integer from 0"):
        ToucanTTSInterface.check_pronunciation(tts, [PHONES], beam=33)
    with pytest.raises(ValueError, match="the blank"):
        ToucanTTSInterface.check_pronunciation(tts, [PHONES], ignore_ids=[144])


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_pronunciation_header_binding_and_library_agree():
    """include/toucan_pronunciation.h, capi.PRONUNCIATION_PROTOTYPES and the symbols libtoucan_hip.so exports are the same set,
    disjoint from every other table, with the argument counts, the constants and the struct the binding mirrors."""
    root = os.path.dirname(HERE)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "toucan_pronunciation.h"), encoding="utf-8").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tts_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.PRONUNCIATION_PROTOTYPES) == ["tts_ctc_beam_search", "tts_ctc_best_path", "tts_edit_distance", "tts_phone_posteriors"]
    tables = [getattr(capi, n) for n in dir(capi) if n.endswith("PROTOTYPES") and n != "PRONUNCIATION_PROTOTYPES"]
    assert len(tables) >= 12 and not any(set(declared) & set(t) for t in tables)
    macros = {k: int(v) for k, v in re.findall(r"#define\s+(TTS_[A-Z0-9_]+)\s+(\d+)", text)}
    assert macros == {"TTS_PRON_MAX_SYMBOLS": capi.PRON_MAX_SYMBOLS, "TTS_BEAM_MAX": capi.BEAM_MAX, "TTS_CTC_SCAN_BLOCK": capi.CTC_SCAN_BLOCK,
                      "TTS_EDIT_MAX_REF": capi.EDIT_MAX_REF, "TTS_EDIT_MAX_HYP": capi.EDIT_MAX_HYP, "TTS_EDIT_LDS_BP_BYTES": capi.EDIT_LDS_BP_BYTES,
                      "TTS_PHONE_COLUMNS": capi.PHONE_COLUMNS}
    assert capi.BEAM_MAX == 32 and capi.EDIT_MAX_HYP == 4096 and capi.EDIT_MAX_REF == capi.CTC_MAX_TARGETS and capi.PRON_MAX_SYMBOLS >= align.N_SYMBOLS
    assert len(pron.PHONE_COLUMNS) == capi.PHONE_COLUMNS
    names = re.findall(r"\bint\s+(tts_[a-z0-9_]+)\s*\(", text)
    assert sorted(names) == declared
    for arg_list, name in zip(re.findall(r"\bint\s+tts_[a-z0-9_]+\s*\((.*?)\)\s*;", text, flags=re.S), names):
        assert len(arg_list.split(",")) == len(capi.PRONUNCIATION_PROTOTYPES[name][1]), name
    fields = re.search(r"typedef struct TtsPronUtt \{(.*?)\}", text, flags=re.S).group(1)
    assert [f.strip() for decl in fields.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")] == \
        [n for n, _ in capi.TtsPronUtt._fields_]
    assert ctypes.sizeof(capi.TtsPronUtt) == 24
    assert "pronunciation.hip" in build.SOURCES
    build.build()
    handle = capi.lib()
    assert isinstance(handle, ctypes.CDLL)
    for n in declared:
        assert hasattr(handle, n) and getattr(handle, n).argtypes == capi.PRONUNCIATION_PROTOTYPES[n][1], n
    assert handle.tts_abi_version() == capi.ABI_VERSION
    # the host refuses before any launch, with a text that names the utterance
    utts = (capi.TtsPronUtt * 2)(capi.TtsPronUtt(0, 4, 0, 0, 0), capi.TtsPronUtt(4, 9, 0, 0, 0))
    rc = handle.tts_ctc_beam_search(1, 8, 5, 5, 4, None, utts, 1, 2, 4, 1, 1 << 20, 1, 1, 1, None)
    assert rc != 0 and b"utterance 1" in handle.tts_last_error()
    assert handle.tts_ctc_beam_search(1, 16, 5, 5, 4, None, utts, 1, 2, 33, 1, 1 << 20, 1, 1, 1, None) != 0 and b"beam of 33" in handle.tts_last_error()
    assert handle.tts_ctc_best_path(1, 16, 5, 5, 5, None, utts, 1, 2, 1, 1, 1, 1, 1, None) != 0 and b"blank 5" in handle.tts_last_error()
    assert handle.tts_ctc_best_path(1, 16, 4, 5, 4, None, utts, 1, 2, 1, 1, 1, 1, 1, None) != 0 and b"rows of 4" in handle.tts_last_error()
    pairs = (capi.TtsPronUtt * 2)(capi.TtsPronUtt(0, 4, 0, 3, -1), capi.TtsPronUtt(4, 9, 3, 2049, -1))
    assert handle.tts_edit_distance(1, 4000, 1, 16, 1, pairs, 1, 2, None, 0, 28672, 1, 1, 1, None) != 0 and b"utterance 1" in handle.tts_last_error()
    pairs[1].n_ref = 5
    pairs[1].scratch_off = 6
    assert handle.tts_edit_distance(1, 4000, 1, 16, 1, pairs, 1, 2, 1, 64, 16, 1, 1, 1, None) != 0 and b"pair 1" in handle.tts_last_error()
    assert handle.tts_phone_posteriors(1, 16, 5, 5, 1, 1, 3, pairs, 1, 2, 1, None) != 0 and b"utterance 1" in handle.tts_last_error()
