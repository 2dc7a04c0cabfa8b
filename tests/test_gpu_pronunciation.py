"""The pronunciation kernels (csrc/pronunciation.hip) on the MI355X against the float64 restatement in tests/pronunciation_ref.py:
the greedy decode, the prefix beam search on seeded inputs whose every selection is wide, the edit distance over a square of sizes
in both forms of the back-pointer store, the posterior scores over given durations, that a ragged batch equals its utterances alone
through ``check_logits``, a sentence with a known answer, and the entries of the interface on the fixture checkpoints (DESIGN.md
section 19)."""
import functools
import math

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, fixture_weights as fw, pronunciation as pron, resample
from ims_toucan_prosody_variance_amd.phonemes import phones_to_features
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import pronunciation_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK = capi.CTC_SCAN_BLOCK
FRAMES = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
PAD = 3  # unused columns behind the symbols: ld > n_symbols


@pytest.fixture(scope="module")
def chk():
    return pron.PronunciationChecker(fw.aligner_state_dict(), DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def one_ulp(got, want):
    """|got - want| is at most one fp32 step at want, entry by entry."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return got.shape == want.shape and bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


def same(x, y):
    """Two result dicts hold the same bits (NaN equal to NaN)."""
    return x.keys() == y.keys() and all(np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=np.asarray(x[k]).dtype.kind == "f") for k in x)


def spell(symbols, S, seed, gain=8.0):
    """Logits [T, S + PAD] whose best symbol per frame is given: unit noise with `gain` added at that symbol."""
    x = np.random.default_rng(seed).normal(0.0, 1.0, size=(len(symbols), S + PAD)).astype(np.float32)
    x[np.arange(len(symbols)), np.asarray(symbols)] += np.float32(gain)
    return x


# ---- tts_ctc_best_path ----------------------------------------------------------------------------------------------------------
def best_path_cases(S):
    """[(name, logits, drop)] with the blank S - 1."""
    blank = S - 1
    rng = np.random.default_rng(7 + S)
    cases = [(f"random {T}", (3.0 * rng.normal(size=(T, S + PAD))).astype(np.float32), None) for T in FRAMES]
    cases.append(("all blank", spell([blank] * (BLOCK + 1), S, 1), None))
    cases.append(("alternating", spell([t % 2 for t in range(2 * BLOCK + 1)], S, 2), None))
    straddle = [blank] * (2 * BLOCK + 1)
    straddle[BLOCK - 6:BLOCK + 5] = [2] * 11  # a run over the first block boundary
    straddle[2 * BLOCK] = 3  # a run that opens on a block's first frame
    cases.append(("straddle", spell(straddle, S, 3), None))
    opens = [blank] * (BLOCK + 4)
    opens[BLOCK:BLOCK + 3] = [1] * 3  # opens on frame BLOCK exactly
    cases.append(("opens on a block", spell(opens, S, 4), None))
    long = [blank] * (3 * BLOCK - 40)
    long[BLOCK - 50:3 * BLOCK - 100] = [0] * (2 * BLOCK - 50)  # a run that fills a whole block and is carried twice
    cases.append(("fills a block", spell(long, S, 5), None))
    cases.append(("equal symbols", spell([1, 1, blank, 1, 1, 2, 2, 1, blank, blank, 1], S, 6), None))
    ties = np.zeros((5, S + PAD), dtype=np.float32)  # exact ties: the lowest index wins, frame after frame
    ties[1, 1:] = 1.0
    ties[2, 2:] = 1.0
    ties[3, blank] = 1.0
    ties[4, [1, 3]] = 2.0
    cases.append(("ties", ties, None))
    drop = np.zeros(S, dtype=np.uint8)
    drop[[1, 3]] = 1
    cases.append(("drop", cases[FRAMES.index(BLOCK + 1)][1].copy(), drop))
    cases.append(("drop between equal symbols", spell([2, 2, 1, 2, 3, 3, 0, blank, 0], S, 8), drop))
    bad = cases[3][1].copy()
    bad[BLOCK - 2, S - 2] = np.nan
    cases.append(("nan", bad, None))
    return cases


@pytest.fixture(scope="module")
def best_path_runs(chk):
    """Per S and drop mask one ragged launch over its cases: {(S, name): (host arrays of the utterance, n_hyp)}."""
    out = {}
    for S in (5, 145):
        cases = best_path_cases(S)
        for with_drop in (False, True):
            group = [c for c in cases if (c[2] is not None) == with_drop]
            rag = Ragged([len(c[1]) for c in group], DEV)
            got = chk.best_path(dev(np.concatenate([c[1] for c in group])), rag, n_symbols=S, blank=S - 1, drop=group[0][2])
            host = {k: v.cpu().numpy() for k, v in got.items()}
            for b, c in enumerate(group):
                b0, n = rag.begins[b], int(host["n_hyp"][b])
                out[(S, c[0])] = ({k: host[k][b0:b0 + max(n, 0)] for k in ("hyp_id", "hyp_first", "hyp_last", "hyp_conf")}, n)
    return out


@pytest.mark.parametrize("S", [5, 145])
def test_best_path_against_the_restatement(best_path_runs, S):
    """Ids, spans and counts exactly; the confidences within one fp32 step (the fp64 exp and log may differ from the host's by a
    few fp64 ulps, which moves the one rounding to fp32 by at most one step)."""
    for name, x, drop in best_path_cases(S):
        want = pr.best_path(x[:, :S], S - 1, drop)
        got, n = best_path_runs[(S, name)]
        if name == "nan":
            assert want is None and n == -1
            continue
        assert n == len(want["ids"]), name
        assert list(got["hyp_id"]) == want["ids"] and list(got["hyp_first"]) == want["first"] and list(got["hyp_last"]) == want["last"], name
        assert got["hyp_conf"].dtype == np.float32 and one_ulp(got["hyp_conf"], np.asarray(want["conf"], dtype=np.float32)), name
    T = 2 * BLOCK + 1
    assert best_path_runs[(S, "all blank")][1] == 0 and best_path_runs[(S, "alternating")][1] == T
    got, n = best_path_runs[(S, "straddle")]
    assert n == 2 and list(got["hyp_first"]) == [BLOCK - 6, 2 * BLOCK] and list(got["hyp_last"]) == [BLOCK + 4, 2 * BLOCK]
    got, n = best_path_runs[(S, "opens on a block")]
    assert n == 1 and got["hyp_first"][0] == BLOCK and got["hyp_last"][0] == BLOCK + 2
    got, n = best_path_runs[(S, "fills a block")]
    assert n == 1 and got["hyp_first"][0] == BLOCK - 50 and got["hyp_last"][0] == 3 * BLOCK - 101
    assert list(best_path_runs[(S, "equal symbols")][0]["hyp_id"]) == [1, 1, 2, 1, 1]
    assert list(best_path_runs[(S, "ties")][0]["hyp_id"]) == [0, 1, 2, 1]  # (frame 3 is the blank alone)
    assert list(best_path_runs[(S, "drop between equal symbols")][0]["hyp_id"]) == [2, 2, 0, 0]


# ---- tts_ctc_beam_search --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def beam_case(case):
    return pr.beam_case(*case)


@pytest.mark.parametrize("W", pr.BEAM_WIDTHS)
@pytest.mark.parametrize("S", pr.BEAM_SYMBOLS)
def test_beam_search_against_the_restatement(chk, S, W):
    """The seeded cases of this symbol count and beam in one ragged launch.  Every case's seed (pr.BEAM_SEEDS: 0 throughout) keeps
    the gap between the W-th and the next candidate total above 1e-9 relative at every frame of the restatement, and between the
    best and the second total after the last frame, which picks the prefix that is returned - asserted here -,
    so a last-ulp difference of exp / log1p cannot choose another beam: the ids are exact.  The score within 1e-9 relative: at most
    3 T fp64 operations of a few ulps each give about 2e-12 at T = 600."""
    cases = [c for c in pr.BEAM_CASES if c[2] == S and c[3] == W]
    assert {c[1] for c in cases} >= set(pr.BEAM_FRAMES)
    solved = [beam_case(c) for c in cases]
    for c, (seed, x, _, gap) in zip(cases, solved):
        print(f"{c}: seed {seed}, smallest gap {gap:.3e}")
        assert seed == pr.BEAM_SEEDS[c] and gap > pr.MIN_GAP
    rag = Ragged([c[1] for c in cases], DEV)
    got = chk.beam_search(dev(np.concatenate([s[1] for s in solved])), rag, W, n_symbols=S, blank=S - 1)
    ids, n, score = got["hyp_id"].cpu().numpy(), got["n_hyp"].cpu().numpy(), got["score"].cpu().numpy()
    assert score.dtype == np.float64
    for b, (c, (_, _, (want_ids, want_score), _)) in enumerate(zip(cases, solved)):
        assert n[b] == len(want_ids) and list(ids[rag.begins[b]:rag.begins[b] + n[b]]) == want_ids, c
        rel = abs(score[b] - want_score) / abs(want_score)
        print(f"{c}: {n[b]} symbols, score {score[b]:.12g}, relative error {rel:.2e}")
        assert rel <= 1e-9, c


def test_beam_search_when_a_prefix_is_pruned_and_made_again(chk):
    """pr.REMADE_CASES: tables of 3 to 5 symbols at beams of 2 to 8 in which a prefix leaves the beams while a child of it lives on
    and is made again from its own parent; extending it must still be joined into that child (the prefixes are compared by what
    they spell, not by the node they were made as).  Ids exactly, the score within 1e-9 relative; the gap is asserted as above."""
    for S in sorted({c[2] for c in pr.REMADE_CASES}):
        for W in sorted({c[3] for c in pr.REMADE_CASES if c[2] == S}):
            cases = [c for c in pr.REMADE_CASES if c[2] == S and c[3] == W]
            solved = [pr.remade_case(*c) for c in cases]
            assert all(gap > pr.MIN_GAP and frames >= 1 for _, _, gap, frames in solved)
            rag = Ragged([c[1] for c in cases], DEV)
            got = chk.beam_search(dev(np.concatenate([s[0] for s in solved])), rag, W, n_symbols=S, blank=S - 1)
            ids, n, score = got["hyp_id"].cpu().numpy(), got["n_hyp"].cpu().numpy(), got["score"].cpu().numpy()
            for b, (c, (_, (want_ids, want_score), _, _)) in enumerate(zip(cases, solved)):
                rel = abs(score[b] - want_score) / abs(want_score)
                print(f"{c}: {list(ids[rag.begins[b]:rag.begins[b] + n[b]])}, score {score[b]:.12g}, relative error {rel:.2e}")
                assert n[b] == len(want_ids) and list(ids[rag.begins[b]:rag.begins[b] + n[b]]) == want_ids, c
                assert rel <= 1e-9, c


def test_beam_search_merges_drops_and_refuses(chk):
    """The merge case meets a live beam at most frames (counted in the restatement); a drop mask; a beam of one against the
    three-frame table where the search and the best path disagree; a NaN gives -1."""
    S = 5
    x = pr.beam_inputs(0, 33, S, "merge")
    met = []
    pr.beam_search(x[:, :S], S - 1, 8, merges=met)
    assert sum(m > 0 for m in met) >= 30
    drop = np.array([0, 0, 1, 0, 0], dtype=np.uint8)
    y = pr.beam_inputs(0, 33, S)
    gaps = []
    want = pr.beam_search(y[:, :S], S - 1, 8, drop=drop, gaps=gaps, final_gap=gaps)
    assert min(gaps) > pr.MIN_GAP and 2 not in want[0]
    three = np.zeros((3, S + PAD), dtype=np.float32)
    three[:, :S] = np.log(np.array([0.45, 0.02, 0.02, 0.01, 0.5]))
    bad = y.copy()
    bad[17, 1] = np.inf
    rag = Ragged([33, 3, 33], DEV)
    got = chk.beam_search(dev(np.concatenate([y, three, bad])), rag, 8, n_symbols=S, blank=S - 1, drop=drop)
    ids, n, score = got["hyp_id"].cpu().numpy(), got["n_hyp"].cpu().numpy(), got["score"].cpu().numpy()
    assert list(n) == [len(want[0]), 1, -1] and list(ids[:n[0]]) == want[0] and abs(score[0] - want[1]) <= 1e-9 * abs(want[1])
    assert ids[33] == 0 and abs(score[1] - pr.beam_search(three[:, :S], S - 1, 8, drop=drop)[1]) < 1e-12
    greedy = chk.best_path(dev(three), Ragged([3], DEV), n_symbols=S, blank=S - 1)
    assert int(greedy["n_hyp"][0]) == 0
    with pytest.raises(ValueError, match="beam is an integer"):
        chk.beam_search(dev(three), Ragged([3], DEV), 33, n_symbols=S, blank=S - 1)


# ---- tts_edit_distance ----------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 257)
UNWRITTEN = -2  # what the maps hold before the launch: a -1 in range is one the kernel stored


@functools.lru_cache(maxsize=None)
def edit_pairs():
    """[(ref, hyp)]: the whole square of SIZES over an alphabet of four, then the named cases, then one pair past the LDS form."""
    rng = np.random.default_rng(11)
    seq = lambda n: [int(v) for v in rng.integers(0, 4, n)]
    pairs = [(seq(R), seq(H)) for R in SIZES for H in SIZES]
    base = [int(v) for v in rng.permutation(65)]  # (distinct: the alignments below are the only ones of their cost)
    pairs.append((base, list(base)))  # identical
    pairs.append((base, [v + 100 for v in base]))  # completely different
    pairs.append((base, base[:20] + [99] + base[21:]))  # one substitution, at 20
    pairs.append((base, base[:33] + base[34:]))  # one deletion, of 33
    pairs.append((base, base[:40] + [98] + base[40:]))  # one insertion, before 40
    pairs.append((seq(520), seq(700)))  # three bands of rows; its back-pointers do not fit the LDS form
    return pairs


@functools.lru_cache(maxsize=None)
def edit_solved():
    return [pr.levenshtein(r, h) for r, h in edit_pairs()]


@pytest.fixture(scope="module")
def edit_runs(chk):
    pairs = edit_pairs()
    rag = Ragged([max(len(h), 1) for _, h in pairs], DEV)
    hyp = np.zeros(rag.total_rows, dtype=np.int32)
    for b, (_, h) in enumerate(pairs):
        hyp[rag.begins[b]:rag.begins[b] + len(h)] = h
    n_hyp = dev(np.asarray([len(h) for _, h in pairs], dtype=np.int32))
    return rag, {force: chk.edit_distance([r for r, _ in pairs], dev(hyp), n_hyp, rag, force_scratch=force, fill=UNWRITTEN) for force in (False, True)}


def test_edit_distance_against_the_restatement(edit_runs):
    """Counts and both maps exactly, for every pair; both forms of the back-pointer store return the same bits."""
    rag, runs = edit_runs
    pairs = edit_pairs()
    sizes = [pron.bp_bytes(len(r), max(len(h), 1)) for r, h in pairs]
    assert any(0 < s <= capi.EDIT_LDS_BP_BYTES for s in sizes) and any(s > capi.EDIT_LDS_BP_BYTES for s in sizes)
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a, b)
    counts, r2h, h2r = (t.cpu().numpy() for t in runs[False])
    assert (r2h != UNWRITTEN).all()  # every reference token was written; the hypothesis tokens are checked pair by pair
    at = 0
    for b, ((ref, hyp), (want, want_r2h, want_h2r)) in enumerate(zip(pairs, edit_solved())):
        assert tuple(counts[b]) == want, (len(ref), len(hyp))
        assert list(r2h[at:at + len(ref)]) == want_r2h and list(h2r[rag.begins[b]:rag.begins[b] + len(hyp)]) == want_h2r, (len(ref), len(hyp))
        at += len(ref)
    n = len(SIZES) ** 2
    assert tuple(counts[n]) == (65, 0, 0, 0) and tuple(counts[n + 1]) == (0, 65, 0, 0)
    assert tuple(counts[n + 2]) == (64, 1, 0, 0) and tuple(counts[n + 3]) == (64, 0, 1, 0) and tuple(counts[n + 4]) == (65, 0, 0, 1)
    first = sum(len(r) for r, _ in pairs[:n])
    assert r2h[first + 3 * 65 + 33] == -1 and h2r[rag.begins[n + 4] + 40] == -1 and r2h[first + 2 * 65 + 20] == 20


def test_edit_distance_of_a_failed_decode(chk):
    """n_hyp = -1 (a decode that met a NaN) and an n_hyp past the utterance's frames give counts of -1; the pair beside them is
    computed."""
    rag = Ragged([4, 3, 4], DEV)
    hyp = dev(np.asarray([1, 2, 3, 0, 0, 0, 0, 1, 2, 3, 9], dtype=np.int32))
    counts, r2h, h2r = chk.edit_distance([[1, 2, 3], [1, 2], [1, 2, 3]], hyp, dev(np.asarray([-1, 4, 3], dtype=np.int32)), rag, fill=UNWRITTEN)
    assert counts.cpu().tolist() == [[-1] * 4, [-1] * 4, [3, 0, 0, 0]]
    assert r2h.cpu().tolist() == [UNWRITTEN] * 5 + [0, 1, 2] and h2r.cpu().tolist() == [UNWRITTEN] * 7 + [0, 1, 2, UNWRITTEN]  # (no maps for a failed pair)


# ---- tts_phone_posteriors -------------------------------------------------------------------------------------------------------
def posterior_cases(S):
    """[(logits, durations, ids)]: per frame count a random partition with zeros and word boundaries, one whose first token owns
    no frame, more tokens than one chunk of the scan, a partition that does not add up and one that MAS could not make."""
    rng = np.random.default_rng(23 + S)
    cases = []
    for T in FRAMES:
        x = (3.0 * rng.normal(size=(T, S + PAD))).astype(np.float32)
        K = min(T, 12) + 3
        cuts = np.sort(rng.choice(np.arange(1, T), size=min(K - 4, T - 1), replace=False)) if T > 1 else np.zeros(0, dtype=np.int64)
        d = list(np.diff(np.concatenate([[0], cuts, [T]])))  # the first token owns frame 0, the last one frame T - 1
        while len(d) < K:
            d.insert(int(rng.integers(1, max(len(d), 2))), 0)  # (a single frame: the zeros follow its token)
        ids = [int(v) for v in rng.integers(0, S, K)]
        big = int(np.argmax(d))
        ids[big] = int(np.argmax(x[sum(d[:big]), :S]))  # the longest token is the best symbol of its first frame
        ids[2 if big == 1 else 1] = -1  # a word boundary
        cases.append((x, [int(v) for v in d], ids))
    x = cases[-1][0]
    T = len(x)
    cases.append((x, [0, T - 5, 0, 5, 0], [1, 2, -1, 3, 0]))  # the first and the last token own nothing
    many = [1] * 300 + [0] * 40 + [T - 300]
    cases.append((x, many, [int(v) for v in rng.integers(0, S, len(many))]))  # tokens past one chunk of 256
    cases.append((x, [T - 6, 5], [1, 2]))  # does not add up
    cases.append((x, [T, 5], [1, 2]))  # leaves the frames
    cases.append((x, [-1, -1, -1], [1, 2, 3]))  # MAS could not run
    return cases


@pytest.mark.parametrize("S", [5, 145])
def test_phone_posteriors_against_the_restatement(chk, S):
    """The frames and the frame accuracy exactly, the two means within one fp32 step; the gop is never positive."""
    cases = posterior_cases(S)
    rag = Ragged([len(c[0]) for c in cases], DEV)
    dur = dev(np.concatenate([np.asarray(c[1], dtype=np.int32) for c in cases]))
    got = chk.phone_posteriors(dev(np.concatenate([c[0] for c in cases])), rag, dur, [c[2] for c in cases], n_symbols=S).cpu().numpy()
    at = 0
    for n, (x, d, ids) in enumerate(cases):
        want, rows = pr.phone_posteriors(x[:, :S], d, ids), got[at:at + len(ids)]
        at += len(ids)
        assert np.array_equal(np.isnan(rows), np.isnan(want)), n
        ok = ~np.isnan(want[:, 0])
        assert np.array_equal(rows[:, 3], want[:, 3], equal_nan=True) and np.array_equal(rows[ok, 2], want[ok, 2]), n
        assert one_ulp(rows[ok, 0], want[ok, 0]) and one_ulp(rows[ok, 1], want[ok, 1]), n
        assert (rows[ok, 1] <= 0).all()
        if n < len(FRAMES):
            assert ok.sum() >= 1 and (len(x) == 1 or rows[ok, 2].max() > 0)
    assert np.isnan(got[-3 - 2 - 2:]).all()


# ---- a ragged batch equals its utterances alone, through check_logits -----------------------------------------------------------
TEXTS = ["~həlˈoʊ~#", "~wˈɜːld tˈu~#", "~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#", "~həlˈoʊ wˈɜːld~#", "~nnˈaʊ tˈɛn~#", "~tˈu~#", "~tˈu~#", "~tˈu~#"]
BATCH_FRAMES = (12, BLOCK - 1, 2 * BLOCK + 1, BLOCK, BLOCK + 1, 40, 2 * BLOCK + 1, 40)
SCRIPTED, FAILED = 6, 7  # the utterance of scripted runs and ties, and the one that holds a NaN


@pytest.mark.parametrize("beam", [0, 8])
def test_a_batch_equals_its_utterances_alone(chk, beam):
    """Eight utterances on both sides of the scan block, the reference's silence ignored: six of noise in which every third frame
    spells the text; one scripted like the cases of the best-path test - a run of the text's second phoneme over the first block
    boundary, one that opens on the second block's first frame, two frames of exact ties - and one with a NaN logit, whose
    n_hyp = -1 goes through the edit distance inside the batch.  Every dict of the batch holds the bits of the utterance checked
    alone.  (Durations that do not add up cannot reach check_logits: tts_mas_durations always spends every frame.)"""
    rng = np.random.default_rng(31)
    feats = [phones_to_features(t, handle_missing=False) for t in TEXTS]
    logits = [(3.0 * rng.normal(size=(T, pron.N_SYMBOLS))).astype(np.float32) for T in BATCH_FRAMES]
    for x, f in zip(logits, feats):  # some frames spell the text, so that hits, substitutions and deletions all occur
        ids = pron.reference_tokens(f)[0]
        for k, t in enumerate(range(0, len(x) - 1, 3)):
            x[t, ids[k % len(ids)]] += 12.0
    silence = int(pron.reference_tokens(feats[0])[0][0])
    said = int(pron.reference_tokens(feats[SCRIPTED])[0][1])
    script = [pron.BLANK] * BATCH_FRAMES[SCRIPTED]
    script[BLOCK - 6:BLOCK + 5] = [said] * 11
    script[2 * BLOCK] = said
    logits[SCRIPTED] = spell(script, pron.N_SYMBOLS - PAD, 41)
    logits[SCRIPTED][[3, 4]] = 0.0  # exact ties: symbol 0, the ignored silence, is the best of both frames
    logits[FAILED][7, 3] = np.nan
    rag = Ragged(BATCH_FRAMES, DEV)
    batch = chk.check_logits(dev(np.concatenate(logits)), rag, feats, beam=beam, ignore_ids=[silence])
    assert len(batch) == 8 and silence == 0 and all(len(pron.reference_tokens(f)[0]) <= T for f, T in zip(feats, BATCH_FRAMES))
    fine = [r for b, r in enumerate(batch) if b != FAILED]
    assert all(r["hits"] + r["substitutions"] + r["deletions"] == r["n_ref"] and r["hits"] + r["substitutions"] + r["insertions"] == r["n_hyp"]
               for r in fine)
    assert any(r["hits"] > 0 for r in fine) and all(silence not in r["hyp_ids"] for r in batch)
    assert all(int(r["durations"].sum()) == T and len(r["gop"]) == len(f) for r, f, T in zip(batch, feats, BATCH_FRAMES))
    assert ("beam_score" in batch[1]) == (beam > 0) and ("hyp_conf" in batch[1]) == (beam == 0)
    bad = batch[FAILED]
    assert bad["n_hyp"] == -1 and bad["hits"] == -1 and math.isnan(bad["per"]) and len(bad["hyp_ids"]) == 0 and (bad["ref_to_hyp"] == -1).all()
    if beam == 0:
        r = batch[SCRIPTED]
        assert list(r["hyp_ids"]) == [said, said] and list(r["hyp_first"]) == [BLOCK - 6, 2 * BLOCK] and list(r["hyp_last"]) == [BLOCK + 4, 2 * BLOCK]
    for b in range(8):
        alone = chk.check_logits(dev(logits[b]), Ragged([BATCH_FRAMES[b]], DEV), [feats[b]], beam=beam, ignore_ids=[silence])[0]
        assert same(batch[b], alone), b


# ---- a sentence with a known answer ---------------------------------------------------------------------------------------------
def test_a_sentence_with_a_known_answer(chk):
    """Logits that spell a 12-token reference with token 2 substituted, token 6 deleted and a symbol inserted behind token 9, three
    frames per symbol and a blank frame between them, at high confidence: per = 3 / 12, the three operations at those tokens, and
    the beam search agrees with the best path.  In the substituted frames the reference symbol is the runner-up (45 below the
    wrong one), so the forced alignment gives them to it: its gop is the lowest - the deleted token owns frames that are 20 below."""
    feats = phones_to_features("~wˈʌns əpˈɑːn ɐ mˈɪdnaɪt~#", handle_missing=False)
    ids_all, flags = pron.reference_tokens(feats)[:2]
    keep = np.nonzero((flags & 1) == 0)[0][11] + 1  # the rows up to the twelfth token that is no word boundary
    feats = feats[:keep]
    ids, _, full_ids, ref, ref_tokens = pron.reference_tokens(feats)
    assert len(ref) == 12
    unused = [i for i in range(pron.BLANK) if i not in set(int(v) for v in ref)]
    wrong, extra = unused[0], unused[1]
    spoken = []  # (symbol, runner-up or None)
    for k, r in enumerate(ref):
        if k == 6:
            continue
        spoken.append((wrong, int(r)) if k == 2 else (int(r), None))
        if k == 9:
            spoken.append((extra, None))
    T = 4 * len(spoken) + 1
    x = np.zeros((T, pron.N_SYMBOLS), dtype=np.float32)
    x[:, pron.BLANK] = 20.0
    for n, (sym, second) in enumerate(spoken):
        x[4 * n + 1:4 * n + 4, pron.BLANK] = 0.0
        x[4 * n + 1:4 * n + 4, sym] = 20.0 if second is None else 60.0
        if second is not None:
            x[4 * n + 1:4 * n + 4, second] = 15.0
    hyp = [s for s, _ in spoken]
    want_counts, want_r2h, want_h2r = pr.levenshtein([int(v) for v in ref], hyp)
    assert want_counts == (10, 1, 1, 1) and want_r2h[6] == -1 and want_r2h[2] == 2 and want_h2r[9] == -1
    results = {beam: chk.check_logits(dev(x), Ragged([T], DEV), [feats], beam=beam)[0] for beam in (0, 8)}
    for beam, r in results.items():
        assert r["per"] == 3 / 12 and (r["hits"], r["substitutions"], r["deletions"], r["insertions"]) == (10, 1, 1, 1)
        assert list(r["hyp_ids"]) == hyp and r["n_ref"] == 12 and r["n_hyp"] == 12
        assert list(r["ref_to_hyp"][ref_tokens]) == want_r2h and r["ref_to_hyp"][ref_tokens[6]] == -1
        assert list(r["hyp_to_ref"]) == [-1 if i < 0 else int(ref_tokens[i]) for i in want_h2r]
        assert r["gop_argmin"] == ref_tokens[2] and r["gop_min"] < -24 and int(r["durations"].sum()) == T
        assert math.isfinite(r["ctc_loss"]) and len(r["gop"]) == len(feats) and r["hyp_phones"] == [pron.id_to_phone()[i] for i in hyp]
    assert list(results[0]["hyp_first"]) == [4 * n + 1 for n in range(12)] and list(results[0]["hyp_last"]) == [4 * n + 3 for n in range(12)]
    assert results[8]["beam_score"] > -1e-6 * T and (results[0]["hyp_conf"] > -1e-6).all()


# ---- the interface --------------------------------------------------------------------------------------------------------------
PHONES = ["~həlˈoʊ wˈɜːld~#", "~wˈʌns əpˈɑːn mˈɪdnaɪt~#"]
WAVES = ("synth",)


def strip(r):
    return {k: v for k, v in r.items() if k not in WAVES}


def test_check_pronunciation_end_to_end(tmp_path, monkeypatch):
    """With the fixture checkpoints (seeded weights: the decoded phonemes are noise, this checks plumbing and identities, not
    quality): ``check_pronunciation`` equals ``PronunciationChecker.check`` on the waves ``synthesize_batch`` returns, a batch equals
    its texts alone, every variant of a grid gets the dict of that variant alone, calls without the new keywords return the bits
    they returned before the checker existed, and every refused keyword raises."""
    from ims_toucan_prosody_variance_amd import interface
    models = tmp_path / "Models"
    interface.write_fixture_checkpoints(str(models), n_lang=20)
    interface.write_fixture_aligner_checkpoint(str(models))
    monkeypatch.setattr(interface, "MODELS_DIR", str(models))
    monkeypatch.delenv("TOUCAN_PY_SEQUENCER", raising=False)
    monkeypatch.setenv("TOUCAN_PRECISION", "bf16")  # the 16-bit contract: a wave holds the same bits whatever its batch
    tts = interface.ToucanTTSInterface(device=DEV, tts_model_path="Meta", faster_vocoder=True)
    tts.set_language("en")
    tts.synthesize_batch(PHONES)
    zs = [torch.from_numpy(fw.normal(f"pron.z{u}", (80, int(d.sum())), 1, 0.8)) for u, d in enumerate(tts.last_durations)]
    grid_kw = dict(duration_scaling_factors=(1.0, 1.3), pitch_variance_scales=(1.0, 1.6))
    frames = [v["frames"] for v in tts.synthesize_grid(PHONES[0], **grid_kw)]
    grid_z = [torch.from_numpy(fw.normal(f"pron.grid{n}", (80, f), 1, 0.8)) for n, f in enumerate(frames)]
    before_batch = [w.cpu().numpy() for w in tts.synthesize_batch(PHONES, z_noise=zs)]
    before_grid = tts.synthesize_grid(PHONES[0], z_noise=grid_z, **grid_kw)
    assert getattr(tts, "_checker_obj", None) is None

    res = tts.check_pronunciation(PHONES, z_noise=zs, keep_waves=True)
    assert len(res) == 2 and all(np.array_equal(r["synth"], w) and r["synth"].dtype == np.float32 for r, w in zip(res, before_batch))
    own = pron.PronunciationChecker(fw.aligner_state_dict(), DEV)
    again = own.check(PHONES, before_batch, 24000)
    for r, a in zip(res, again):
        assert same(strip(r), a)
        assert r["hits"] + r["substitutions"] + r["deletions"] == r["n_ref"] and r["hits"] + r["substitutions"] + r["insertions"] == r["n_hyp"]
        assert r["per"] == (r["substitutions"] + r["deletions"] + r["insertions"]) / r["n_ref"] and math.isfinite(r["ctc_loss"])
        assert int(r["durations"].sum()) == 1 + resample.out_length(len(r["synth"]), 24000, 16000) // 256
        ok = ~np.isnan(r["gop"])
        assert ok.any() and (r["gop"][ok] <= 0).all() and r["gop_min"] == r["gop"][ok].min() and math.isfinite(r["beam_score"])
    for u in range(2):
        alone = tts.check_pronunciation([PHONES[u]], z_noise=[zs[u]])[0]
        assert same(alone, strip(res[u])), u
    greedy = tts.check_pronunciation(PHONES, z_noise=zs, beam=0, ignore_ids=[int(res[0]["hyp_ids"][0])] if res[0]["n_hyp"] > 0 else ())
    assert "hyp_conf" in greedy[0] and "beam_score" not in greedy[0] and all(len(g["gop"]) == len(r["gop"]) for g, r in zip(greedy, res))

    grid = tts.synthesize_grid(PHONES[0], z_noise=grid_z, check_pronunciation=True, **grid_kw)
    assert len(grid) == 4
    for n, (v, b) in enumerate(zip(grid, before_grid)):
        assert torch.equal(v["wave"], b["wave"]) and v["scales"] == b["scales"] and set(v) == set(b) | {"pronunciation"}
        d, p, e, s = v["scales"]
        alone = tts.check_pronunciation([PHONES[0]], z_noise=[grid_z[n]], duration_scaling_factor=[d], pitch_variance_scale=[p],
                                        energy_variance_scale=[e], pause_duration_scaling_factor=[s])[0]
        assert same(v["pronunciation"], alone), n

    after_batch = [w.cpu().numpy() for w in tts.synthesize_batch(PHONES, z_noise=zs)]
    after_grid = tts.synthesize_grid(PHONES[0], z_noise=grid_z, **grid_kw)
    assert all(np.array_equal(a, b) for a, b in zip(after_batch, before_batch))
    assert all(torch.equal(a["wave"], b["wave"]) and set(a) == set(b) and "pronunciation" not in a for a, b in zip(after_grid, before_grid))

    for kw in (dict(distributed=True), dict(sample_rate=16000), dict(pcm16=True), dict(loudness=-23.0), dict(speech_level=-26.0)):
        with pytest.raises(ValueError):
            tts.check_pronunciation(PHONES, **kw)
    with pytest.raises(ValueError):
        tts.check_pronunciation(PHONES, beam=33)
    with pytest.raises(ValueError):
        tts.synthesize_grid(PHONES[0], check_pronunciation=True, beam=-1)
    with pytest.raises(capi.ToucanHipError):
        pron.PronunciationChecker(fw.aligner_state_dict(), "cpu")
