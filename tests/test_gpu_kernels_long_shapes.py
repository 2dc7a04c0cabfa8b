"""The per-utterance kernels past one sweep of 256 items, one chunk of 8 utterances and the capped grid: library entry points
against plain float64 restatements (torch.nn.functional, torch.repeat_interleave, torch's float64 CTC, the oracle's functions and
tests/aligner_ref.py / tests/scorer_ref.py) - never against the ABI emulator.  The inputs, references and assertions live in
tests/long_shape_cases.py; tests/test_long_shape_references_cpu.py checks those references themselves.  fp32 results lie within
2e-5 of the output scale, integers are exact, everything is seeded.

The code path each test exists to reach (retire the test with the path):

* test_length_regulator_*            csrc/sequence_ops.hip length_regulate_kernel: the second and later sweeps of the 256-wide
                                     inclusive scan and their running carry (L = 257, 600, 4096 = LR_MAX_PHONES), runs of zero
                                     durations across a sweep edge, the all-zero utterance beside others; the host's limit check.
* test_prosody_control_*             csrc/prosody.hip prosody_control_kernel / scale_variance: the r += 256 stride loops (1000, 257 rows), the NaN
                                     mean of an all-unvoiced pitch row, scale 0 and scale 1.
* test_duration_head_*               duration_kernel: both clamps (0 and 1e6), expf next to a half, 16 blocks.
* test_glow_mix_*                    glow_mix_kernel: the stride loop behind the 2048-block grid cap (rows * 40 > 524 288: 13 108
                                     and 14 000 rows; 13 107 is the last shape without it), a row stride larger than c.
* test_dwconv_swish_*                dwconv_swish_kernel: C = 80 (a partial 64-lane channel tile), utterances shorter than the
                                     half-kernel beside tile edges (1, 2, 15, 16 frames; 63, 64, 65), a saturated swish.
* test_lstm_three_chunks_*           csrc/align.hip lstm_step_kernel<32>: blockIdx.z > 0 (19 utterances = chunks of 8, 8, 3), a chunk
                                     whose utterances end early, a partial last chunk.
* test_lstm_hidden_256_*             lstm_step_kernel<16> (hidden == 256, KPT = 16).
* test_mas_*                         mas_durations_kernel: the j0 loop over token blocks of 256, a last block where only some
                                     wavefronts own a bit word (W * 64 = 320, 384, 1024, 8192), the LDS and the scratch form,
                                     the limit of 8192 tokens.
* test_token_average_*               token_average_kernel: k += AVG_THREADS (257, 1500 tokens), durations whose sum passes T (the
                                     min(cum, T) clamp), an utterance with every token dropped.
* test_ctc_*                         csrc/score.hip ctc_loss_kernel: the > 64 KiB LDS launch (raise_lds_limit; n = 1250, 2048 = the
                                     limit), n = 0, T = 1, the infeasible case; the host's limit check.

Measured on the MI355X: see DESIGN.md §4, "long shapes"."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import align, capi, engine, fixture_weights as fw, scorer
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import aligner_ref as ar
from tests import long_shape_cases as lc
from tests.test_gpu_kernels_vs_float64 import DEV, TOL

pytestmark = pytest.mark.gpu
TO = lc.mover(DEV)
assert TOL[capi.COMPUTE_F32] == lc.TOL32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return engine.Ops(DEV)


@pytest.fixture(scope="module")
def extractor():
    return align.ProsodyExtractor(fw.aligner_state_dict(), DEV)


@pytest.fixture(scope="module")
def eng(extractor):
    return extractor.aligner


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


# ---- 1. length regulator ---------------------------------------------------------------------------------------------------
def test_length_regulator_scan_past_one_sweep(ops):
    up, dec, ragf = lc.run_length_regulate(ops, TO)
    torch.cuda.synchronize()
    print(f"length regulator: largest error {lc.check_length_regulate(up, dec, ragf):.2e} of the output scale")


def test_length_regulator_refuses_more_phonemes_than_its_scan_holds(ops):
    """4097 phonemes: the argument check fails on the host, before any launch."""
    with pytest.raises(capi.ToucanHipError, match="4097 phonemes"):
        lc.run_length_regulate(ops, TO, lengths=[4097])
    torch.cuda.synchronize()


# ---- 2. prosody control ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", lc.PC_SCALES)
def test_prosody_control_long_utterances(ops, scales):
    assert lc.prosody_half_distance(scales) > 1e-3  # no rounded product near a half: the durations must match exactly
    p, e, d = lc.run_prosody(ops, TO, scales)
    torch.cuda.synchronize()
    print(f"prosody control {scales}: largest error {lc.check_prosody(p, e, d, scales):.2e} of the output scale")


# ---- 3. duration head ------------------------------------------------------------------------------------------------------
def test_duration_head_clamps_and_halves(ops):
    d = lc.run_duration(ops, TO)
    torch.cuda.synchronize()
    excused = lc.check_duration(d)
    print(f"duration head: {excused} of {lc.DUR_N} durations differ from fp32 torch, all next to a half "
          f"({int(lc.duration_case().near_half.sum())} inputs lie there)")
    assert excused <= lc.DUR_EXCUSED_MAX


# ---- 4. Glow inverse mix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,pad", [(77, 0), (13107, 0), (13108, 0), (13108, 16), (14000, 0)])
def test_glow_mix_past_the_grid_cap(ops, rows, pad):
    buf = lc.run_glow(ops, TO, rows, pad)
    torch.cuda.synchronize()
    print(f"glow mix, {rows} rows, row stride {lc.GLOW_C + pad}: largest error {lc.check_glow(buf, rows):.2e} of the output scale")


# ---- 5. depthwise conv + swish ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c,family", lc.DW_CASES)
def test_dwconv_swish_vs_float64(ops, k, c, family):
    y = lc.run_dwconv(ops, TO, k, c, family)
    torch.cuda.synchronize()
    print(f"dwconv k = {k}, C = {c}, {family}: largest error {lc.check_dwconv(y, k, c, family):.2e} of the output scale")


# ---- 6. LSTM recurrence ----------------------------------------------------------------------------------------------------
def _lstm_case(lstm, w_hh_t, H, lens, what):
    rag = Ragged(lens, DEV)
    xproj = fw.normal("long.lstm.x", (rag.total_rows, 8 * H), 5, 0.5)
    y = lstm(_t(xproj), rag, poison_state=True).cpu().numpy()
    assert np.isfinite(y).all()
    err = float(np.abs(y - ar.lstm_reference(xproj, w_hh_t, lens, H)).max())
    print(f"{what}: max abs error vs float64 {err:.2e}")
    assert err < 2e-4
    for b, (b0, n) in enumerate(zip(rag.begins, lens)):
        one = lstm(_t(xproj[b0:b0 + n]), Ragged([n], DEV), poison_state=True).cpu().numpy()
        assert np.array_equal(one, y[b0:b0 + n]), f"utterance {b} alone differs from its rows of the batch"


def test_lstm_three_chunks_of_utterances(eng):
    lens = [40, 1, 7, 33, 2, 40, 12, 5, 1, 40, 3, 9, 40, 2, 2, 2, 17, 40, 6]
    assert eng.H == 512
    _lstm_case(eng.lstm, eng.w_hh_t, 512, lens, "lstm, H = 512, 19 utterances")


def test_lstm_hidden_256_instantiation(ops):
    """tts_lstm_recurrence with hidden = 256 through AlignerEngine.lstm's own launch loop, on seeded weights blocked by align.block_w_hh."""
    H = 256
    w_hh_t = fw.normal("long.lstm.w_hh", (2, H, 4 * H), 6, 1.0 / np.sqrt(H))
    shim = SimpleNamespace(ops=ops, H=H, device=ops.device, w_hh_blk=_t(align.block_w_hh(w_hh_t)))
    lstm = lambda x, rag, poison_state=False: align.AlignerEngine.lstm(shim, x, rag, poison_state)
    _lstm_case(lstm, w_hh_t, H, [1, 2, 37, 130], "lstm, H = 256")


# ---- 7. MAS ----------------------------------------------------------------------------------------------------------------
def _mas_gpu(eng, cases, flags, force_scratch):
    rag = Ragged([c.logits.shape[0] for c in cases], DEV)
    lg = _t(np.concatenate([c.logits for c in cases]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d, begins = eng.durations(lg, rag, [c.ids for c in cases], flags, force_scratch)
    d = d.cpu().numpy()
    ms = (time.perf_counter() - t0) * 1e3
    return [d[b:b + len(f)] for b, f in zip(begins, flags)], ms


def _check_mas(c, got, pm):
    assert np.array_equal(got, c.dur), "durations differ from the float32 restatement"
    gap = lc.mas_rel_gap(ar.mas_float64_score(pm, got), c.optimum)
    assert gap <= lc.MAS_REL
    return gap


@pytest.mark.parametrize("force_scratch", [False, True])
def test_mas_token_blocks_past_256(eng, force_scratch):
    """Four shapes in one batch (257, 321, 300 and 1000 tokens: 2 - 4 token blocks, last blocks of 1, 2, 1 and 4 bit words), the
    L = 300 one a second time with word-boundary and repeat flags.  Without force_scratch the host keeps 700 x 257, 640 x 321 and
    900 x 300 in LDS and sends 2500 x 1000 to the scratch buffer."""
    cases = [lc.mas_case(i) for i in range(4)]
    flagged = cases[lc.MAS_FLAGGED]
    flags = [np.zeros(len(c.ids), np.int32) for c in cases] + [flagged.flags]
    got, ms = _mas_gpu(eng, cases + [flagged], flags, force_scratch)
    worst = max(_check_mas(c, g, c.logits[:, c.ids]) for c, g in zip(cases, got))
    assert np.array_equal(got[4], flagged.dur_flagged), "word-boundary zeros / repeat repair"
    print(f"MAS ({'scratch' if force_scratch else 'LDS where it fits'}), 4 + 1 utterances: {ms:.0f} ms; exact; float64 score within "
          f"{worst:.1e} of the optimum")


@pytest.mark.parametrize("force_scratch", [False, True])
def test_mas_at_the_limit_of_8192_tokens(eng, force_scratch):
    c = lc.mas_case(4)
    got, ms = _mas_gpu(eng, [c], [np.zeros(len(c.ids), np.int32)], force_scratch)
    gap = _check_mas(c, got[0], c.logits[:, c.ids])
    T, L = lc.MAS_SHAPES[4]
    print(f"MAS {T} x {L} ({'scratch, no LDS bits' if force_scratch else 'scratch'}): {ms:.0f} ms; exact; float64 score within {gap:.1e} "
          f"of the optimum")


# ---- 8. token averages -----------------------------------------------------------------------------------------------------
def test_token_average_past_256_tokens(extractor):
    """Token counts 1, 256, 257, 1500 (~3 frames per token, zero durations mixed in), one utterance whose durations sum to T + 50
    (reference: the durations truncated at T), one with every token dropped (NaN, as the reference's mean of an empty selection)."""
    rng = np.random.default_rng(41)
    durs, keeps, frames, trunc = [], [], [], []
    for u, n_tok in enumerate([1, 256, 257, 1500, 300, 40]):
        d = rng.integers(1, 7, n_tok).astype(np.int32)
        d[rng.random(n_tok) < 0.2] = 0
        d[0] = 3
        T = int(d.sum()) - (50 if u == 4 else 0)
        k = rng.random(n_tok) > 0.2
        k[0] = True
        if u == 5:
            k[:] = False
        cum = np.minimum(np.cumsum(d), T)
        durs.append(d), keeps.append(k), frames.append(T), trunc.append(np.diff(np.concatenate([[0], cum])))
    assert trunc[4].sum() == frames[4] and (trunc[4] != durs[4]).sum() > 5 and all(np.array_equal(a, b) for a, b in zip(trunc[:4], durs[:4]))
    rag = Ragged(frames, DEV)
    x = np.abs(rng.standard_normal(rag.total_rows)).astype(np.float32)
    x[rng.random(rag.total_rows) < 0.3] = 0.0
    n_full = [len(d) for d in durs]
    full_begin = lc.begins_of(n_full)
    dd = _t(np.concatenate(durs), torch.int32)
    for mode in (0, 1):
        out = extractor.token_average(_t(x), rag, dd, np.concatenate(keeps), full_begin, n_full, mode).cpu().numpy()
        worst = 0.0
        for b, (b0, n) in enumerate(zip(rag.begins, frames)):
            want = ar.token_average(x[b0:b0 + n], trunc[b], keeps[b], mode)
            got = out[full_begin[b]:full_begin[b] + n_full[b]]
            assert np.isnan(want).all() == (b == 5)
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7, equal_nan=True)
            if b != 5:
                worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        print(f"token average, mode {mode}: largest error {worst:.2e} of the largest average")


# ---- 9. CTC ----------------------------------------------------------------------------------------------------------------
def _ctc(ops, cases):
    rag = Ragged([c.logits.shape[0] for c in cases], ops.device)
    return scorer.ctc_loss_batch(ops, _t(np.concatenate([c.logits for c in cases])), rag, [c.ids for c in cases]).cpu().numpy()


def test_ctc_up_to_2048_targets(ops):
    cases = [lc.ctc_case(i) for i in range(len(lc.CTC_SHAPES))]
    batch = _ctc(ops, cases)
    worst = 0.0
    for (T, n), c, got in zip(lc.CTC_SHAPES, cases, batch):
        if T < n:
            assert got == 0.0 and c.ref32 == 0.0 and c.ref64 == 0.0, (T, n, got)  # infeasible: exactly 0
            continue
        for ref in (c.ref32, c.ref64):
            rel = abs(float(got) - ref) / abs(ref)
            worst = max(worst, rel)
            assert rel <= 1e-5, (T, n, float(got), ref)
    alone = np.array([_ctc(ops, [c])[0] for c in cases])
    assert np.array_equal(batch.view(np.uint32), alone.view(np.uint32)), "the batch differs from its utterances one by one"
    print(f"CTC, T up to 4200, n up to 2048: largest relative error against either float64 reference {worst:.2e}")


def test_ctc_refuses_2049_targets(ops):
    c = SimpleNamespace(logits=np.zeros((4, 145), dtype=np.float32), ids=np.zeros(capi.CTC_MAX_TARGETS + 1, dtype=np.int32))
    assert capi.CTC_MAX_TARGETS == 2048
    with pytest.raises(ValueError):
        _ctc(ops, [c])
