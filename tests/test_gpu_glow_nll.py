"""The scorer's glow loss on the MI355X (csrc/glow_forward.hip, tts_postflow_nll, TTSScorer.score(include_glow=True)): the row kernel
and the reduction against the float64 restatement (tests/glow_ref.py), the forward pass against the reference's float64 modules
(tests/golden/make_glow_golden.py) for the three checkpoint variants, the round trip through the synthesis direction with no golden
involved, a ragged batch against its utterances one by one, and the scorer end to end.

Largest deviations measured (DESIGN.md section 10 keeps them): printed by the tests that bound them."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, fixture_weights as fw, packing, scorer
from tests import glow_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
S = np.load(os.path.join(HERE, "golden", "scorer", "scorer.npz"))
G = np.load(os.path.join(HERE, "golden", "scorer", "glow.npz"))
VARIANTS = ["meta", "monolingual", "single"]
LID = int(S["tts_lang_id"])
BLOCK_ROWS, GRID_ROWS = capi.GLOW_FORWARD_BLOCK_ROWS, capi.GLOW_FORWARD_GRID_ROWS


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- kernel level ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks():
    """(wfwd, winv, an_bias, an_logs) float32 of the 18 fixture blocks."""
    sd = packing.fold_weight_norm(fw.acoustic_state_dict())
    out = []
    for b in range(18):
        pa, pn = f"post_flow.flows.{3 * b}.", f"post_flow.flows.{3 * b + 1}."
        out.append((packing.invconv_forward(sd, pn), packing.invconv_inverse(sd, pn), np.asarray(sd[pa + "bias"], dtype=np.float32).reshape(-1),
                    np.asarray(sd[pa + "logs"], dtype=np.float32).reshape(-1)))
    return out


def _rows_kernel(x, ld, ml=None, ld_ml=160, row_logdet=None, blk=None, row0=0, calls=1):
    """tts_glow_forward_rows on rows x [R, 160] placed at row ``row0`` of a buffer with row stride ld (and ml likewise, stride ld_ml) ->
    (x after, row_logdet after).  The buffers' other elements hold a sentinel, checked to be untouched."""
    lib = capi.lib()
    R = x.shape[0]
    SENT = np.float32(-12345.0)
    xb = np.full((row0 + R + 1, ld), SENT, dtype=np.float32)
    xb[row0:row0 + R, :160] = x
    xd = _dev(xb)
    mld = ldd = None
    if ml is not None:
        mb = np.full((row0 + R + 1, ld_ml), SENT, dtype=np.float32)
        mb[row0:row0 + R, :160] = ml
        mld = _dev(mb)
        ldb = np.full(row0 + R + 1, -777.0)
        ldb[row0:row0 + R] = 0.0 if row_logdet is None else row_logdet
        ldd = _dev(ldb, np.float64)
    w = ab = al = None
    if blk is not None:
        w, ab, al = _dev(blk[0]), _dev(blk[2]), _dev(blk[3])
    for _ in range(calls):
        capi.check(lib.tts_glow_forward_rows(C.c_void_p(xd.data_ptr() + 4 * row0 * ld), ld, R, None if mld is None else C.c_void_p(mld.data_ptr() + 4 * row0 * ld_ml),
                                             ld_ml, None if ldd is None else C.c_void_p(ldd.data_ptr() + 8 * row0), _ptr(w), _ptr(ab), _ptr(al), _stream()),
                   "tts_glow_forward_rows")
    got = xd.cpu().numpy()
    assert (got[:row0] == SENT).all() and (got[row0 + R:] == SENT).all() and (got[:, 160:] == SENT).all()
    ldg = None
    if ldd is not None:
        ldg = ldd.cpu().numpy()
        assert (ldg[:row0] == -777.0).all() and (ldg[row0 + R:] == -777.0).all()
        assert torch.equal(mld.cpu(), torch.from_numpy(mb))  # (the conv's output is read only)
        ldg = ldg[row0:row0 + R]
    return got[row0:row0 + R, :160], ldg


def _row_inputs(R, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-6.0, 2.0, size=(R, 160)).astype(np.float32)  # the range of a log-mel spectrogram
    # [m | logs]; logs with a mean, as a trained coupling's: a row's sum stays away from zero, where a relative bound means nothing
    ml = np.concatenate([rng.normal(0.0, 1.0, size=(R, 80)), rng.normal(-0.2, 0.3, size=(R, 80))], axis=1).astype(np.float32)
    return x, ml


@pytest.mark.parametrize("rows,ld,ld_ml", [(1, 160, 160), (3, 164, 160), (BLOCK_ROWS + 1, 161, 163), (BLOCK_ROWS + 1, 172, 168),
                                           (GRID_ROWS + 2 * BLOCK_ROWS + 5, 160, 160)])
def test_row_kernel_matches_float64(blocks, rows, ld, ld_ml):
    """Each half alone and both together; strides that allow 16-byte accesses (160, 164, 168, 172) and that do not (161, 163); one
    row, one wavefront's three rows, one row past a workgroup's, and more rows than the grid covers in one sweep.  The kernel rounds
    a float64 result once: every value within 1e-6 relative of the float64 restatement (the rounding alone is 6e-8)."""
    x, ml = _row_inputs(rows, seed=rows + ld)
    blk = blocks[5]
    worst = 0.0
    for use_ml, use_w in ((True, False), (False, True), (True, True)):
        got, ldg = _rows_kernel(x, ld, ml if use_ml else None, ld_ml, None, blk if use_w else None)
        want, ldw = gr.rows_forward(x, ml if use_ml else None, *((blk[0], blk[2], blk[3]) if use_w else (None, None, None)))
        err = np.abs(got - want) / np.abs(want)
        worst = max(worst, float(err.max()))
        assert (err <= 1e-6).all(), (use_ml, use_w, float(err.max()))
        if not use_w:
            assert np.array_equal(got[:, :80], x[:, :80])  # the coupling leaves x0 alone
        if use_ml:
            assert (np.abs(ldg - ldw) <= 1e-12 * np.abs(ldw)).all(), float((np.abs(ldg - ldw) / np.abs(ldw)).max())
    print(f"rows {rows}, strides {ld} / {ld_ml}: largest relative error against float64 {worst:.2e}")


def test_row_kernel_accumulates_the_logdet_in_fp64(blocks):
    """18 blocks add to one double per row: two calls on a row that starts at 1e6 keep the small addends."""
    x, ml = _row_inputs(7, seed=3)
    start = np.full(7, 1.0e6)
    _, ldg = _rows_kernel(x, 160, ml, 160, start, None, calls=2)
    want = start + 2.0 * ml[:, 80:].astype(np.float64).sum(axis=1)
    assert (np.abs(ldg - want) <= 1e-15 * np.abs(want) * 4).all()


def test_row_kernel_is_bit_identical_in_any_layout(blocks):
    """A row's result depends on the row alone: the same rows at another offset (other lanes, waves and workgroups), with other strides
    and in a sweep of the strided grid give the same bits."""
    R = 3 * BLOCK_ROWS + 2
    x, ml = _row_inputs(R, seed=9)
    a, la = _rows_kernel(x, 160, ml, 160, None, blocks[2])
    b, lb = _rows_kernel(x, 161, ml, 164, None, blocks[2], row0=7)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(la.view(np.uint64), lb.view(np.uint64))
    big_x, big_ml = _row_inputs(GRID_ROWS + R, seed=10)
    big_x[GRID_ROWS:], big_ml[GRID_ROWS:] = x, ml  # these rows: the grid's second sweep
    c, lc = _rows_kernel(big_x, 160, big_ml, 160, None, blocks[2])
    assert np.array_equal(a.view(np.uint32), c[GRID_ROWS:].view(np.uint32)) and np.array_equal(la.view(np.uint64), lc[GRID_ROWS:].view(np.uint64))


def test_forward_half_then_reverse_kernel_returns_the_input(blocks):
    """ActNorm and InvConvNear forward (this kernel), then tts_glow_invconv_actnorm with the stored inverse: every fixture block."""
    lib = capi.lib()
    rng = np.random.default_rng(4)
    x = rng.uniform(-6.0, 2.0, size=(BLOCK_ROWS + 1, 160)).astype(np.float32)
    worst = 0.0
    for blk in blocks:
        xd = _dev(x)
        w, winv, ab, al = (_dev(t) for t in blk)
        capi.check(lib.tts_glow_forward_rows(_ptr(xd), 160, x.shape[0], None, 0, None, _ptr(w), _ptr(ab), _ptr(al), _stream()), "tts_glow_forward_rows")
        capi.check(lib.tts_glow_invconv_actnorm(_ptr(xd), 160, x.shape[0], 160, _ptr(winv), _ptr(ab), _ptr(al), _stream()), "tts_glow_invconv_actnorm")
        worst = max(worst, float(np.abs(xd.cpu().numpy() - x).max()))
    print(f"kernel-level round trip, inputs in [-6, 2]: largest absolute error {worst:.2e}")
    assert worst <= 1e-5


def test_reduce_kernel_matches_float64():
    """Utterances of 0 (NaN), 1, 5 and 46 rows laid out with gaps, row stride 164; float32 parts for the utterances' rows only."""
    lib = capi.lib()
    rng = np.random.default_rng(6)
    begins, counts, frames = [0, 2, 4, 12], [0, 1, 5, 46], [1, 3, 10, 93]
    R = 60
    z = rng.normal(0.0, 2.0, size=(R, 160)).astype(np.float32)
    ld = rng.normal(-30.0, 5.0, size=R)
    const = -7.25
    zb = np.zeros((R, 164), dtype=np.float32)
    zb[:, :160] = z
    zd, ldd = _dev(zb), _dev(ld, np.float64)
    parts = torch.full((R, 2), -1.0, dtype=torch.float32, device=DEV)
    loss = torch.zeros(4, dtype=torch.float32, device=DEV)
    rb, nr, nf = (_dev(v, np.int32) for v in (begins, counts, frames))
    capi.check(lib.tts_glow_nll_reduce(_ptr(zd), 164, _ptr(ldd), _ptr(rb), _ptr(nr), _ptr(nf), 4, const, _ptr(loss), _ptr(parts), _stream()), "tts_glow_nll_reduce")
    loss, parts = loss.cpu().numpy(), parts.cpu().numpy()
    assert np.isnan(loss[0])
    touched = np.zeros(R, dtype=bool)
    for u in range(1, 4):
        sl = slice(begins[u], begins[u] + counts[u])
        touched[sl] = True
        want = gr.row_parts(z[sl], ld[sl], const)
        assert abs(loss[u] - gr.loss_from_parts(want, frames[u])) <= 1e-6 * abs(gr.loss_from_parts(want, frames[u])), u
        assert (np.abs(parts[sl] - want) <= 6e-8 * np.abs(want)).all(), u  # fp64 sums, rounded once to fp32
    assert (parts[~touched] == -1.0).all()


# ---- stage level -------------------------------------------------------------------------------------------------------------
def _write_checkpoints(d, variant_kw):
    model, emb = os.path.join(d, "model.pt"), os.path.join(d, "embedding_function.pt")
    t = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    torch.save({"model": t(fw.acoustic_state_dict(**variant_kw))}, model)
    torch.save({"style_emb_func": t(fw.style_state_dict())}, emb)
    return model, emb


@pytest.fixture(scope="module")
def scorers(tmp_path_factory):
    made = {}

    def get(variant):
        if variant not in made:
            model, emb = _write_checkpoints(str(tmp_path_factory.mktemp("ckpt_" + variant)), json.loads(str(S[f"tts_{variant}_fixture"])))
            made[variant] = scorer.TTSScorer(model, DEV, path_to_embedding_checkpoint=emb)
        return made[variant]
    return get


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("golden_corpus"))
    fw.write_fixture_corpus(d, **json.loads(str(S["tts_corpus"])))
    return d


@pytest.fixture(scope="module")
def items(corpus):
    return scorer.read_tts_cache(corpus)[1]


def _nll(tts, out, sentinel=None):
    """tts_postflow_nll on the handle state forward_batch left -> (loss [B], row parts [RF / 2, 2], z [RF / 2, 160]) numpy."""
    pipe = tts.pipe
    rs = out["rag_frame"].total_rows // 2
    B = out["rag_frame"].n_seq
    loss = torch.empty(B, dtype=torch.float32, device=pipe.device)
    parts = torch.full((rs, 2), 0.0 if sentinel is None else sentinel, dtype=torch.float32, device=pipe.device)
    z = torch.zeros(rs, 160, dtype=torch.float32, device=pipe.device)
    with torch.cuda.device(pipe.device):
        capi.check(pipe.lib.tts_postflow_nll(pipe.h, _ptr(out["gold"]), 80, _ptr(loss), _ptr(parts), _ptr(z), pipe._stream()), "tts_postflow_nll")
    return loss.cpu().numpy(), parts.cpu().numpy(), z


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.fixture(scope="module")
def alone(scorers, items):
    """variant -> the glow losses of the five fixture utterances, each scored alone (computed once)."""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = scorers(variant).score_items(items, LID, batch_size=1, include_glow=True)
        return cache[variant]
    return get


@pytest.mark.parametrize("variant", VARIANTS)
def test_glow_loss_matches_the_reference_in_float64(variant, alone, scorers, items):
    """The five fixture utterances, each alone, against the reference's float64 modules: 1e-4 relative, the bound test_gpu_scorer.py
    gives the l1 loss against the same kind of golden.  The four other losses stay what they are without the glow loss."""
    got = alone(variant).astype(np.float64)
    ref = G[f"glow_{variant}_f64"]
    rel = np.abs(got[:, 4] - ref) / np.abs(ref)
    print(f"{variant}: glow loss, largest relative error against float64 {rel.max():.2e} (the reference's fp32 run: "
          f"{(np.abs(G[f'glow_{variant}_ref'] - ref) / np.abs(ref)).max():.2e})")
    assert (rel <= 1e-4).all(), (got[:, 4], ref)
    four = scorers(variant).score_items(items, LID, batch_size=1)  # (another pass: to rounding order, as test_gpu_scorer.py compares passes)
    assert four.shape == (5, 4) and (np.abs(four - alone(variant)[:, :4]) <= 1e-5 * np.abs(four)).all()


def test_odd_frame_count_uses_46_rows_and_the_divisor_93(scorers, items, alone):
    tts = scorers("meta")
    assert items[0]["spec"].shape[0] == 93
    out = tts.forward_batch([items[0]], LID)
    loss, parts, _ = _nll(tts, out, sentinel=-5.0)
    assert parts.shape == (47, 2) and (parts[46] == -5.0).all() and (parts[:46] != -5.0).all()  # 94 frame rows, 46 live squeezed rows
    assert _rel(loss[0], alone("meta")[0, 4]) <= 1e-5  # (another pass)
    # float32 parts (6e-8 each) recombine to the loss with the divisors 160 * 46 and 80 * 93, and with no other frame count
    assert _rel(gr.loss_from_parts(parts[:46], 93), loss[0]) <= 1e-6
    assert _rel(gr.loss_from_parts(parts[:46], 92), loss[0]) > 2e-4 and _rel(gr.loss_from_parts(parts[:46], 94), loss[0]) > 2e-4
    assert _rel(loss[0], G["glow_meta_f64"][0]) <= 1e-4


def test_latent_and_row_parts_match_the_golden(scorers, items):
    """Utterance 0 of the multilingual variant: z against the float64 z (the bound of the mels in test_gpu_scorer.py), the row parts -
    the loss's summands, all of one sign in each column - within the loss's own 1e-4."""
    tts = scorers("meta")
    out = tts.forward_batch([items[0]], LID)
    _, parts, z = _nll(tts, out)
    z = z.cpu().numpy()[:46].reshape(92, 80)
    err = np.abs(z - G["glow_meta_z0"])
    rel = np.abs(parts[:46] - G["glow_meta_rows0"]) / np.abs(G["glow_meta_rows0"])
    print(f"z against float64: mean-abs {err.mean():.2e}, max-abs {err.max():.2e}; row parts, largest relative error {rel.max(axis=0)}")
    assert err.mean() < 1e-5
    assert (rel <= 1e-4).all()


def test_stage_round_trip_returns_the_gold_mels(scorers, items):
    """No golden involved: z_out of a ragged batch, fed to tts_postflow as z_noise on the same handle state, returns the gold mels on the
    frames the squeeze keeps.  Bound: ten times the reference's own fp32 round-trip error (its forward pass, then its inference
    direction): this is another fp32 order of the same 18 blocks."""
    tts = scorers("meta")
    pipe = tts.pipe
    out = tts.forward_batch(items, LID)
    _, _, z = _nll(tts, out)
    rf = out["rag_frame"].total_rows
    back = torch.empty(rf, 80, dtype=torch.float32, device=pipe.device)
    ld, ptr_mel = C.c_int32(), C.c_void_p()
    with torch.cuda.device(pipe.device):
        capi.check(pipe.lib.tts_postflow(pipe.h, _ptr(z), pipe._stream()), "tts_postflow")
        capi.check(pipe.lib.tts_copy_mel(pipe.h, _ptr(back), 80, pipe._stream()), "tts_copy_mel")
        capi.check(pipe.lib.tts_mel(pipe.h, C.byref(ptr_mel), C.byref(ld), None, None), "tts_mel")
        assert ld.value == 80
        # the synthesis direction has replaced the PostNet's mel: the likelihood pass needs tts_postnet again
        rc = pipe.lib.tts_postflow_nll(pipe.h, _ptr(out["gold"]), 80, _ptr(torch.empty(5, device=pipe.device)), None, None, pipe._stream())
        assert rc < 0 and "run tts_postnet first" in pipe.lib.tts_last_error().decode()
    back = back.cpu().numpy()
    worst = 0.0
    for it, b0 in zip(items, out["rag_frame"].begins):
        n = it["spec"].shape[0] // 2 * 2
        worst = max(worst, float(np.abs(back[b0:b0 + n] - it["spec"][:n]).max()))
    bound = 10.0 * float(G["glow_roundtrip_fp32"])
    print(f"stage-level round trip: largest absolute error {worst:.2e} (bound {bound:.2e}, the reference's own {float(G['glow_roundtrip_fp32']):.2e})")
    assert worst <= bound


def test_ragged_batch_matches_one_by_one(scorers, items, alone):
    many = scorers("meta").score_items(items, LID, batch_size=32, include_glow=True)
    one = alone("meta")
    rel = np.abs(many - one) / np.abs(one)
    print(f"ragged batch of five against one by one, largest relative difference per loss {rel.max(axis=0)}")
    assert (rel <= 1e-5).all(), (many, one)


def test_entry_refuses_before_the_postnet(tmp_path):
    model, emb = _write_checkpoints(str(tmp_path), json.loads(str(S["tts_single_fixture"])))
    tts = scorer.TTSScorer(model, DEV, path_to_embedding_checkpoint=emb)  # holds the forward weights; nothing has run
    x = torch.zeros(4, 80, device=tts.pipe.device)
    rc = tts.pipe.lib.tts_postflow_nll(tts.pipe.h, _ptr(x), 80, _ptr(x), None, None, tts.pipe._stream())
    assert rc < 0 and "run tts_postnet first" in tts.pipe.lib.tts_last_error().decode()


def test_scorer_end_to_end_with_the_glow_loss(scorers, corpus, items, alone, capsys):
    tts = scorers("meta")
    pipe = tts.pipe
    tts.score(corpus, lang_id="en", include_glow=True, keep_row_scores=True)
    paths = [it["filepath"] for it in items]
    assert list(tts.path_to_score) == paths and tts.nans == [] and list(tts.path_to_row_scores) == paths
    ref = np.concatenate([S["tts_meta_losses"], G["glow_meta_f64"][:, None]], axis=1)
    # per part: the golden bounds (1e-4 relative; 1e-6 absolute floor of the three prosody losses) + batch against alone (1e-5)
    bound = 1.1e-4 * np.abs(ref)
    bound[:, 1:4] = np.maximum(bound[:, 1:4], 1e-6 + 1e-5 * np.abs(ref[:, 1:4]))
    for k, p in enumerate(paths):
        parts = np.array(tts.path_to_parts[p])
        assert parts.shape == (5,) and (np.abs(parts - ref[k]) <= bound[k]).all(), (k, parts, ref[k])
        five = np.float32(parts[0]) + np.float32(parts[1]) + np.float32(parts[2]) + np.float32(parts[3]) + np.float32(parts[4])
        assert tts.path_to_score[p] == float(five)
        assert abs(tts.path_to_score[p] - ref[k].sum()) <= bound[k].sum() + 1e-6 * ref[k].sum()
        rows, T = tts.path_to_row_scores[p], items[k]["spec"].shape[0]
        assert rows.dtype == np.float32 and rows.shape == (T // 2, 2)
        assert _rel(gr.loss_from_parts(rows, T), parts[4]) <= 1e-6  # the row scores recombine to the loss
    # the defaults on the same object: four losses, as before
    tts.score(corpus, lang_id="en")
    assert list(tts.path_to_score) == paths and tts.path_to_row_scores == {}
    for k in (0, 2, 4):
        four = tts.forward_batch([items[k]], LID)["losses"].cpu().numpy()[0]
        want = np.float32(four[0]) + np.float32(four[1]) + np.float32(four[2]) + np.float32(four[3])
        assert abs(tts.path_to_score[paths[k]] - want) <= 1e-5 * abs(want), (k, tts.path_to_score[paths[k]], want)
        assert len(tts.path_to_parts[paths[k]]) == 4
    # the likelihood pass leaves the handle's mel alone: the PostNet output, row stride 272, the same bytes at the same address
    out = tts.forward_batch(items, LID)
    rf = out["rag_frame"].total_rows
    mel = lambda: (torch.empty(rf, 80, dtype=torch.float32, device=pipe.device), C.c_void_p(), C.c_int32())
    (m0, p0, l0), (m1, p1, l1) = mel(), mel()
    with torch.cuda.device(pipe.device):
        capi.check(pipe.lib.tts_mel(pipe.h, C.byref(p0), C.byref(l0), None, None), "tts_mel")
        capi.check(pipe.lib.tts_copy_mel(pipe.h, _ptr(m0), 80, pipe._stream()), "tts_copy_mel")
        claimed = pipe.workspace_claimed()
        _nll(tts, out)
        capi.check(pipe.lib.tts_mel(pipe.h, C.byref(p1), C.byref(l1), None, None), "tts_mel")
        capi.check(pipe.lib.tts_copy_mel(pipe.h, _ptr(m1), 80, pipe._stream()), "tts_copy_mel")
    assert l0.value == l1.value == 272 and p0.value == p1.value and torch.equal(m0, m1)
    assert pipe.workspace_claimed() == claimed  # (its scratch was reserved by the passes above: nothing grows on a repeat)
    tts.show_samples_with_highest_loss(2)
    assert "Loss:" in capsys.readouterr().out
