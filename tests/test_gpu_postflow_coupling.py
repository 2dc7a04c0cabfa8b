"""The PostFlow's coupling block as one launch (csrc/wavenet.hip, wavenet_block_kernel: after the four WaveNet layers the same
workgroup runs the end conv with the coupling, the inverse 1x1 conv and ActNorm on the skip sum it still holds, and writes the new
x into a second buffer - 18 launches per pass, x ping-ponging between two buffers, block 17 reading the caller's noise directly).

(1) Ping-pong against the halo: squeezed lengths with interior tiles on both sides of a 48-row tile boundary (96, 97, 144, 145, 200)
    and the degenerate ends (1, 8, 9), adjacent in the packed layout; mel torch.equal to the Python sequencer (engine.py: the unfused
    launches), bf16 and fp16.  An interior tile's halo rows are rewritten by two other workgroups of the same launch.
(2) Odd frame counts: the squeezed row behind such an utterance holds its dropped last frame and the pad frame.  It lies in no tile,
    but tts_copy_mel copies it out (mel_packed), so it is observable: the kernel passes it through the inverse 1x1 conv and ActNorm
    of every block, as glow_invconv_actnorm did when it ran over all rows.  mel and the whole mel_packed equal the sequencer's.
(3) One handle, changing batches: long, shorter, long again - each equal to a fresh handle's result; a repeated forward is equal.
(4) z_noise is an input: unchanged by the pass.
(5) Each utterance alone has the bits it has in the batch.
(6) CPU: the 48-row tiles cover every squeezed row of every utterance exactly once, and the rows of the squeezed layout outside all
    tiles are exactly the rows behind the utterances with an odd frame count (none for even counts) - the rows the kernel's extra
    workgroups handle.
(7) The workspace bound does not grow: tts_workspace_bytes(B = 4, 128 phonemes, 640 frames) against the value of the commit before
    this kernel (0d04230, acoustic handle without a vocoder; the bound does not depend on which 16-bit format).
"""
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import engine, fixture_weights as fw, native, synthetic as syn
from ims_toucan_prosody_variance_amd.ragged import Ragged

DEV = "cuda:0"
SQUEEZED = [1, 8, 9, 96, 97, 144, 145, 200]
EVEN_T = [2 * s for s in SQUEEZED]
ODD_T = [17, 40, 97, 291]  # squeezed 8, 20, 48, 145: a pad row behind the first, the third (on a tile boundary) and the last
SHORT = slice(0, 3)        # the shorter batch of (3): the first three utterances of EVEN_T
TILE = 48
PARENT_WORKSPACE_BYTES = 154949840  # tts_workspace_bytes(4, 128, 640) of 0d04230, bf16 and f16 alike


def _make(Ts, seed):
    n = len(Ts)
    return dict(Ts=Ts, texts=[torch.from_numpy(syn.utterance_features(seed + u, 2, word_boundaries=False)) for u in range(n)],
                embs=torch.stack([torch.from_numpy(syn.utterance_embedding(seed + u)) for u in range(n)]),
                durs=[torch.tensor([1, T - 1], dtype=torch.int32) for T in Ts],
                zs=[torch.from_numpy(syn.postflow_noise(seed + u, T)) for u, T in enumerate(Ts)], langs=[syn.LANG_EN] * n)


def _run(model, b, sel=None, **kw):
    sel = slice(None) if sel is None else sel
    return model.forward(b["texts"][sel], b["embs"][sel], b["langs"][sel], durations=b["durs"][sel], z_noise=b["zs"][sel], **kw)


def _keep(out):
    return {"mel": [m.clone() for m in out["mel"]], "mel_packed": out["mel_packed"].clone()}


def _outside_tiles(Ts):
    """(rows of the squeezed layout in no 48-row tile, rows behind utterances with an odd frame count, hits per row)"""
    rag_f = Ragged(Ts, "cpu", align=2)
    rag_s = rag_f.halved()
    RS = rag_f.total_rows // 2
    hits = torch.zeros(RS, dtype=torch.int32)
    tiles, n = rag_s.tiles(TILE)
    assert n == sum((T // 2 + TILE - 1) // TILE for T in Ts)
    for row0, sb, se, u in tiles.tolist():
        assert (sb, se) == (rag_s.begins[u], rag_s.begins[u] + rag_s.lengths[u]) and sb <= row0 < se and (row0 - sb) % TILE == 0
        hits[row0:min(row0 + TILE, se)] += 1
    outside = [r for r in range(RS) if hits[r] == 0]
    pad = [b + n for b, n, T in zip(rag_s.begins, rag_s.lengths, Ts) if T % 2]
    return outside, pad, hits


def test_tiles_cover_every_utterance_row_once_and_only_pad_rows_lie_outside():
    outside, pad, hits = _outside_tiles(EVEN_T)
    assert outside == [] and pad == [] and (hits == 1).all()
    outside, pad, hits = _outside_tiles(ODD_T)
    assert outside == pad and len(pad) == sum(T % 2 for T in ODD_T) and int(hits.max()) == 1
    rag_s = Ragged(ODD_T, "cpu", align=2).halved()
    for b, n in zip(rag_s.begins, rag_s.lengths):
        assert (hits[b:b + n] == 1).all()


@pytest.fixture(scope="module")
def batches():
    return {"even": _make(EVEN_T, 170), "odd": _make(ODD_T, 190), "sd": fw.acoustic_state_dict()}


@pytest.fixture(scope="module")
def stage(batches):
    """Per precision: the sequencer's and a fresh native handle's results of both batches (the native handle is kept: it has run the
    even batch, then the odd one)."""
    cache = {}

    def get(precision):
        if precision not in cache:
            eng = engine.AcousticEngine(batches["sd"], DEV, precision=precision)
            ref = {k: _keep(_run(eng, batches[k])) for k in ("even", "odd")}
            pipe = native.NativePipeline(batches["sd"], None, None, DEV, precision=precision)
            out = {"even": _keep(_run(pipe, batches["even"]))}
            odd_fresh = native.NativePipeline(batches["sd"], None, None, DEV, precision=precision)
            out["odd"] = _keep(_run(odd_fresh, batches["odd"]))
            torch.cuda.synchronize()
            cache[precision] = (ref, pipe, out)
        return cache[precision]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_ping_pong_against_the_halo_equals_the_python_sequencer(batches, stage, precision):
    ref, _, out = stage(precision)
    for u, T in enumerate(EVEN_T):
        assert tuple(out["even"]["mel"][u].shape) == (T, 80)
        assert torch.isfinite(out["even"]["mel"][u]).all()
        assert torch.equal(out["even"]["mel"][u], ref["even"]["mel"][u]), f"utterance {u} ({T // 2} squeezed rows): mel differs from the Python sequencer"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_odd_frame_counts_and_the_rows_behind_them(batches, stage, precision):
    ref, _, out = stage(precision)
    for u, T in enumerate(ODD_T):
        assert tuple(out["odd"]["mel"][u].shape) == (T // 2 * 2, 80)
        assert torch.equal(out["odd"]["mel"][u], ref["odd"]["mel"][u]), f"utterance {u} ({T} frames): mel differs from the Python sequencer"
    # the packed tensor the handle copies out includes the rows behind the odd utterances: the sequencer's bits there too
    assert out["odd"]["mel_packed"].shape == ref["odd"]["mel_packed"].shape
    assert torch.isfinite(out["odd"]["mel_packed"]).all()
    assert torch.equal(out["odd"]["mel_packed"], ref["odd"]["mel_packed"])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_same_handle_changing_batches(batches, stage, precision):
    _, pipe, out = stage(precision)
    fresh_short = _keep(_run(native.NativePipeline(batches["sd"], None, None, DEV, precision=precision), batches["even"], SHORT))
    long1 = _keep(_run(pipe, batches["even"]))
    short = _keep(_run(pipe, batches["even"], SHORT))
    odd = _keep(_run(pipe, batches["odd"]))
    long2 = _keep(_run(pipe, batches["even"]))
    long3 = _keep(_run(pipe, batches["even"]))
    for got, want, what in ((long1, out["even"], "long"), (short, fresh_short, "shorter"), (odd, out["odd"], "odd"), (long2, out["even"], "long again"),
                            (long3, long2, "repeated")):
        assert len(got["mel"]) == len(want["mel"])
        for u, (a, b) in enumerate(zip(got["mel"], want["mel"])):
            assert torch.equal(a, b), f"{what} batch, utterance {u}: differs from a fresh handle's result"
        assert torch.equal(got["mel_packed"], want["mel_packed"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_z_noise_is_an_input(batches, stage, precision):
    _, pipe, out = stage(precision)
    b = batches["odd"]
    z_sq = pipe.squeeze_noise(b["zs"], b["Ts"])
    keep = z_sq.clone()
    got = pipe.forward(b["texts"], b["embs"], b["langs"], durations=b["durs"], z_sq=z_sq)
    torch.cuda.synchronize()
    assert torch.equal(z_sq, keep), "tts_postflow wrote into z_noise"
    assert torch.equal(got["mel_packed"], out["odd"]["mel_packed"])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_each_utterance_alone_has_the_bits_it_has_in_the_batch(batches, stage, precision):
    _, pipe, out = stage(precision)
    for u in range(len(EVEN_T)):
        one = _run(pipe, batches["even"], slice(u, u + 1))
        assert torch.equal(one["mel"][0], out["even"]["mel"][u]), f"utterance {u}: alone it differs from its rows in the batch"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_workspace_bound_does_not_grow(stage, precision):
    _, pipe, _ = stage(precision)
    now = pipe.workspace_bytes(4, 128, 640)
    print(f"tts_workspace_bytes(4, 128, 640), {precision}: {now} (before: {PARENT_WORKSPACE_BYTES})")
    assert 0 < now <= PARENT_WORKSPACE_BYTES
