"""The decoder's fused Conformer launches of the native pipeline (csrc/conformer_conv.hip, 16-bit configurations): the convolution
module as one launch (conformer_conv_kernel: 128 computed rows per workgroup, of which 98 are stored and 15 a side are the halo of
the 31-tap depthwise conv) and LayerNorm inside the q | k | v projection (ln_linear_kernel, 128-row tiles).  The encoder (7 taps)
keeps the stand-alone launches: both fused forms gave its bits too but measured slower there.

(1) The acoustic model through the native handle against the Python sequencer (engine.py: tts_layernorm, tts_conv1d,
    tts_dwconv_swish one launch each, same weights), torch.equal on mel, pitch, energy and durations, bf16 and fp16, on two ragged
    batches of adjacent utterances:
      * "enc": many phonemes with gold durations of one frame each, so encoder and decoder see the same lengths - 1, 2, 3, 4, 7,
        121, 122, 123, 125, 126 (around the 128-row tile of ln_linear and past the first 98-row tile by 23 .. 28 rows: the second
        tile's halo reaches the utterance end), 245 and 300 (three and four 98-row tiles).  The whole model, PostFlow included;
      * "dec": frames set through gold durations (one phoneme for the single frame, else two phonemes with (1, T - 1)): shorter
        than the halo (1, 2, 15), just past it (16, 31), around the 98-row tile (97, 98, 99), 98 + 15 and 98 + 16 (113, 114), two
        tiles and one row (197), three tiles (250).  Seven of them are odd: the 2-aligned frame layout then has a gap row, which
        the fused module must neither read nor write.  This batch runs without the PostFlow, whose squeeze drops an odd last
        frame: the mel is then the decoder's (and PostNet's) own output and shows every decoder row.
(2) Batch independence: each utterance alone gives the bits it has in the batch.
(3) CPU: the 98-row tile table covers every row of every utterance of both batches' frame layouts exactly once, and stored rows
    plus halo are the 128 computed rows.
"""
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import engine, fixture_weights as fw, native, synthetic as syn
from ims_toucan_prosody_variance_amd.ragged import Ragged

DEV = "cuda:0"
COMPUTED = 128
TRD, HD = 98, 15    # decoder: stored rows per tile, halo (kernel 31)
ENC_LENGTHS = [1, 2, 3, 4, 7, 121, 122, 123, 125, 126, 245, 300]
DEC_LENGTHS = [1, 2, 15, 16, 31, TRD - 1, TRD, TRD + 1, TRD + 15, TRD + 16, 2 * TRD + 1, 250]
KEYS = ("mel", "pitch", "energy", "durations")


@pytest.mark.parametrize("lengths,align,tile,halo", [(DEC_LENGTHS, 2, TRD, HD), (ENC_LENGTHS, 2, TRD, HD)])
def test_tile_tables_of_the_fused_module_cover_every_row_exactly_once(lengths, align, tile, halo):
    assert tile + 2 * halo == COMPUTED
    rag = Ragged(lengths, "cpu", align=align)
    tiles, n = rag.tiles(tile)
    assert n == sum((s + tile - 1) // tile for s in lengths)
    hits = torch.zeros(rag.total_rows, dtype=torch.int32)
    for row0, sb, se, u in tiles.tolist():
        assert (sb, se) == (rag.begins[u], rag.begins[u] + rag.lengths[u]) and sb <= row0 < se and (row0 - sb) % tile == 0
        stored = range(row0, min(row0 + tile, se))
        computed = range(row0 - halo, row0 - halo + COMPUTED)
        assert stored[0] - computed[0] == halo and computed[-1] - (row0 + tile - 1) == halo  # (K - 1) / 2 taps either side
        hits[stored[0]:stored[-1] + 1] += 1
    live = torch.zeros(rag.total_rows, dtype=torch.bool)
    for b, s in zip(rag.begins, rag.lengths):
        live[b:b + s] = True
    assert (hits[live] == 1).all() and (hits[~live] == 0).all()


def test_the_decoder_batch_has_gap_rows():
    assert sum(T % 2 for T in DEC_LENGTHS) >= 3
    rag = Ragged(DEC_LENGTHS, "cpu", align=2)
    assert rag.total_rows > sum(DEC_LENGTHS)


def _batch(kind):
    if kind == "enc":
        Ls = ENC_LENGTHS
        durs = [torch.ones(L, dtype=torch.int32) for L in Ls]
    else:
        Ls = [1 if T == 1 else 2 for T in DEC_LENGTHS]
        durs = [torch.tensor([1] if T == 1 else [1, T - 1], dtype=torch.int32) for T in DEC_LENGTHS]
    Ts = [int(d.sum()) for d in durs]
    texts = [torch.from_numpy(syn.utterance_features(90 + u, L, word_boundaries=False)) for u, L in enumerate(Ls)]
    embs = torch.stack([torch.from_numpy(syn.utterance_embedding(90 + u)) for u in range(len(Ls))])
    zs = [torch.from_numpy(syn.postflow_noise(90 + u, T)) for u, T in enumerate(Ts)]
    return dict(Ls=Ls, Ts=Ts, texts=texts, embs=embs, durs=durs, zs=zs, langs=[syn.LANG_EN] * len(Ls), postflow=kind == "enc")


def _forward(model, b, sel=None):
    pick = (lambda x: x) if sel is None else (lambda x: x[sel:sel + 1])
    return model.forward(pick(b["texts"]), pick(b["embs"]), pick(b["langs"]), durations=pick(b["durs"]), z_noise=pick(b["zs"]) if b["postflow"] else None,
                         run_postflow=b["postflow"])


@pytest.fixture(scope="module")
def stage():
    """Sequencer and native results of a batch, once per (batch, precision)."""
    sd = fw.acoustic_state_dict()
    batches, pipes, cache = {}, {}, {}

    def get(kind, precision):
        if kind not in batches:
            batches[kind] = _batch(kind)
        b = batches[kind]
        if (kind, precision) not in cache:
            ref = _forward(engine.AcousticEngine(sd, DEV, precision=precision), b)
            if precision not in pipes:
                pipes[precision] = native.NativePipeline(sd, None, None, DEV, precision=precision)
            out = _forward(pipes[precision], b)
            torch.cuda.synchronize()
            cache[(kind, precision)] = ({k: [t.clone() for t in ref[k]] for k in KEYS}, {k: [t.clone() for t in out[k]] for k in KEYS})
        return b, pipes[precision], cache[(kind, precision)]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["enc", "dec"])
def test_fused_conformer_equals_the_python_sequencer(stage, kind, precision):
    b, _, (ref, out) = stage(kind, precision)
    for u, (L, T) in enumerate(zip(b["Ls"], b["Ts"])):
        frames = T - T % 2 if b["postflow"] else T  # (the PostFlow's squeeze drops an odd last frame)
        assert tuple(out["mel"][u].shape) == (frames, 80)
        for k in KEYS:
            assert out[k][u].shape[0] == (frames if k == "mel" else L)
            assert torch.isfinite(out[k][u].float()).all(), f"utterance {u} ({L} phonemes, {T} frames): {k} is not finite"
            assert torch.equal(out[k][u], ref[k][u]), f"utterance {u} ({L} phonemes, {T} frames): {k} differs from the Python sequencer"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["enc", "dec"])
def test_each_utterance_alone_has_the_bits_it_has_in_the_batch(stage, kind, precision):
    b, pipe, (_, out) = stage(kind, precision)
    for u in range(len(b["Ls"])):
        one = _forward(pipe, b, u)
        for k in KEYS:
            assert torch.equal(one[k][0], out[k][u]), f"utterance {u}: alone its {k} differs from its rows in the batch"
