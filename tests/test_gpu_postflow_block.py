"""The PostFlow's one-launch WaveNet block (csrc/wavenet.hip, wavenet_block_kernel: the start conv and the four layers of a coupling
block with the hidden state and the skip sum kept on chip, 48 stored rows per workgroup plus 8 recomputed rows a side).

(1) The whole PostFlow stage through the native handle against the Python sequencer (engine.py: one tts_wavenet_layer launch per
    layer, with the same weights), torch.equal, bf16 and fp16.  Squeezed lengths: utterances shorter than the halo (1, 2, 7), one
    just past it (9), an utterance end on the 48-row tile boundary and one row to either side (47, 48, 49), the same around the 64
    computed rows (63, 64, 65), and three tiles (130).  The utterances are adjacent in the packed layout, so every tile's halo
    reaches into its neighbours' rows.
(2) Batch independence: each utterance alone gives the bits it has in the batch.
(3) CPU: the 48-row tile table covers every row exactly once.
"""
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import engine, fixture_weights as fw, native, synthetic as syn
from ims_toucan_prosody_variance_amd.ragged import Ragged

DEV = "cuda:0"
SQUEEZED = [1, 2, 7, 9, 47, 48, 49, 63, 64, 65, 130]
TILE, HALO, COMPUTED = 48, 8, 64


def test_tile_table_of_the_block_covers_every_row_exactly_once():
    rag = Ragged(SQUEEZED, "cpu")
    tiles, n = rag.tiles(TILE)
    assert n == sum((s + TILE - 1) // TILE for s in SQUEEZED)
    hits = torch.zeros(rag.total_rows, dtype=torch.int32)
    for row0, sb, se, u in tiles.tolist():
        assert (sb, se) == (rag.begins[u], rag.begins[u] + rag.lengths[u]) and sb <= row0 < se and (row0 - sb) % TILE == 0
        stored = range(row0, min(row0 + TILE, se))
        computed = range(row0 - HALO, row0 - HALO + COMPUTED)
        assert stored[0] - computed[0] == HALO and computed[-1] - (row0 + TILE - 1) == HALO  # four 5-tap layers either side
        hits[stored[0]:stored[-1] + 1] += 1
    assert (hits == 1).all()


@pytest.fixture(scope="module")
def batch():
    """Utterances of two phonemes with gold durations (1, T - 1), T = twice the squeezed length."""
    Ts = [2 * s for s in SQUEEZED]
    texts = [torch.from_numpy(syn.utterance_features(70 + u, 2, word_boundaries=False)) for u in range(len(Ts))]
    embs = torch.stack([torch.from_numpy(syn.utterance_embedding(70 + u)) for u in range(len(Ts))])
    durs = [torch.tensor([1, T - 1], dtype=torch.int32) for T in Ts]
    zs = [torch.from_numpy(syn.postflow_noise(70 + u, T)) for u, T in enumerate(Ts)]
    return dict(Ts=Ts, texts=texts, embs=embs, durs=durs, zs=zs, langs=[syn.LANG_EN] * len(Ts), sd=fw.acoustic_state_dict())


@pytest.fixture(scope="module")
def stage(batch):
    """Sequencer and native results of the batch, once per precision."""
    cache = {}

    def get(precision):
        if precision not in cache:
            b = batch
            ref = engine.AcousticEngine(b["sd"], DEV, precision=precision).forward(b["texts"], b["embs"], b["langs"], durations=b["durs"], z_noise=b["zs"])
            pipe = native.NativePipeline(b["sd"], None, None, DEV, precision=precision)
            out = pipe.forward(b["texts"], b["embs"], b["langs"], durations=b["durs"], z_noise=b["zs"])
            torch.cuda.synchronize()
            cache[precision] = ({"mel": [m.clone() for m in ref["mel"]]}, pipe, {"mel": [m.clone() for m in out["mel"]]})
        return cache[precision]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_postflow_stage_equals_the_python_sequencer(batch, stage, precision):
    ref, _, out = stage(precision)
    for u, T in enumerate(batch["Ts"]):
        assert tuple(out["mel"][u].shape) == (T, 80)
        assert torch.isfinite(out["mel"][u]).all()
        assert torch.equal(out["mel"][u], ref["mel"][u]), f"utterance {u} ({T // 2} squeezed rows): mel differs from the Python sequencer"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_each_utterance_alone_has_the_bits_it_has_in_the_batch(batch, stage, precision):
    b = batch
    _, pipe, out = stage(precision)
    for u in range(len(b["Ts"])):
        one = pipe.forward([b["texts"][u]], b["embs"][u:u + 1], b["langs"][u:u + 1], durations=[b["durs"][u]], z_noise=[b["zs"][u]])
        assert torch.equal(one["mel"][0], out["mel"][u]), f"utterance {u}: alone it differs from its rows in the batch"
