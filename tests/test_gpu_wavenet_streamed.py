"""The barrier-free WaveNet layer (csrc/wavenet.hip) on a real MI355X:
(1) the stage API's PostFlow - fused layers that compute their conditioning columns themselves - against the Python sequencer
    (engine.py: stand-alone cond convs + tts_wavenet_layer), bit for bit, on one ragged batch and utterance by utterance;
(2) the public tts_wavenet_layer against the numpy ABI emulator, incl. that nothing is stored outside an utterance;
(3) the workspace bound of a 16-bit handle, which no longer holds the [RS, 1536] conditioning buffer.
Squeezed lengths cover a single row, less than the 5-tap halo, and both sides of a 32-frame block and of a 64-frame tile."""
import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, fixture_weights as fw, native, packing, synthetic as syn
from ims_toucan_prosody_variance_amd.ragged import Ragged
from tests import abi_emulator

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SQUEEZED = [1, 2, 3, 31, 33, 63, 64, 65, 129, 193]
# tts_workspace_bytes(32, 128, 640) of an acoustic-only 16-bit handle before the cond buffer left the frame arena
PARENT_WORKSPACE_BYTES = 837362816


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def batch():
    """Ten utterances of two phonemes with gold durations (1, T - 1); T = twice the squeezed length, and once 2 * 3 + 1: the flow
    drops that utterance's last frame."""
    Ts = [2 * s for s in SQUEEZED]
    Ts[2] += 1
    texts = [torch.from_numpy(syn.utterance_features(40 + u, 2, word_boundaries=False)) for u in range(len(Ts))]
    embs = torch.stack([torch.from_numpy(syn.utterance_embedding(40 + u)) for u in range(len(Ts))])
    durs = [torch.tensor([1, T - 1], dtype=torch.int32) for T in Ts]
    zs = [torch.from_numpy(syn.postflow_noise(40 + u, T)) for u, T in enumerate(Ts)]
    return dict(Ts=Ts, texts=texts, embs=embs, durs=durs, zs=zs, langs=[syn.LANG_EN] * len(Ts), sd=fw.acoustic_state_dict())


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_stage_api_postflow_equals_the_python_sequencer_and_does_not_depend_on_the_batch(batch, precision):
    b = batch
    ref = engine.AcousticEngine(b["sd"], DEV, precision=precision).forward(b["texts"], b["embs"], b["langs"], durations=b["durs"], z_noise=b["zs"])
    pipe = native.NativePipeline(b["sd"], None, None, DEV, precision=precision)
    out = pipe.forward(b["texts"], b["embs"], b["langs"], durations=b["durs"], z_noise=b["zs"])
    torch.cuda.synchronize()
    for u, T in enumerate(b["Ts"]):
        assert tuple(out["mel"][u].shape) == (T // 2 * 2, 80)
        assert torch.isfinite(out["mel"][u]).all()
        assert torch.equal(out["mel"][u], ref["mel"][u]), f"utterance {u} ({T} frames): mel differs from the Python sequencer"
    for u in range(len(b["Ts"])):
        one = pipe.forward([b["texts"][u]], b["embs"][u:u + 1], b["langs"][u:u + 1], durations=[b["durs"][u]], z_noise=[b["zs"][u]])
        assert torch.equal(one["mel"][0], out["mel"][u]), f"utterance {u}: alone it differs from its rows in the batch"


@pytest.fixture(scope="module")
def layer_reference():
    """Emulator results, once per (compute, cout2)."""
    cpu = engine.Ops("cpu", lib=abi_emulator.Emulator())
    cache = {}

    def get(compute, cout2):
        if (compute, cout2) not in cache:
            cache[(compute, cout2)] = _run_layer(cpu, lambda t: t.clone().contiguous(), compute, cout2)
        return cache[(compute, cout2)]

    return get


SENTINEL = 12345.0
PACK16 = {capi.COMPUTE_BF16: "bf16", capi.COMPUTE_F16: "f16"}
TOL = {capi.COMPUTE_BF16: 2e-2, capi.COMPUTE_F16: 3e-3}  # of tests/test_gpu_kernels.py::test_fused_wavenet_layer: same emulator, same rounding points


def _run_layer(ops, to, compute, cout2):
    H = 192
    w_in = rnd(2 * H, H, 5, seed=1, scale=1.0 / np.sqrt(5 * H)).numpy()
    b_in = rnd(2 * H, seed=2, scale=0.1).numpy()
    w_rs = rnd(cout2, H, 1, seed=3, scale=1.0 / np.sqrt(H)).numpy()
    b_rs = rnd(cout2, seed=4, scale=0.1).numpy()
    rag = Ragged(SQUEEZED, ops.device, align=2)
    R = rag.total_rows
    inl = packing.pack_conv(w_in, b_in, ops.device, mode=capi.MODE_GATED, bf16=PACK16[compute])
    rs = packing.pack_conv(w_rs, b_rs, ops.device, bf16=PACK16[compute])
    hs = to(rnd(R, 2 * H, seed=5))
    cond = to(rnd(R, 8 * H, seed=6, scale=0.5))[:, 2 * H:4 * H]  # a 384-column slice of a [R, 1536] conditioning
    out = to(torch.full((R, 2 * H), SENTINEL))
    ops.wavenet_layer(inl, rs, hs, out, cond, rag)
    return out


@pytest.mark.parametrize("compute", [capi.COMPUTE_BF16, capi.COMPUTE_F16])
@pytest.mark.parametrize("cout2", [384, 192])
def test_public_wavenet_layer_matches_the_emulator_and_stores_nothing_outside_an_utterance(layer_reference, compute, cout2):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    gpu = engine.Ops(DEV)
    assert not isinstance(gpu.lib, abi_emulator.Emulator)
    g = _run_layer(gpu, lambda t: t.to(DEV).contiguous(), compute, cout2).cpu()
    torch.cuda.synchronize()
    c = layer_reference(compute, cout2)
    rag = Ragged(SQUEEZED, "cpu", align=2)
    live = torch.zeros(rag.total_rows, dtype=torch.bool)
    for b0, n in zip(rag.begins, rag.lengths):
        live[b0:b0 + n] = True
    assert int((~live).sum()) == sum(n % 2 for n in SQUEEZED)  # the alignment rows behind odd lengths
    cols = slice(0, 384) if cout2 == 384 else slice(192, 384)
    a, r = g[live][:, cols].numpy(), c[live][:, cols].numpy()
    scale = max(1.0, float(np.abs(r).max()))
    err = float(np.abs(a - r).max())
    print(f"compute {compute} cout2 {cout2}: max abs err {err:.3e}, bound {TOL[compute] * scale:.3e}")
    assert err <= TOL[compute] * scale
    assert (g[~live] == SENTINEL).all(), "rows outside every utterance were written"
    if cout2 == 192:
        assert (g[:, :192] == SENTINEL).all(), "the last layer writes the skip half only"


def test_workspace_bound_of_a_16_bit_handle_is_not_larger_than_before():
    pipe = native.NativePipeline(fw.acoustic_state_dict(), None, None, DEV, precision="bf16")
    now = pipe.workspace_bytes(32, 128, 640)
    print(f"tts_workspace_bytes(32, 128, 640): {now} (before: {PARENT_WORKSPACE_BYTES})")
    assert 0 < now <= PARENT_WORKSPACE_BYTES
