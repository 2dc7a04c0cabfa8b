"""Micro-benchmark of tts_wavenet_layer vs the two-launch form at the bench shape (32 utterances x 320 squeezed frames).
`--block [batch]`: the one-launch coupling block of the native PostFlow (wavenet_block: start conv, four layers, end conv with the
coupling, inverse 1x1 conv and ActNorm) instead, timed alone by the stage profiler (HIP events around each of its 18 launches
inside tts_postflow, which in the 16-bit configurations launches nothing else per block)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, engine, packing
from ims_toucan_prosody_variance_amd.ragged import Ragged


def block(B):
    """wavenet_block (the whole coupling block) inside tts_postflow: B utterances of 128 phonemes x 5 frames (320 squeezed rows each), bf16, fixture weights."""
    from ims_toucan_prosody_variance_amd import fixture_weights as fw, native, synthetic as syn
    dev = torch.device("cuda:0")
    pipe = native.NativePipeline(fw.acoustic_state_dict(), None, None, dev, precision="bf16")
    L = 128
    texts = [torch.from_numpy(syn.utterance_features(i, L, word_boundaries=False)).to(dev) for i in range(B)]
    embs = torch.stack([torch.from_numpy(syn.utterance_embedding(i)) for i in range(B)]).to(dev)
    durs = [torch.full((L,), 5, dtype=torch.int32, device=dev) for _ in range(B)]
    zs = [torch.from_numpy(syn.postflow_noise(i, 5 * L)).to(dev) for i in range(B)]
    packed = pipe.pack_inputs(texts, embs, [syn.LANG_EN] * B, durations=durs)
    z_sq = pipe.squeeze_noise(zs, [5 * L] * B)
    for _ in range(3):
        pipe.forward(None, None, packed=packed, z_sq=z_sq)
    torch.cuda.synchronize()
    pipe.profile(1, "wavenet_block")
    reps = 10
    for _ in range(reps):
        pipe.forward(None, None, packed=packed, z_sq=z_sq)
    torch.cuda.synchronize()
    s = pipe.profile_summary()["wavenet_block"]
    pipe.profile(0)
    print(f"rows {B * 320}: wavenet_block {s['avg_us']:.1f} us per launch over {s['launches']} launches "
          f"({18 * s['avg_us'] / 1e3:.3f} ms per pass, {s['tflops']:.0f} TFLOP/s algorithmic)")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--block":
        return block(int(sys.argv[2]) if len(sys.argv) > 2 else 32)
    dev = torch.device("cuda:0")
    ops = engine.Ops(dev)
    B, T, H = int(sys.argv[1]) if len(sys.argv) > 1 else 32, 320, 192
    rag = Ragged([T] * B, dev)
    R = rag.total_rows
    rs = np.random.RandomState(0)
    inl = packing.pack_conv((rs.randn(2 * H, H, 5) / np.sqrt(5 * H)).astype(np.float32), np.zeros(2 * H, np.float32), dev, mode=capi.MODE_GATED, bf16=True)
    res = packing.pack_conv((rs.randn(2 * H, H, 1) / np.sqrt(H)).astype(np.float32), np.zeros(2 * H, np.float32), dev, bf16=True)
    hs, out = torch.randn(R, 2 * H, device=dev), torch.empty(R, 2 * H, device=dev)
    cond = torch.randn(R, 8 * H, device=dev)[:, : 2 * H]
    acts = torch.empty(R, H, device=dev, dtype=torch.bfloat16)

    def t(fn, reps=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / reps

    fused = t(lambda: ops.wavenet_layer(inl, res, hs, out, cond, rag))

    def two():
        ops.conv(inl, hs[:, :H], acts, rag, preadd=cond, compute=capi.COMPUTE_BF16)
        ops.conv(res, acts, hs, rag, accumulate=True, compute=capi.COMPUTE_BF16)

    print(f"rows {R}: fused {fused:.1f} us   two launches {t(two):.1f} us   ({2 * R * H * 384 * 6 / fused / 1e6:.0f} TFLOP/s fused)")


if __name__ == "__main__":
    main()
