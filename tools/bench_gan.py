"""Speaker-embedding GAN throughput on the MI355X: the fixture generator (fixture_weights.GAN_PARAMS: size 16, nfilter 32,
nfilter_max 512) through gan.GeneratorEngine.  Prints one JSON line:

* embeddings/s at N = 1 (the GUI's call: latent upload, the launches, the result back), 1100 and 50 000 (latents already on the
  device, HIP-event time of the whole generator, chunked as the engine chunks);
* kernel time per layer at N = 1100 (HIP events around --steps launches of each layer alone) and the FLOP it does;
* GanWrapper.compute_controllability(50 000) split into the GPU intermediate (upload included), the device-to-host copy and the CPU
  PCA with lstsq;
* a yardstick: the same generator restated in eager torch (F.conv2d, F.batch_norm, F.interpolate) on the same GPU, fp32.

    python tools/bench_gan.py --steps 20 --warmup 3
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import controllable, gan, interface


def eager_generator(sd, params, dev):
    """ResNet_G.forward in eval mode restated from scratch with torch functional ops (the yardstick)."""
    sd = {k[len("module."):]: v.to(dev) for k, v in sd.items()}
    z_dim, data_dim, size, nf0, blocks = gan.architecture(params)
    bn = lambda x, p: F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)
    act = lambda x: F.leaky_relu(x, 0.2)

    def run(z):
        out = act(bn(F.linear(z, sd["fc.weight"], sd["fc.bias"]), "bn1d")).view(z.shape[0], nf0, 4, 4)
        for idx, fin, fout, upsampled in blocks:
            if upsampled:
                out = F.interpolate(out, scale_factor=2, mode="nearest")
            p = f"resnet.{idx}."
            xs = bn(F.conv2d(out, sd[p + "conv_s.weight"]), p + "bn2d_s") if fin != fout else out
            dx = act(bn(F.conv2d(out, sd[p + "conv_0.weight"], padding=1), p + "bn2d_0"))
            dx = bn(F.conv2d(dx, sd[p + "conv_1.weight"], padding=1), p + "bn2d_1")
            out = act(xs + 0.1 * dx)
        out = act(F.conv2d(out, sd["conv_img.weight"], sd["conv_img.bias"], padding=1))
        return F.linear(out.flatten(1), sd["fc_out.weight"], sd["fc_out.bias"])
    return run


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ctrl-samples", type=int, default=50000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        path = interface.write_fixture_gan_checkpoint(d)
        ck = torch.load(path, weights_only=True)
        wrapper = controllable.GanWrapper.__new__(controllable.GanWrapper)
        wrapper.device = dev
        wrapper.load_model(path)
    params, eng = ck["model_parameters"], wrapper.generator
    g = torch.Generator().manual_seed(0)
    flop = {l["name"]: 2 * l["h"] * l["h"] * l["cin"] * l["cout"] * l["taps"] for l in eng.plan["layers"]}
    flop_sample = sum(flop.values())
    out = {"metric": "gan_embeddings_per_s", "params": {k: params[k] for k in ("size", "nfilter", "nfilter_max", "z_dim")},
           "data_dim": eng.data_dim, "mflop_per_sample": round(flop_sample / 1e6, 2), "steps": args.steps, "chunk": eng.chunk}

    # N = 1: the GUI's modify_embed path, host latent in, host embedding out
    z1 = torch.randn((1, 32), generator=g)
    for _ in range(args.warmup):
        eng.forward(z1).cpu()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        eng.forward(z1).cpu()
        t.append((time.perf_counter() - t0) * 1e3)
    out["n1_ms_wall"] = round(float(np.median(t)), 4)
    out["n1_embeddings_per_s"] = round(1e3 / float(np.median(t)), 1)

    eager = eager_generator(ck["generator_state_dict"], params, dev)
    for n in (1100, 50000):
        zn = torch.randn((n, 32), generator=g).to(dev)
        steps = max(2, args.steps // (10 if n > 10000 else 1))
        ms = event_ms(lambda: eng.forward(zn), steps, min(args.warmup, 2))
        with torch.no_grad():
            ms_eager = event_ms(lambda: eager(zn), steps, min(args.warmup, 2))
            diff = float((eng.forward(zn) - eager(zn)).abs().max())
        out[f"n{n}_ms"] = round(ms, 4)
        out[f"n{n}_embeddings_per_s"] = round(n * 1e3 / ms, 1)
        out[f"n{n}_tflops"] = round(n * flop_sample / ms / 1e9, 2)
        out[f"n{n}_eager_torch_ms"] = round(ms_eager, 4)
        out[f"n{n}_speedup_vs_eager"] = round(ms_eager / ms, 2)
        out[f"n{n}_max_abs_diff_vs_eager"] = diff

    # per layer at N = 1100: each layer's launch alone, on the outputs of a full pass
    zn = torch.randn((1100, 32), generator=g).to(dev)
    outs = []
    for l in eng.layers:
        x = zn if l["src"] < 0 else outs[l["src"]]
        outs.append(eng._launch(l, x, 1100, None if l["res"] is None else outs[l["res"]]))
    layers = []
    for i, l in enumerate(eng.layers):
        x = zn if l["src"] < 0 else outs[l["src"]]
        r = None if l["res"] is None else outs[l["res"]]
        ms = event_ms(lambda: eng._launch(l, x, 1100, r), args.steps, args.warmup)
        layers.append({"layer": l["name"], "h": l["h"], "cin": l["cin"], "cout": l["cout"], "taps": l["taps"], "us": round(ms * 1e3, 2),
                       "tflops": round(1100 * flop[l["name"]] / ms / 1e9, 2)})
    out["n1100_layers"] = layers
    out["n1100_layer_sum_ms"] = round(sum(x["us"] for x in layers) / 1e3, 4)

    # compute_controllability(50 000): GPU intermediate, device-to-host copy, CPU PCA + lstsq
    torch.manual_seed(0)
    zc = torch.randn((args.ctrl_samples, eng.z_dim))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inter = eng.intermediate(zc)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    inter = inter.cpu()
    t2 = time.perf_counter()
    wrapper.controllable_speakers(inter, zc)
    t3 = time.perf_counter()
    out["ctrl_samples"] = args.ctrl_samples
    out["ctrl_gpu_intermediate_ms"] = round((t1 - t0) * 1e3, 2)
    out["ctrl_d2h_ms"] = round((t2 - t1) * 1e3, 2)
    out["ctrl_d2h_mb"] = round(inter.numel() * 4 / 2**20, 1)
    out["ctrl_cpu_pca_lstsq_ms"] = round((t3 - t2) * 1e3, 2)
    out["cpu_threads"] = torch.get_num_threads()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
