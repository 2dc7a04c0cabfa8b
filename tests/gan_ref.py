"""numpy restatement of include/toucan_gan.h (tts_gan_conv2d) and of the launch plan gan.pack_generator builds, in float64.

``conv2d`` computes what one launch computes; ``run_plan`` chains the launches as gan.GeneratorEngine does.  Checked against the
reference's own ResNet_G (tests/golden/gan/gan.npz) on the CPU, so the packing (BatchNorm folding, the fc row and fc_out column
permutations, the upsampled reads) is pinned without a GPU; the GPU tests hold the kernel to the same restatement.
"""
import numpy as np

from ims_toucan_prosody_variance_amd import capi

UPSAMPLE, PRE_LRELU, RESIDUAL, RES_UPSAMPLE, LRELU = (capi.GAN_UPSAMPLE, capi.GAN_PRE_LRELU, capi.GAN_RESIDUAL, capi.GAN_RES_UPSAMPLE,
                                                      capi.GAN_LRELU)


def lrelu(v, slope):
    return np.where(v > 0, v, v * slope)


def upsample2(x):
    """nearest x2 of NHWC [n, h, h, c]."""
    return x.repeat(2, axis=1).repeat(2, axis=2)


def conv2d(x, w, cin, cout, taps, h, flags=0, scale=None, shift=None, res=None, pre_slope=0.2, res_ratio=0.1, slope=0.2):
    """One tts_gan_conv2d in float64.  x: [n, hs, hs, cin] (hs = h/2 with UPSAMPLE); w: packed [taps][cin_pad][cout_pad];
    res: [n, h, h, cout] (or h/2 with RES_UPSAMPLE).  Returns [n, h, h, cout]."""
    x = np.asarray(x, np.float64)
    if flags & UPSAMPLE:
        x = upsample2(x)
    if flags & PRE_LRELU:
        x = lrelu(x, pre_slope)
    n = x.shape[0]
    assert x.shape == (n, h, h, cin)
    wk = np.asarray(w, np.float64)[:, :cin, :cout]
    if taps == 9:
        xp = np.zeros((n, h + 2, h + 2, cin))
        xp[:, 1:-1, 1:-1] = x
        v = sum(xp[:, t // 3:t // 3 + h, t % 3:t % 3 + h] @ wk[t] for t in range(9))
    else:
        v = x @ wk[0]
    if scale is not None:
        v = v * np.asarray(scale, np.float64)
    if shift is not None:
        v = v + np.asarray(shift, np.float64)
    if flags & RESIDUAL:
        r = np.asarray(res, np.float64)
        if flags & RES_UPSAMPLE:
            r = upsample2(r)
        v = r + res_ratio * v
    if flags & LRELU:
        v = lrelu(v, slope)
    return v


def run_plan(plan, z):
    """gan.GeneratorEngine.forward in float64: z [N, z_dim] -> [N, data_dim]."""
    z = np.asarray(z, np.float64)
    n, outs = z.shape[0], []
    for l in plan["layers"]:
        x = z if l["src"] < 0 else outs[l["src"]]
        hs = l["h"] // 2 if l["flags"] & UPSAMPLE else l["h"]
        x = x.reshape(n, hs, hs, l["cin"])
        r = None
        if l["res"] is not None:
            hr = l["h"] // 2 if l["flags"] & RES_UPSAMPLE else l["h"]
            r = outs[l["res"]].reshape(n, hr, hr, l["cout"])
        outs.append(conv2d(x, l["w"], l["cin"], l["cout"], l["taps"], l["h"], l["flags"], l["scale"], l["shift"], r))
    return outs[-1].reshape(n, -1)


def intermediate(plan, z):
    """GeneratorEngine.intermediate in float64: l_1 in the reference's (c, h, w) order."""
    l = plan["fc_ref"]
    z = np.asarray(z, np.float64)
    return conv2d(z.reshape(-1, 1, 1, l["cin"]), l["w"], l["cin"], l["cout"], 1, 1, l["flags"], l["scale"], l["shift"]).reshape(len(z), -1)
